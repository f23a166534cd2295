"""CPU: psy-trellis (--psy-rd A:B) outside the kernels -- the validated command line reaches the encoders with the reference's fixed-point
strength and chroma QP offset (R/encoder/encoder.c:502-522, restated in psy_trellis_cases.validated); the fixtures equal the live reference
where it is built; the scalar trellis quantiser's new entry with the strength at 0 is the old entry."""
import os

import numpy as np
import pytest

import psy_trellis_cases as PC
from paths import REF_SO
from x264_vs2008_amd import encode as E
from x264_vs2008_amd import mux, slice as sl


class Reached(Exception):
    pass


@pytest.mark.parametrize("args", ["--trellis 1 --psy-rd 1.0:0.15", "--trellis 1 --psy-rd 0.1:0.3 --chroma-qp-offset -11", "--trellis 2 --subme 6 --bframes 2 --psy-rd 1.0:1.0"])
def test_command_line_takes_psy_trellis_with_either_trellis(hip_lib_host, args):
    """Nothing about psy-trellis is left for encode.check_built to refuse: trellis 1, and trellis 2 where a B slice is below the RD levels while the
    P slices are not, are built (x264hip_slice_rd.psy_carry)."""
    o = E.build_parser().parse_args(("--crf 23 " + args).split() + ["-o", "x.264", "in_96x80.yuv"])
    p = mux.encoder_params(hip_lib_host, width=96, height=80, **E.param_fields(o))
    E.check_built(p)
    assert sl.psy_trellis_fix8(p.psy_trellis) > 0


@pytest.mark.parametrize("args,trellis,strength", [
    ("--trellis 1 --psy-rd 1.0:0.15", 1, 0.15), ("--trellis 2 --psy-rd 0.6:1.0", 2, 1.0),
    ("--trellis 2 --psy-rd 1.0:0.15 --bframes 0", 2, 0.15), ("--trellis 1 --psy-rd 0.6:1.0 --subme 7", 1, 1.0),
    ("--trellis 1 --psy-rd 1.0:0.15 --no-cabac --subme 5", 0, 0.0), ("--trellis 2 --psy-rd 0.6:1.0 --no-cabac --subme 5", 0, 0.0),
    ("--trellis 0 --psy-rd 1.0:0.15", 0, 0.0), ("--trellis 0 --psy-rd 0.6:1.0", 0, 0.0),
    ("--trellis 2 --psy-rd 0.1:0.3 --chroma-qp-offset -11 --subme 7", 2, 0.3), ("--trellis 2 --psy-rd 1.0:40 --bframes 0 --scenecut -1 --qp 30", 2, 10.0)])
def test_command_line_hands_the_encoders_the_validated_strength(hip_lib_host, monkeypatch, args, trellis, strength):
    """encode_streams with the encoder classes replaced by a recorder: what would be given, and what ChainEncoder makes of it (rd_side_options)."""
    seen = {}

    def recorder(lib, w, h, cq, **kw):
        seen.update(kw)
        raise Reached()

    from x264_vs2008_amd import stream
    monkeypatch.setattr(sl, "ChainEncoder", recorder)
    monkeypatch.setattr(stream, "StreamEncoder", recorder)
    if "--qp" not in args:
        args = "--crf 23 " + args                   # (a rate control has to be named: without one the parameters validate as for QP 0)
    o = E.build_parser().parse_args(args.split() + ["-o", "x.264", "in_96x80.yuv"])
    p = mux.encoder_params(hip_lib_host, width=96, height=80, **E.param_fields(o))

    class Src:
        w, h = 96, 80
    with pytest.raises(Reached):
        E.encode_streams(hip_lib_host, p, [Src()], 1, [None])
    assert abs(seen["psy_trellis"] - strength) < 1e-6 and seen["trellis"] == trellis
    got = sl.rd_side_options(seen["cabac"], seen["subme"], seen["trellis"], seen["psy_rd"], seen["psy_trellis"], seen["chroma_qp_offset"])
    # the reference's lines on the command line's own values
    pr = [float(x) for x in o.psy_rd.split(":")]
    fix, off = PC.validated(o.trellis, not o.no_cabac, o.subme, pr[0], pr[1], o.chroma_qp_offset)
    assert got[2] == fix and got[3] == off, "encoders: (i_psy_trellis, chroma_qp_offset) %s, x264_validate_parameters %s" % ((got[2], got[3]), (fix, off))
    assert got[3] == p.chroma_qp_offset                         # ... which is also what the PPS carries
    assert fix == {0.0: 0, 0.15: 10, 0.3: 19, 1.0: 64, 10.0: 640}[strength]
    assert abs(p.psy_trellis - strength) < 1e-6 and ("psy_rd=%.1f:%.1f" % (p.psy_rd, p.psy_trellis)).encode() in mux.headers(hip_lib_host, p)      # the SEI says the same


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libx264ref.so not built (the fixtures hold the same chains)")
@pytest.mark.parametrize("name,size,frames,kind,kw,ekw", PC.PT_CASES, ids=[c[0] for c in PC.PT_CASES])
def test_fixture_equals_the_live_reference(name, size, frames, kind, kw, ekw):
    gold, live = PC.load(name), PC.to_fixture(PC.reference_chain(size, frames, kind, kw, ekw))
    assert sorted(gold) == sorted(live)
    for k in gold:
        assert np.array_equal(gold[k], live[k]), k


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libx264ref.so not built (the fixture holds the same stream)")
def test_stream_fixture_equals_the_live_reference(hip_lib_host):
    with np.load(PC.fixture_path("stream")) as z:
        gold = {k: z[k] for k in z.files}
    a, n = PC.cli_reference(PC.cli_params(hip_lib_host)), PC.CLI_CLIP["n"]
    for k in PC.STREAM_KEYS:
        assert np.array_equal(gold[k], a[k][:n]), k


def zigzag8():
    """x264_zigzag_scan8[0]: scan position -> index in the transposed storage (R/common/dct.c ZIGZAG8_FRAME)."""
    order = sorted(((y, x) for y in range(8) for x in range(8)), key=lambda t: (t[0] + t[1], t[0] if (t[0] + t[1]) % 2 == 0 else t[1]))
    return np.array([x * 8 + y for y, x in order], np.uint8)


@pytest.mark.parametrize("n_coef,cat,b_ac", [(16, 2, 0), (16, 1, 1), (64, 5, 0)])
def test_scalar_trellis_with_strength_zero_is_the_old_entry(hip_lib_host, n_coef, cat, b_ac):
    """Seeded random blocks through td_trellis_quant's twelve-argument entry and through the psy-trellis entry: equal at strength 0 whatever
    the source coefficients say; and the strength does something."""
    import ctypes as C
    from psy_trellis_host_util import host_trellis
    from x264_vs2008_amd.frame import cqm_init
    H, cq = host_trellis(), cqm_init(hip_lib_host)
    zz = np.array([0, 4, 1, 2, 5, 8, 12, 9, 6, 3, 7, 10, 13, 14, 11, 15], np.uint8) if n_coef == 16 else zigzag8()
    assert sorted(zz.tolist()) == list(range(n_coef))
    r = np.random.default_rng(1000 + n_coef + cat)
    st = np.zeros(460, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    moved = 0
    for it in range(200):
        qp = int(r.integers(10, 45))
        if it % 20 == 0:
            H.pt_host_context_init(p(st), 0, qp, 0)
        mf = np.ascontiguousarray((cq["quant4_mf"][1] if n_coef == 16 else cq["quant8_mf"][1])[qp], np.uint16)
        unq = np.ascontiguousarray((cq["unquant4_mf"][1] if n_coef == 16 else cq["unquant8_mf"][1])[qp], np.int32)
        weight = r.integers(100, 900, n_coef).astype(np.int32)
        scale = int(r.choice([8, 40, 200, 1200]))
        dct = (r.standard_normal(n_coef) * scale / (1 + np.arange(n_coef) / 4.0)).astype(np.int16)[np.argsort(zz)]
        fenc = (dct[zz].astype(np.int32) + r.integers(-300, 300, n_coef)).astype(np.int16)          # scan order
        lam = int(r.integers(50, 200000))
        a, b, c = dct.copy(), dct.copy(), dct.copy()
        nz_a = H.pt_host_trellis(p(a), p(mf), p(unq), p(weight), p(zz), p(st), cat, lam, b_ac, 0, n_coef)
        nz_b = H.pt_host_trellis_psy(p(b), p(mf), p(unq), p(weight), p(zz), p(st), cat, lam, b_ac, 0, n_coef, p(fenc), 0)
        assert nz_a == nz_b and np.array_equal(a, b), "block %d: strength 0 is not the old entry" % it
        H.pt_host_trellis_psy(p(c), p(mf), p(unq), p(weight), p(zz), p(st), cat, lam, b_ac, 0, n_coef, p(fenc), 64)
        moved += int(not np.array_equal(a, c))
    assert moved > 0, "strength 64 changed no block"
