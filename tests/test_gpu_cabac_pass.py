"""The CABAC pass on the GPU (x264hip_cabac_write_frame; ChainEncoder(cabac_pass=True): the wavefront variant of the sweep -- under adaptive
quantisation the raster variant without its writer -- and the slice written from the state behind it):

  * against the in-loop writer: the same options with cabac_pass=None (the raster variant with the writer in its loop) and cabac_pass=True;
    payload, payload_len, mb_bits, every array of the state the two sweeps leave and the filtered planes, every chain and frame;
  * against the REFERENCE's bytes and positions, tests/golden/cabac_pass_*.npz (tests/cabac_pass_cases.py);
  * encode_streams: a constant-QP CABAC stream is the same file with the pass forced, refused and selected by default;
  * what the entry point and ChainEncoder refuse, and a payload slot too small: a reported abort, nothing written behind the slot."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import cabac_pass_cases as cc
import edge_cases as ec
from oracle import refslice as rs
from paths import GOLDEN
from x264_vs2008_amd import encode as E
from x264_vs2008_amd import mux
from x264_vs2008_amd import slice as sl
from x264_vs2008_amd.abi import STATE_FIELDS, CabacParams
from x264_vs2008_amd.frame import DeviceArray, FrameCtx, cqm_init

pytestmark = pytest.mark.gpu

MED = dict(qp=26, me_method=rs.ME_HEX, subme=5, n_refs=3, inter=0x33, intra=0x3, transform8x8=1, mixed_refs=1, cabac=1, deblock=1)
STATE_KEYS = [f[0] for f in STATE_FIELDS]


def run(hip_lib, size, clips, n, cabac_pass, kw, ext=None, cqm=None, keep_state=True):
    """Every frame of a batch of chains: [frame]{payload [B] bytes, mb_bits [B][n_mb], state arrays, fin_y / fin_u / fin_v [B]}."""
    enc = sl.ChainEncoder(hip_lib, size[0], size[1], cqm or cqm_init(hip_lib), batch=len(clips), write=1, cabac_pass=cabac_pass, **kw, **(ext or {}))
    assert enc.cabac_pass == bool(cabac_pass) and enc.raster == bool(not cabac_pass or (ext or {}).get("aq_mode")), (enc.cabac_pass, enc.raster)
    assert enc.rd_opt["write"] == int(not cabac_pass)
    out = []
    try:
        for f in range(n):
            for b, (y, u, v) in enumerate(clips):
                enc.upload(y[f], u[f], v[f], b=b)
            _, _, state = enc.encode_frame()
            enc.status()
            r = dict(payload=enc.payloads(), mb_bits=enc.last_bufs["mb_bits"].get(), payload_len=enc.last_bufs["payload_len"].get())
            if keep_state:
                r.update({k: state.get(k) for k in STATE_KEYS})
            enc.finish_frame()
            enc.ctx.sync()
            if keep_state:
                for pl in "yuv":
                    r["fin_" + pl] = [enc.ctx.download(enc.refs[0][0], pl, padded=False, b=b) for b in range(len(clips))]
            out.append(r)
    finally:
        enc.close()
    return out


def same(tag, a, b):
    for f, (ra, rb) in enumerate(zip(a, b)):
        for k in ra:
            if k == "payload":
                for c, (pa, pb) in enumerate(zip(ra[k], rb[k])):
                    assert pa == pb, "%s frame %d chain %d: payload differs (%d vs %d bytes)" % (tag, f, c, len(pa), len(pb))
            elif k.startswith("fin_"):
                for c, (pa, pb) in enumerate(zip(ra[k], rb[k])):
                    assert np.array_equal(pa, pb), "%s frame %d chain %d: plane %s differs" % (tag, f, c, k)
            else:
                assert np.array_equal(ra[k], rb[k]), "%s frame %d: %s differs" % (tag, f, k)


def test_pass_equals_in_loop_writer_batch_of_moving_chains(hip_lib):
    clips = [rs.clip(96, 80, 4, t0) for t0 in (0, 13, 29)]
    same("moving", run(hip_lib, (96, 80), clips, 4, None, MED), run(hip_lib, (96, 80), clips, 4, True, MED))


@pytest.mark.parametrize("size", ec.SIZES, ids=ec.size_id)
def test_pass_equals_in_loop_writer_edge_pictures(hip_lib, size):
    clips = [ec.clip(kind, size, 3) for kind in ("noise", "satnoise", "flat0")]
    same(ec.size_id(size), run(hip_lib, size, clips, 3, None, MED), run(hip_lib, size, clips, 3, True, MED))


@pytest.mark.parametrize("size", cc.QP1_SIZES, ids=ec.size_id)
def test_pass_equals_in_loop_writer_at_qp1(hip_lib, size):
    """Lossy QP 1 (the I slice at QP 0, which is not lossless): levels beyond 2900, deep in the Exp-Golomb tail of coeff_abs_level_minus1, in
    both writers.  The same chains against the reference's bytes: test_pass_equals_reference_fixture's qp1_* cases."""
    clips = [ec.clip(kind, size, 3) for kind in cc.QP1_KINDS]
    loop = run(hip_lib, size, clips, 3, None, cc.QP1_KW)
    top = max(int(np.abs(r[k].astype(np.int32)).max()) for r in loop for k in ("luma", "luma_dc", "chroma_dc", "chroma_ac"))
    assert top >= cc.QP1_LEVEL, "largest |level| %d" % top
    same("qp1 " + ec.size_id(size), loop, run(hip_lib, size, clips, 3, True, cc.QP1_KW))


def test_pass_equals_in_loop_writer_adaptive_quantisation(hip_lib):
    clips = [rs.clip(96, 80, 4, t0) for t0 in (0, 5)]
    kw, ext = dict(MED, qp=30, n_refs=2), dict(aq_mode=1, aq_strength=1.5)
    same("aq", run(hip_lib, (96, 80), clips, 4, None, kw, ext), run(hip_lib, (96, 80), clips, 4, True, kw, ext))


def test_pass_equals_in_loop_writer_empty_i16_behind_a_qp_change(hip_lib):
    """cabac_pass_cases' aq_empty_i16: I_16x16 macroblocks without coefficients behind macroblocks of another QP.  The writer gives such a
    macroblock the previous QP, which the next macroblock's QP rule and the loop filter read: the raster variant without its writer must leave
    the same qp array and the same filtered planes as the one with it."""
    c = cc.CASES["aq_empty_i16"]
    clips = [cc.clip_of(c), cc.clip_of(c, live=True)]
    loop = run(hip_lib, c["size"], clips, c["n"], None, c["kw"], c["ext"])
    assert sum(int(((r["mb_type"] == sl.I_16x16) & (r["cbp"] == 0)).sum()) for r in loop) >= 16
    same("aq_empty_i16", loop, run(hip_lib, c["size"], clips, c["n"], True, c["kw"], c["ext"]))


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_pass_equals_reference_fixture(hip_lib, name):
    c, gold = cc.CASES[name], cc.fixture(name)
    cqm = None
    if c["kw"].get("cqm_preset"):                      # --cqm jvt: the quantiser tables x264_cqm_init builds for the JVT matrices
        with np.load(os.path.join(GOLDEN, "cqm_jvt.npz")) as z:
            cqm = {k: z[k] for k in z.files}
    kw = {k: v for k, v in c["kw"].items() if k != "cqm_preset"}
    got = run(hip_lib, c["size"], [cc.clip_of(c)], c["n"], True, kw, c.get("ext"), cqm, keep_state=False)
    for f in range(c["n"]):
        want = bytes(gold["payload"][f, :gold["payload_len"][f]])
        assert got[f]["payload"][0] == want, "%s frame %d: payload differs (%d vs %d bytes)" % (name, f, len(got[f]["payload"][0]), len(want))
        assert np.array_equal(got[f]["mb_bits"][0], gold["mb_bits"][f]), "%s frame %d: mb_bits differ" % (name, f)


class Clip:
    def __init__(self, y, u, v):
        self.planes = (y, u, v)

    def read(self, t):
        return tuple(p[t] for p in self.planes)


def test_encode_streams_same_file_with_and_without_the_pass(hip_lib, monkeypatch):
    w, h, n = 96, 80, 5
    args = "--qp 26 --scenecut -1 --bframes 0 --ref 2 --me hex --subme 5 --8x8dct --mixed-refs --aq-mode 0 --keyint 3 --min-keyint 1".split()
    o = E.build_parser().parse_args(args + ["-o", "x", "in_96x80.yuv"])
    p = mux.encoder_params(hip_lib, width=w, height=h, fps_num=25, fps_den=1, **E.param_fields(o))
    assert p.cabac and not E.needs_lookahead(p)
    built = []
    real = sl.ChainEncoder

    def spy(*a, **k):
        built.append(real(*a, **k))
        return built[-1]
    monkeypatch.setattr(sl, "ChainEncoder", spy)
    files = {}
    for mode in (True, False, None):
        sink = io.BytesIO()
        assert E.encode_streams(hip_lib, p, [Clip(*rs.clip(w, h, n, 7))], n, [sink], cabac_pass=mode) == n
        files[mode] = sink.getvalue()
    assert [e.cabac_pass for e in built] == [True, False, True] and [e.raster for e in built] == [False, True, False]
    assert len(files[True]) > 500 and files[True] == files[False], "forced pass vs in-loop writer: %d vs %d bytes" % (len(files[True]), len(files[False]))
    assert files[None] == files[False], "the default's file differs"


def test_chain_encoder_refuses_what_the_pass_does_not_go_with(hip_lib):
    cqm = cqm_init(hip_lib)
    for bad in (dict(subme=6), dict(trellis=1), dict(bframes=2, inter=0x133), dict(qp=0, fast_pskip=0), dict(levels=False), dict(lanes=2), dict(cabac=0), dict(write=0)):
        with pytest.raises(ValueError) as e:
            sl.ChainEncoder(hip_lib, 96, 80, cqm, **dict(dict(MED, write=1, cabac_pass=True), **bad))
        assert "cabac_pass" in str(e.value), bad


def test_entry_point_refusals_and_slot_too_small(hip_lib):
    """Refused before any launch: a B slice, a state without level arrays, payload buffers missing or below one macroblock's worst case.  A
    slot of X264HIP_PAYLOAD_LEAD + SW_MB_BYTES_MAX + 128 bytes on a noisy low-QP picture: the pass stops before the macroblock that might not
    fit, the status call reports the abort, and the bytes behind the slot (the next chain's slot, filled with a pattern) stay as they were."""
    size, cap = (40, 24), sl.PAYLOAD_LEAD + sl.MB_BYTES_MAX + 128
    y, u, v = ec.clip("noise", size, 1)
    enc = sl.ChainEncoder(hip_lib, size[0], size[1], cqm_init(hip_lib), write=1, cabac_pass=True, payload_cap=cap, **dict(MED, qp=4))
    bare = sl.DeviceState(enc.ctx, levels=False)
    guard = DeviceArray(hip_lib, (2, cap), np.uint8, np.full((2, cap), 0xA5, np.uint8))
    plen = DeviceArray(hip_lib, (2,), np.int32)
    try:
        enc.upload(y[0], u[0], v[0])
        _, qp, state = enc.encode_frame()
        with pytest.raises(RuntimeError) as e:
            enc.status()
        assert "out of payload space" in str(e.value)
        assert enc.last_bufs["payload_len"].get()[0] == 0

        def call(st, **k):
            bp = CabacParams(**dict(dict(slice_type=sl.SLICE_I, n_ref0=0, analyse_inter=0x33, transform8x8=1, slice_qp=qp, cabac_init_idc=0, i_frame=0,
                                         i_frame_stride=0, payload=guard.ptr, payload_cap=cap, payload_len=plen.ptr, mb_bits=None), **k))
            return hip_lib.x264hip_cabac_write_frame(enc.ctx.h, C.byref(st), C.byref(bp)), hip_lib.x264hip_last_error().decode()
        for k, word in ((dict(slice_type=sl.SLICE_B), "B slices"), (dict(payload=None), "payload buffers"), (dict(payload_len=None), "payload buffers"),
                        (dict(payload_cap=sl.MB_BYTES_MAX + 127), "payload buffers")):
            rc, msg = call(state.st, **k)
            assert rc == -1 and word in msg, (k, msg)
        rc, msg = call(bare.st)
        assert rc == -1 and "coefficient levels" in msg, msg
        wide = FrameCtx(hip_lib, 16 * 513, 16)             # one row of 513 macroblocks: beyond the pass's row of mvd
        wide_state = sl.DeviceState(wide)
        try:
            bp = CabacParams(slice_type=sl.SLICE_I, transform8x8=1, slice_qp=qp, payload=guard.ptr, payload_cap=cap, payload_len=plen.ptr)
            assert hip_lib.x264hip_cabac_write_frame(wide.h, C.byref(wide_state.st), C.byref(bp)) == -1
            assert "macroblocks per row" in hip_lib.x264hip_last_error().decode()
        finally:
            wide_state.free()
            wide.close()
        # the same slice into chain 0's slot of a two-slot buffer: slot 1 is what lies behind it
        rc, msg = call(state.st)
        assert rc == 0, msg
        enc.ctx.sync()
        raw = guard.get()
        assert (raw[1] == 0xA5).all(), "the pass wrote behind its slot"
        assert (raw[0, sl.PAYLOAD_LEAD:] != 0xA5).any() and plen.get()[0] == 0
    finally:
        for d in (guard, plen):
            d.free()
        bare.free()
        enc.close()
