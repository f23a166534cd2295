"""GPU: psy-trellis (--psy-rd A:B with B > 0 under --trellis 1 / 2) in the raster-order sweep -- I, P and B slices, below the RD levels, with
the RD mode decision and with the RD refinement -- against chains the REFERENCE's own loop produced with h->mb.i_psy_trellis set
(oracle/ref_slice.c; fixtures tests/golden/pt_*.npz, made by tests/psy_trellis_cases.py): every decision, every level, mb_bits, the payload
bytes and the planes.  Lock-step launches (x264hip_slice_sweep_frame), a batch, the chain table (x264hip_slice_sweep_chains), the frame
queue (StreamEncoder) and the command line.

Without the feature every chain test here fails with ChainEncoder's unexpected-keyword error for psy_trellis."""
import hashlib
import os

import numpy as np
import pytest

import psy_trellis_cases as PC
from mux_cases import mux_reference_stream, write_clip
from oracle.gen_golden_slice import case_inputs
from paths import REF_SO
from slice_util import run_chain2
from psy_table_util import ViaTable
from table_util import table_launch
from x264_vs2008_amd import encode as E
from x264_vs2008_amd import slice as sl
from x264_vs2008_amd.frame import DeviceArray

pytestmark = pytest.mark.gpu
STATE = [k for k in PC.WHOLE if k not in ("mvr", "frame_info", "frame_info2", "stat", "payload_len", "mb_bits", "mv1", "ref1")]


def check_frame(d, gold, f, b=0, what=""):
    """One frame of one chain against the fixture (or the live reference's arrays put through psy_trellis_cases.to_fixture)."""
    stype, qp = int(gold["frame_info"][f][0]), int(gold["frame_info"][f][1])
    assert d["info"] == (stype, qp), "%sframe %d: slice type / QP %s, the reference %s" % (what, f, d["info"], (stype, qp))
    for k in STATE + (["mv1", "ref1"] if stype == sl.SLICE_B else []):
        if stype == sl.SLICE_I and k in ("mv", "ref"):
            continue
        got, want = d[k][b], gold[k][f]
        assert np.array_equal(got.reshape(want.shape), want), "%sframe %d: %s differs first at %s" % (what, f, k, np.argwhere(got.reshape(want.shape) != want)[:3].tolist())
    if stype != sl.SLICE_B:
        skip = gold["mb_type"][f] == sl.P_SKIP
        for r in range(int(gold["frame_info"][f][2])):
            assert np.array_equal(d["mvr"][b][r][~skip], gold["mvr"][f][r][~skip]), "%sframe %d: mvr[%d]" % (what, f, r)
        assert int(d["cost_intra"][b].sum()) == int(gold["stat"][f][0]) and int(d["cost_inter"][b].sum()) == int(gold["stat"][f][1]), "%sframe %d: statistics" % (what, f)
    want_bits = gold["mb_bits"][f]
    assert np.array_equal(d["mb_bits"][b], want_bits), "%sframe %d: mb_bits differ first at macroblock %s" % (what, f, np.argwhere(d["mb_bits"][b] != want_bits)[:1].tolist())
    pay = d["payload"][b]
    assert len(pay) == int(gold["payload_len"][f]), "%sframe %d: payload %d bytes, the reference %d" % (what, f, len(pay), int(gold["payload_len"][f]))
    assert hashlib.md5(pay).hexdigest() == str(gold["payload_md5"][f]), "%sframe %d: payload bytes differ" % (what, f)
    for nm in ("y", "u", "v"):
        for kind in ("rec_",) if stype == sl.SLICE_B else ("rec_", "fin_"):        # (a disposable B frame is never filtered)
            assert PC.md5(d[kind + nm][b]) == str(gold[kind + nm + "_md5"][f]), "%sframe %d: %s%s differs from the reference" % (what, f, kind, nm)


@pytest.mark.parametrize("name,size,frames,kind,kw,ekw", PC.PT_CASES, ids=[c[0] for c in PC.PT_CASES])
def test_psy_trellis_chain_matches_reference(hip_lib, cqm, name, size, frames, kind, kw, ekw):
    gold = PC.load(name)
    y, u, v = case_inputs(size, frames, kind)
    out = run_chain2(hip_lib, cqm, size, frames, y, u, v, kw, ekw)
    for f in range(frames):
        check_frame(out[f], gold, f)
    st = gold["frame_info"][:, 0].tolist()
    assert sl.SLICE_I in st and sl.SLICE_P in st and ((sl.SLICE_B in st) == bool(ekw.get("bframes")))


@pytest.mark.parametrize("name", ["t1_s7", "t2_s8", "t1_s8"])
def test_chain_table_all_psy_trellis(hip_lib, cqm, name):
    """x264hip_slice_sweep_chains with psy-trellis in every chain (the table kernels: I / P, I / P with the RD refinement): the fixture's bytes in every
    chain -- with trellis 1 every chain against its own slot of x264hip_slice_rd.psy_carry."""
    _, size, frames, kind, kw, ekw = PC.PT_BY_NAME[name]
    gold = PC.load(name)
    y, u, v = case_inputs(size, frames, kind)
    out = table_launch(hip_lib, cqm, size, frames, y, u, v, dict(kw, **ekw), [kw["qp"]] * 3)
    for f in range(frames):
        for b in range(3):
            assert np.array_equal(out[f]["mb_type"][b], gold["mb_type"][f]), "frame %d chain %d: mb_type" % (f, b)
            assert np.array_equal(out[f]["mb_bits"][b], gold["mb_bits"][f]), "frame %d chain %d: mb_bits" % (f, b)
            assert hashlib.md5(out[f]["payload"][b]).hexdigest() == str(gold["payload_md5"][f]), "frame %d chain %d: payload" % (f, b)
            for i, nm in enumerate(("y", "u", "v")):
                assert PC.md5(out[f]["rec"][i][b]) == str(gold["rec_%s_md5" % nm][f]) and PC.md5(out[f]["fin"][i][b]) == str(gold["fin_%s_md5" % nm][f]), "frame %d chain %d: %s" % (f, b, nm)


def test_chain_table_extended_b_kernel_three_chains(hip_lib, cqm):
    """The B chain with temporal direct prediction as a table of three chains (psy_table_util.ViaTable: table_launch knows I and P slices only): every
    frame of every chain against the fixture, the B frames through the chain-table launch of the extended B kernel."""
    name, size, frames, kind, kw, ekw = PC.PT_BY_NAME["t2_s7_bt"]
    gold = PC.load(name)
    y, u, v = case_inputs(size, frames, kind)
    via = ViaTable(hip_lib, 3)
    try:
        out = run_chain2(via, cqm, size, frames, y, u, v, kw, ekw, batch=3)
    finally:
        via.free()
    assert via.launches == frames
    assert sl.SLICE_B in gold["frame_info"][:, 0].tolist()
    for f in range(frames):
        for b in range(3):
            check_frame(out[f], gold, f, b=b, what="chain %d " % b)


def test_three_chains_with_different_content_in_one_launch(hip_lib, cqm):
    """Chain b codes the clip rotated by b frames: the fixture where the rotation is the identity, the live reference (where it is built) for the
    others -- each group of sixteen lanes reads its own block's sign and source coefficient, each chain its own source."""
    name, size, frames, kind, kw, ekw = PC.PT_BY_NAME["t2_s7"]
    gold = PC.load(name)
    y, u, v = case_inputs(size, frames, kind)
    rot = [np.roll(np.arange(frames), -b) for b in range(3)]
    live = os.path.exists(REF_SO)
    want = [gold] + [PC.to_fixture(PC.reference_chain_of(size, kw, ekw, y[rot[b]], u[rot[b]], v[rot[b]])) if live else None for b in (1, 2)]
    enc = sl.ChainEncoder(hip_lib, size[0], size[1], cqm, batch=3, write=1, **kw, **ekw)
    try:
        for f in range(frames):
            for b in range(3):
                t = (f + b) % frames
                enc.upload(y[t], u[t], v[t], b=b)
            stype, qp, state = enc.encode_frame()
            enc.status()
            recon = enc.last[0]
            d = {k: state.get(k) for k in STATE + ["mvr", "cost_intra", "cost_inter"]}
            d["info"], d["payload"], d["mb_bits"] = (stype, qp), enc.payloads(), enc.rd_bufs["mb_bits"].get()
            for nm in ("y", "u", "v"):
                d["rec_" + nm] = np.stack([enc.ctx.download(recon, nm, padded=False, b=b) for b in range(3)])
            enc.finish_frame()
            enc.ctx.sync()
            for nm in ("y", "u", "v"):
                d["fin_" + nm] = np.stack([enc.ctx.download(recon, nm, padded=False, b=b) for b in range(3)])
            for b in range(3):
                if want[b] is not None:
                    check_frame(d, want[b], f, b=b, what="chain %d " % b)
                else:
                    assert len(d["payload"][b]) > 0
    finally:
        enc.close()


def test_chain_table_mixing_psy_trellis_on_and_off_is_refused(hip_lib, cqm):
    """No kernel is launched: the table is refused while it is built (a launch would leave the abort flag or the payload lengths touched)."""
    from x264_vs2008_amd.stream import ChainSweep
    import ctypes as C
    from x264_vs2008_amd.frame import DeviceArray
    _, size, frames, kind, kw, ekw = PC.PT_BY_NAME["t2_s7"]
    y, u, v = case_inputs(size, 1, kind)
    on = sl.ChainEncoder(hip_lib, size[0], size[1], cqm, batch=2, write=1, **kw, **ekw)
    off = sl.ChainEncoder(hip_lib, size[0], size[1], cqm, batch=2, write=1, **kw, **dict(ekw, psy_trellis=0.0))
    lib, c = hip_lib, on.ctx
    tb = lib.x264hip_chain_sweep_bytes()
    tab_host, tab_dev = lib.x264hip_host_alloc(tb * 2), DeviceArray(lib, (tb * 2,), np.uint8)
    try:
        assert on.psy_trellis_fix == 64 and off.psy_trellis_fix == 0
        for b in range(2):
            on.upload(y[0], u[0], v[0], b=b)
        recon, state = on.pool[0], on.states[0]
        entries, keep = (ChainSweep * 2)(), []
        qp = sl.iframe_qp(kw["qp"])
        for b, e in enumerate((on, off)):
            p = e.slice_params(sl.SLICE_I, qp, 0, e.cost_table(qp).ptr, None)
            rd = e.slice_rd(dict(e.rd_bufs, payload=on.rd_bufs["payload"], payload_len=on.rd_bufs["payload_len"], mb_bits=on.rd_bufs["mb_bits"], stale=on.rd_bufs["stale"]),
                            float(qp), 0, None, 1, 0)
            rd.payload_cap = on.payload_cap
            p.rd = C.addressof(rd)
            keep += [p, rd]
            entries[b] = ChainSweep(chain=b, fenc=C.addressof(on.fenc), refs=None, n_refs=0, recon=C.addressof(recon), params=C.addressof(p), l0=None, out=C.addressof(state.st))
        c.check(lib.x264hip_mb_state_clear_progress(c.h, C.byref(state.st)), "mb_state_clear_progress")
        before = state.get("mb_type").copy()
        with pytest.raises(RuntimeError, match="all-psy-trellis or not at all"):
            c.check(lib.x264hip_slice_sweep_chains(c.h, entries, 2, tab_host, tab_dev.p), "slice_sweep_chains")
        c.sync()
        assert np.array_equal(state.get("mb_type"), before), "a kernel wrote the state of a refused table"
    finally:
        c.sync()
        tab_dev.free()
        lib.x264hip_host_free(tab_host)
        on.close()
        off.close()


@pytest.mark.parametrize("what,needle", [("no_trellis", "without trellis"), ("lossless", "lossless with psy-trellis")])
def test_psy_trellis_preconditions_are_refused(hip_lib, cqm, what, needle):
    """What x264_validate_parameters turns off is the caller's precondition (ChainEncoder applies it; here it is put back by hand)."""
    y, u, v = case_inputs((96, 80), 1, "moving")
    enc = sl.ChainEncoder(hip_lib, 96, 80, cqm, qp=0 if what == "lossless" else 26, subme=6, me_method=1, n_refs=1, inter=0x13, intra=0x3, transform8x8=1, cabac=1, write=1,
                          trellis=0, psy_trellis=1.0)
    try:
        assert enc.psy_trellis_fix == 0 and enc.rd_opt["trellis"] == 0
        enc.psy_trellis_fix = 64
        enc.rd_bufs["psy_carry"] = DeviceArray(hip_lib, (1, 512), np.int16)
        enc.upload(y[0], u[0], v[0])
        with pytest.raises(RuntimeError) as e:
            enc.encode_frame()
        assert "psy-trellis" in str(e.value) and needle in str(e.value), str(e.value)
    finally:
        enc.close()


def test_psy_trellis_without_its_carry_is_refused(hip_lib, cqm):
    """x264hip_slice_rd.psy_carry is where a chain keeps h->mb.pic.fenc_dct4 / fenc_dct8 between macroblocks and frames: required."""
    name, size, frames, kind, kw, ekw = PC.PT_BY_NAME["t1_s7"]
    y, u, v = case_inputs(size, 1, kind)
    enc = sl.ChainEncoder(hip_lib, size[0], size[1], cqm, write=1, **kw, **ekw)
    try:
        carry = enc.rd_bufs.pop("psy_carry")
        enc.upload(y[0], u[0], v[0])
        with pytest.raises(RuntimeError, match="psy_carry"):
            enc.encode_frame()
    finally:
        enc.close()
        carry.free()


def stream_records(hip_lib, psy_trellis):
    """The command line's clip and settings through StreamEncoder: [(input number, slice type, qp, payload)] in coding order."""
    from x264_vs2008_amd.frame import cqm_init
    from x264_vs2008_amd.stream import StreamEncoder
    from oracle import refslice as rs
    c = PC.CLI_CLIP
    y, u, v = rs.clip(c["w"], c["h"], c["n"], c["t0"])
    p = PC.cli_params(hip_lib)
    enc = StreamEncoder(hip_lib, c["w"], c["h"], cqm_init(hip_lib), batch=1, crf=23.0, b_adapt=1, bframe_bias=p.bframe_bias, keyint_min=p.keyint_min,
                        scenecut_threshold=p.scenecut_threshold, pre_scenecut=p.pre_scenecut, qp=p.qp_constant, me_method=p.me_method, me_range=p.me_range,
                        subme=p.subpel_refine, n_refs=p.frame_reference, inter=p.inter, intra=p.intra, transform8x8=p.transform_8x8, cabac=1, deblock=1,
                        keyint=p.keyint_max, mixed_refs=p.mixed_references, chroma_me=p.chroma_me, mv_range=p.mv_range, trellis=p.trellis, psy_rd=1.0, psy_trellis=psy_trellis,
                        aq_mode=1, aq_strength=p.aq_strength, bframes=2, weightb=1, direct_pred=p.direct_mv_pred, qp_min=p.qp_min, qp_max=p.qp_max)
    got, fed, idle, frames = [], 0, 0, c["n"]
    try:
        def fill(pic, f):
            enc.src_ctx.upload(pic, y[f], u[f], v[f], b=0)
        for _ in range(4 * frames + 40):
            coded = enc.step(fill if fed < frames else None)
            fed += fed < frames
            idle = 0 if coded else idle + (fed >= frames and enc.flushing)
            if idle >= 2:
                break
            if coded:
                enc.sync()
                enc.status()
                pl = enc.payloads()
                got += [(cd.frame, cd.slice_type, cd.qp, pl[cd.chain]) for cd in coded]
    finally:
        enc.close()
    return got


def test_stream_encoder_with_psy_trellis_equals_the_reference_encoder(hip_lib):
    """crf 23, bframes 2, b_adapt 1, weightb, aq_mode 1, trellis 1, psy_rd 1.0, psy_trellis 0.15 at 112x96, 10 frames: frame order, types, QPs, payload
    bytes (the chain-table launches: I / P kernels and the extended B kernel)."""
    with np.load(PC.fixture_path("stream")) as z:
        gold = {k: z[k] for k in z.files}
    got, n = stream_records(hip_lib, 0.15), PC.CLI_CLIP["n"]
    assert len(got) == n
    st = gold["frame_info"][:n, 0].tolist()
    assert sl.SLICE_I in st and sl.SLICE_P in st and sl.SLICE_B in st
    for f, (frame, stype, qp, payload) in enumerate(got):
        ref = (int(gold["frame_info2"][f][0]), int(gold["frame_info"][f][0]), int(gold["frame_info"][f][1]))
        assert (frame, stype, qp) == ref, "coded frame %d: (input, slice, qp) %s, the reference %s" % (f, (frame, stype, qp), ref)
        want = bytes(gold["payload"][f, :gold["payload_len"][f]])
        assert hashlib.md5(payload).hexdigest() == hashlib.md5(want).hexdigest(), "coded frame %d (input %d, slice %d, qp %d): payload differs (%d vs %d bytes)" % (f, frame, stype, qp, len(payload), len(want))


def test_command_line_with_psy_trellis(hip_lib, tmp_path):
    """The same clip as a y4m through the command line: the .264 is the harness's payloads inside this library's headers, and the SEI says psy_rd=1.0:0.2."""
    c = PC.CLI_CLIP
    src, out = str(tmp_path / "in.y4m"), str(tmp_path / "out.264")
    write_clip(src, c["w"], c["h"], c["n"], t0=c["t0"], y4m=True)
    assert E.main(PC.CLI_ARGS.split() + ["-o", out, src]) == 0
    p = PC.cli_params(hip_lib)
    with np.load(PC.fixture_path("stream")) as z:
        gold = {k: z[k] for k in z.files}
    want = mux_reference_stream(hip_lib, p, gold, c["n"])
    got = open(out, "rb").read()
    assert got == want, "%d vs %d bytes" % (len(got), len(want))
    assert b"psy_rd=1.0:0.2" in got and b"trellis=1" in got
