"""GPU: lossless (--qp 0) in the raster-order variant of the sweep -- I and P slices with the CABAC writer in the loop, below the RD levels
(subme 2, 5), with the RD mode decision (6, 7) and with the RD refinement (8, 9) -- against chains the REFERENCE's own loop produced with
h->mb.b_lossless on (oracle/ref_slice.c refslice_encode_chain2 at qp 0; fixtures tests/golden/ll_*.npz, made by tests/lossless_cases.py):
every decision, every level, mb_bits, the payload bytes and the planes; and, independently of the reference, every reconstructed plane
against the source.  Lock-step launches (x264hip_slice_sweep_frame), batches, and the chain table (x264hip_slice_sweep_chains).

Without the lossless raster kernels every test here fails with "lossless is not built in the raster variant"."""
import hashlib
import os

import numpy as np
import pytest

import lossless_cases as LC
from conftest import GOLDEN
from oracle.gen_golden_slice import case_inputs
from x264_vs2008_amd import slice as sl
from paths import REF_SO
from slice_util import run_chain2
from table_util import table_launch
from x264_vs2008_amd.frame import DeviceArray

pytestmark = pytest.mark.gpu
STATE = [k for k in LC.WHOLE if k not in ("mvr", "frame_info", "stat", "payload_len", "mb_bits")]


def load(name):
    with np.load(os.path.join(GOLDEN, "ll_%s.npz" % name)) as z:
        return {k: z[k] for k in z.files}


def check_frame(d, gold, f, src, b=0, what=""):
    """One frame of one chain against the fixture (or the live reference's arrays put through lossless_cases.to_fixture) and the source."""
    for k in STATE:
        got, want = d[k][b], gold[k][f]
        assert np.array_equal(got.reshape(want.shape), want), "%sframe %d: %s differs first at %s" % (what, f, k, np.argwhere(got.reshape(want.shape) != want)[:3].tolist())
    skip = gold["mb_type"][f] == sl.P_SKIP
    for r in range(int(gold["frame_info"][f][2])):
        assert np.array_equal(d["mvr"][b][r][~skip], gold["mvr"][f][r][~skip]), "%sframe %d: mvr[%d]" % (what, f, r)
    assert d["info"] == (int(gold["frame_info"][f][0]), 0), "%sframe %d: slice type / QP %s" % (what, f, d["info"])
    assert int(d["cost_intra"][b].sum()) == int(gold["stat"][f][0]) and int(d["cost_inter"][b].sum()) == int(gold["stat"][f][1]), "%sframe %d: statistics" % (what, f)
    want_bits = gold["mb_bits"][f]
    assert np.array_equal(d["mb_bits"][b], want_bits), "%sframe %d: mb_bits differ first at macroblock %s" % (what, f, np.argwhere(d["mb_bits"][b] != want_bits)[:1].tolist())
    pay = d["payload"][b]
    assert len(pay) == int(gold["payload_len"][f]), "%sframe %d: payload %d bytes, the reference %d" % (what, f, len(pay), int(gold["payload_len"][f]))
    assert hashlib.md5(pay).hexdigest() == str(gold["payload_md5"][f]), "%sframe %d: payload bytes differ" % (what, f)
    for i, nm in enumerate(("y", "u", "v")):
        for kind in ("rec_", "fin_"):
            assert LC.md5(d[kind + nm][b]) == str(gold[kind + nm + "_md5"][f]), "%sframe %d: %s%s differs from the reference" % (what, f, kind, nm)
            # lossless: whatever the reference says, the reconstruction IS the source (the loop filter leaves QP 0 alone)
            assert np.array_equal(d[kind + nm][b], src[i]), "%sframe %d: %s%s is not the source at %s" % (what, f, kind, nm, np.argwhere(d[kind + nm][b] != src[i])[:3].tolist())


@pytest.mark.parametrize("name,size,frames,kind,kw", LC.LL_CASES, ids=[c[0] for c in LC.LL_CASES])
def test_lossless_raster_matches_reference(hip_lib, cqm, name, size, frames, kind, kw):
    gold = load(name)
    y, u, v = case_inputs(size, frames, kind)
    out = run_chain2(hip_lib, cqm, size, frames, y, u, v, kw, {})
    for f in range(frames):
        check_frame(out[f], gold, f, (y[f], u[f], v[f]))
    t = gold["mb_type"]
    assert (t == sl.P_L0).any() and (t[0] <= sl.I_16x16).all()          # I and P slices


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libx264ref.so not built (the fixtures hold the same chains)")
@pytest.mark.parametrize("name", ["s5_sub8x8", "s7_umh", "s9_umh"])
def test_lossless_raster_matches_reference_live(hip_lib, cqm, name):
    """The same options on the other clip kind, against the reference run here."""
    _, size, frames, kind, kw = LC.LL_BY_NAME[name]
    kind = "static" if kind == "moving" else "moving"
    gold = LC.to_fixture(LC.reference_chain(size, frames, kind, kw))
    y, u, v = case_inputs(size, frames, kind)
    out = run_chain2(hip_lib, cqm, size, frames, y, u, v, kw, {})
    for f in range(frames):
        check_frame(out[f], gold, f, (y[f], u[f], v[f]))


def test_three_chains_with_different_content_in_one_launch(hip_lib, cqm):
    """Chain b codes the clip rotated by b frames: every element must equal the reference's chain for ITS input.  The rotations of a
    fixture's clip are not fixtures themselves, so the levels and bytes are held to the fixture where the rotation is the identity and
    to the live reference where it is built; every chain is held to its source."""
    name, size, frames, kind, kw = LC.LL_BY_NAME["s7_umh"]
    gold = load(name)
    y, u, v = case_inputs(size, frames, kind)
    enc = sl.ChainEncoder(hip_lib, size[0], size[1], cqm, batch=3, write=1, **kw)
    live = os.path.exists(REF_SO)
    want = [gold] + [LC.to_fixture(LC.reference_chain_of(size, kw, y[np.roll(np.arange(frames), -b)], u[np.roll(np.arange(frames), -b)], v[np.roll(np.arange(frames), -b)]))
                     if live else None for b in (1, 2)]
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
                t = (f + b) % frames
                if want[b] is not None:
                    check_frame(d, want[b], f, (y[t], u[t], v[t]), b=b, what="chain %d " % b)
                else:
                    for i, nm in enumerate(("y", "u", "v")):
                        assert np.array_equal(d["fin_" + nm][b], (y[t], u[t], v[t])[i]), "chain %d frame %d: %s is not the source" % (b, f, nm)
                    assert len(d["payload"][b]) > 0
    finally:
        enc.close()


@pytest.mark.parametrize("name", ["s6_med", "s8_med"])
def test_chain_table_all_lossless(hip_lib, cqm, name):
    """x264hip_slice_sweep_chains with every chain at QP 0 (the table kernels, below and with the RD refinement): the fixture's bytes in every chain."""
    _, size, frames, kind, kw = LC.LL_BY_NAME[name]
    gold = load(name)
    y, u, v = case_inputs(size, frames, kind)
    out = table_launch(hip_lib, cqm, size, frames, y, u, v, kw, [0, 0, 0])
    for f in range(frames):
        for b in range(3):
            assert np.array_equal(out[f]["mb_type"][b], gold["mb_type"][f]), "frame %d chain %d: mb_type" % (f, b)
            assert np.array_equal(out[f]["mb_bits"][b], gold["mb_bits"][f]), "frame %d chain %d: mb_bits" % (f, b)
            assert hashlib.md5(out[f]["payload"][b]).hexdigest() == str(gold["payload_md5"][f]), "frame %d chain %d: payload" % (f, b)
            for i, src in enumerate((y[f], u[f], v[f])):
                assert np.array_equal(out[f]["rec"][i][b], src), "frame %d chain %d: plane %d is not the source" % (f, b, i)


def test_chain_table_mixing_lossless_and_lossy_is_refused(hip_lib, cqm):
    _, size, frames, kind, kw = LC.LL_BY_NAME["s6_med"]
    y, u, v = case_inputs(size, 1, kind)
    with pytest.raises(RuntimeError, match="all-lossless or not at all"):
        table_launch(hip_lib, cqm, size, 1, y, u, v, kw, [0, 26])


@pytest.mark.parametrize("what,needle", [("trellis", "trellis"), ("psy_rd", "psy-rd"), ("nr", "noise reduction"), ("fast_pskip", "fast_pskip"),
                                         ("chroma_qp_offset", "chroma QP offset"), ("aq", "adaptive quantisation")])
def test_lossless_preconditions_are_refused(hip_lib, cqm, what, needle):
    """What x264_validate_parameters turns off at QP 0 is the caller's precondition (ChainEncoder applies it; here it is put back by hand)."""
    y, u, v = case_inputs((96, 80), 1, "moving")
    enc = sl.ChainEncoder(hip_lib, 96, 80, cqm, qp=0, subme=6, me_method=1, n_refs=1, inter=0x13, intra=0x3, transform8x8=1, cabac=1, write=1)
    try:
        assert enc.lossless and enc.raster
        if what == "trellis":
            enc.rd_opt["trellis"] = 1
        elif what == "psy_rd":
            enc.psy_rd_fix = 256
        elif what == "nr":
            enc.opt["noise_reduction"] = 100
        elif what == "fast_pskip":
            enc.opt["fast_pskip"] = 1
        elif what == "chroma_qp_offset":
            enc.opt["chroma_qp_offset"] = 2
        else:
            n = enc.ctx.dims.mb_w * enc.ctx.dims.mb_h
            enc.rd_bufs["aq_energy"] = DeviceArray(hip_lib, (1, n), np.int32)
            enc.rd_bufs["aq_offset"] = DeviceArray(hip_lib, (1, n), np.float32)
            enc.rd_opt["aq_mode"] = 1
        enc.upload(y[0], u[0], v[0])
        with pytest.raises(RuntimeError) as e:
            enc.encode_frame()
        assert "lossless" in str(e.value) and needle in str(e.value), str(e.value)
    finally:
        enc.close()


def test_lossless_b_slices_and_sub8x8_rd_stay_refused(hip_lib, cqm):
    y, u, v = case_inputs((96, 80), 2, "moving")
    enc = sl.ChainEncoder(hip_lib, 96, 80, cqm, qp=0, subme=7, me_method=1, n_refs=1, inter=0x33, intra=0x3, transform8x8=1, cabac=1, write=1)
    try:
        enc.upload(y[0], u[0], v[0])
        with pytest.raises(RuntimeError, match="sub-8x8"):
            enc.encode_frame()
    finally:
        enc.close()
    enc = sl.ChainEncoder(hip_lib, 96, 80, cqm, qp=0, subme=5, me_method=1, n_refs=1, inter=0x113, intra=0x3, transform8x8=1, cabac=1, write=1, bframes=1)
    try:
        for disp, stype in ((0, sl.SLICE_I), (2, sl.SLICE_P)):
            enc.upload(y[0], u[0], v[0])
            enc.encode_frame(stype=stype, disp=disp)
            enc.finish_frame()
        enc.upload(y[1], u[1], v[1])
        with pytest.raises(RuntimeError, match="B slices"):
            enc.encode_frame(stype=sl.SLICE_B, disp=1)
    finally:
        enc.close()


def test_default_payload_buffer_follows_the_lossless_bound(hip_lib, cqm):
    """Below the RD levels nothing caps a lossless macroblock: the default buffer provides LL_MB_BYTES for each; a frame of noise (about
    800 bytes per macroblock, the lossy default's whole provision) is coded, and its planes come back."""
    w, h = 96, 80
    rng = np.random.default_rng(7)
    y, u, v = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    enc = sl.ChainEncoder(hip_lib, w, h, cqm, qp=0, subme=5, me_method=1, n_refs=1, inter=0x13, intra=0x3, transform8x8=1, cabac=1, write=1)
    try:
        n = enc.ctx.dims.mb_w * enc.ctx.dims.mb_h
        assert enc.payload_cap >= n * sl.LL_MB_BYTES + sl.MB_BYTES_MAX + 128
        enc.upload(y, u, v)
        enc.encode_frame()
        enc.status()
        pay = enc.payloads()[0]
        assert len(pay) > n * 384                      # more than raw samples would take: nothing capped it
        for nm, src in (("y", y), ("u", u), ("v", v)):
            assert np.array_equal(enc.ctx.download(enc.last[0], nm, padded=False), src)
    finally:
        enc.close()
