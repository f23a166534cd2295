"""GPU: the quality pass (x264hip_frame_report_chains: csrc/frame_quality.hip) against the reference's x264_pixel_ssd_wxh / x264_pixel_ssim_wxh called with
x264_fdec_filter_row's chunking (tests/quality_cases.py) -- first on synthetic planes without an encoder, then behind ChainEncoder's frames against
tests/golden/quality_chains.npz.  ssd is compared as integers, ssim on its 8 bytes: a whole-frame call of the same function differs from the chunked sum in
the low bits for nearly every frame, so anything but the reference's nesting of the float adds shows."""
import ctypes as C

import numpy as np
import pytest

import quality_cases as qc
from x264_vs2008_amd import slice as sl
from x264_vs2008_amd.frame import FrameCtx
from x264_vs2008_amd.quality import Reporter

pytestmark = pytest.mark.gpu

# 16x16: one macroblock, one call, a 2-wide last group; 24x40: ragged; then ((W - 2) >> 2) - 1 mod 4 = 1, 2, 3, 0 (last groups of 1, 2, 3, 4 values), the block
# column count even and odd, heights 16 k + 8 (as 1080), 16 k, and a single-digit row count
SIZES = [(16, 16), (24, 40), (204, 120), (208, 144), (212, 72), (200, 120)]


@pytest.fixture(scope="module")
def measure():
    return qc.Measure()


def planes(rng, w, h, base=None, noise=0):
    if base is None:
        return [rng.integers(0, 256, (h >> s, w >> s), dtype=np.uint8) for s in (0, 1, 1)]
    return [np.clip(p.astype(np.int32) + rng.integers(-noise, noise + 1, p.shape), 0, 255).astype(np.uint8) for p in base]


def smooth(rng, w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    y = (128 + 60 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + rng.integers(-4, 5, (h, w))).clip(0, 255).astype(np.uint8)
    return [y, y[::2, ::2].copy(), y[1::2, 1::2].copy()]


@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_kernel_equals_reference_functions_on_planes(hip_lib, measure, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    assert ((w - 2) >> 2) - 1 > 0
    ctx = FrameCtx(hip_lib, w, h, batch=3)
    rep = Reporter(ctx, 8)
    try:
        pics = {k: ctx.new_picture(source_only=True) for k in ("srcA", "srcB", "recA", "recB")}
        host = {}
        host["srcA", 0], host["srcA", 1], host["srcA", 2] = planes(rng, w, h), smooth(rng, w, h), planes(rng, w, h)
        host["srcB", 0], host["srcB", 1], host["srcB", 2] = smooth(rng, w, h), planes(rng, w, h), planes(rng, w, h)
        host["recA", 0] = planes(rng, w, h)                                      # noise against noise
        host["recA", 1] = [p.copy() for p in host["srcA", 1]]                     # a picture against itself
        one = [p.copy() for p in host["srcA", 2]]                                # ... plus one changed pixel in the last measured row and in the last column
        one[0][h - 1, 5] ^= 0x40; one[0][7, w - 1] ^= 0x20; one[1][(h >> 1) - 1, (w >> 1) - 1] ^= 0x10; one[2][0, (w >> 1) - 1] ^= 0x08
        host["recA", 2] = one
        host["recB", 0] = planes(rng, w, h, host["srcB", 0], 3)                   # a plausible reconstruction
        host["recB", 1] = planes(rng, w, h)
        last = [p.copy() for p in host["srcA", 0]]
        last[0][h - 1, w - 1] ^= 0x80
        host["recB", 2] = last
        for (k, b), p in host.items():
            ctx.upload(pics[k], p[0], p[1], p[2], b=b)
        # entries name different pictures and elements, not in element order; (psnr, ssim) both on except in the last two
        table = [("srcA", 2, "recA", 2, 1, 1), ("srcB", 0, "recB", 0, 1, 1), ("srcA", 1, "recA", 1, 1, 1), ("srcA", 0, "recA", 0, 1, 1), ("srcA", 0, "recB", 2, 1, 1),
                 ("srcB", 0, "recB", 0, 0, 1), ("srcB", 0, "recB", 0, 1, 0)]
        s = rep.chains([(i % 3, pics[a], ea, pics[b], eb, None, i % 3, ps, ss, 1) for i, (a, ea, b, eb, ps, ss) in enumerate(table)])
        ctx.sync()
        got, parts = Reporter.records(s), rep.partials(s)
        for i, (a, ea, b, eb, ps, ss) in enumerate(table):
            ssd, want_parts, f_ssim = measure.frame(host[b, eb], host[a, ea], psnr=ps, ssim=ss)
            what = "%dx%d entry %d (%s[%d] against %s[%d])" % (w, h, i, b, eb, a, ea)
            print(what, "ssd", got[i]["ssd"].tolist(), ssd.tolist(), "f_ssim", float(got[i]["ssim"]), f_ssim)
            assert got[i]["ssd"].tolist() == ssd.tolist(), what
            if ss:
                assert parts[i]["ssim"].tobytes() == want_parts.tobytes(), "%s: the calls' floats %s, the reference's %s" % (what, parts[i]["ssim"].tolist(), want_parts.tolist())
            assert np.float64(got[i]["ssim"]).tobytes() == np.float64(f_ssim).tobytes(), what
            assert not got[i]["mb_count"].any() and not got[i]["mb_count_ref"].any() and got[i]["qp_sum"] == 0          # no state: no counters
        assert got[2]["ssd"].tolist() == [0, 0, 0] and got[5]["ssd"].tolist() == [0, 0, 0] and got[6]["ssim"] == 0.0
        assert got[0]["ssd"].tolist() == [0x40 ** 2 + 0x20 ** 2, 0x10 ** 2, 0x08 ** 2] and got[4]["ssd"].tolist() == [0x80 ** 2, 0, 0]
    finally:
        rep.close()
        ctx.close()


def make_encoder(hip_lib, cqm, name, batch=1, **over):
    size, frames, kind, kw, ekw, clip = qc.case_config(name)
    kw.pop("cqm_preset", 0)
    kw.update(over)
    enc = sl.ChainEncoder(hip_lib, size[0], size[1], cqm, batch=batch, write=1, psnr=1, ssim=1, **kw, **{k: v for k, v in ekw.items() if k not in ("write", "lowres_seed")})
    order = sl.coding_order(frames, kw.get("keyint", 0), ekw["bframes"]) if ekw.get("bframes") else [(f, None) for f in range(frames)]
    return enc, order, clip, size


@pytest.mark.parametrize("name", qc.CASES)
def test_lock_step_chain_reports_equal_the_fixture(hip_lib, cqm, name):
    """Every frame's whole record -- measurements and counters -- against what the reference measured on its own pictures (fin_* for I / P, rec_* for the
    unfiltered B frames) and what its counting rules give on its own state arrays.  Two chains of the same content: both elements."""
    want = qc.load_fixture(name)
    enc, order, (y, u, v), size = make_encoder(hip_lib, cqm, name, batch=2)
    try:
        for f, (disp, stype) in enumerate(order):
            for b in range(2):
                enc.upload(y[disp], u[disp], v[disp], b=b)
            enc.encode_frame(stype=stype, disp=disp) if stype is not None else enc.encode_frame()
            enc.status()
            enc.finish_frame()
            enc.sync()
            got = enc.reports()
            assert len(got) == 2
            for b in range(2):
                qc.same_record(got[b], qc.record_of(want[f]), "%s frame %d chain %d" % (name, f, b))
    finally:
        enc.close()


def test_lanes_measure_b_frames_on_their_own_streams(hip_lib, cqm):
    """lanes = 3: the B frames' passes run on the lanes' streams behind their sweeps, nothing synchronises until the clip is enqueued."""
    want = qc.load_fixture("b_medium")
    enc, order, (y, u, v), size = make_encoder(hip_lib, cqm, "b_medium", lanes=3)
    try:
        srcs = []
        for d in range(len(order)):
            pic = enc.ctx.new_picture(source_only=True)
            enc.ctx.upload(pic, y[d], u[d], v[d], b=0)
            srcs.append(pic)
        handles = []
        for f, (disp, stype) in enumerate(order):
            enc.encode_frame(srcs[disp], stype=stype, disp=disp)
            enc.finish_frame()
            handles.append(enc.last_report)
        enc.sync()
        enc.status()
        assert len({id(h) for h in handles}) == len(handles)
        for f, h in enumerate(handles):
            qc.same_record(Reporter.records(h)[0], qc.record_of(want[f]), "b_medium frame %d (lanes)" % f)
    finally:
        enc.close()


def test_without_the_loop_filter_every_frame_is_measured_as_coded(hip_lib, cqm, measure):
    """deblock = 0: kept frames are measured on their unfiltered reconstruction too.  Such a chain's P frames predict from unfiltered pictures, so only its
    I frame has a fixture (rec_* of frame 0 does not depend on the filter); every frame is compared with the reference's functions and counting rules applied
    to the planes and the state this very chain left on the device."""
    want = qc.load_fixture("b_medium")
    enc, order, (y, u, v), (w, h) = make_encoder(hip_lib, cqm, "b_medium", deblock=0)
    n_refs = enc.opt["n_refs"]
    try:
        for f, (disp, stype) in enumerate(order):
            enc.upload(y[disp], u[disp], v[disp])
            enc.encode_frame(stype=stype, disp=disp)
            enc.status()
            enc.finish_frame()
            enc.sync()
            got = enc.reports()[0]
            recon, state = enc.last
            rec = [enc.ctx.download(recon, p, padded=False, b=0)[:h >> (p != "y"), :w >> (p != "y")] for p in "yuv"]
            ssd, parts, f_ssim = measure.frame(rec, (y[disp], u[disp], v[disp]))
            st = {k: state.get(k)[0] for k in ("mb_type", "partition", "sub_partition", "ref", "cbp", "t8", "qp")}
            ref1 = np.zeros_like(st["ref"])
            assert hip_lib.x264hip_memcpy_d2h(ref1.ctypes.data_as(C.c_void_p), state.st.ref1, ref1.nbytes) == 0
            e = dict(qc.count_state(stype, n_refs, st["mb_type"], st["partition"], st["sub_partition"], st["ref"], ref1, st["cbp"], st["t8"], st["qp"]), ssd=ssd, f_ssim=f_ssim)
            qc.same_record(got, qc.record_of(e), "deblock 0, frame %d" % f)
            if f == 0:
                assert got["ssd"].tolist() == want[0]["rec0_ssd"].tolist() and float(got["ssim"]) == want[0]["rec0_f_ssim"]
    finally:
        enc.close()
