"""GPU: whole-plane kernels (upload + mod-16 pad, border expansion, half-pel
planes, half-resolution planes, AQ energy, SSD) against the CPU twin built
from the oracle's table entries.  Byte-exact over the FULL padded planes,
padding included, because motion vectors may point into it."""
import ctypes as C

import numpy as np
import pytest

from frame_util import HostPic, make_clip_frame
from x264_vs2008_amd.frame import FrameCtx

pytestmark = pytest.mark.gpu

SIZES = [(352, 288), (200, 120), (1920, 1080)]


@pytest.fixture(params=SIZES, ids=lambda s: "%dx%d" % s)
def ctx(request, hip_lib):
    c = FrameCtx(hip_lib, *request.param)
    yield c
    c.close()


def _eq(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d bytes differ, first at (row, col) %s" % (what, len(bad), bad[0]))


def test_upload_and_border(ctx, hip_lib, oracle_lib):
    pic = ctx.new_picture()
    hp = make_clip_frame(ctx, pic, 3, oracle_lib)
    assert hip_lib.x264hip_expand_border(ctx.h, C.byref(pic), 0) == 0
    for name in ("y", "u", "v"):
        _, stride, w, h, padh, padv = hp.full[name]
        oracle_lib.x264o_plane_expand_border(hp.ptr(name), stride, w, h, padh, padv)
        _eq(ctx.download(pic, name), hp.arr(name), "border " + name)


def test_hpel_planes(ctx, hip_lib, oracle_lib):
    pic = ctx.new_picture()
    hp = make_clip_frame(ctx, pic, 5, oracle_lib)
    assert hip_lib.x264hip_expand_border(ctx.h, C.byref(pic), 0) == 0
    assert hip_lib.x264hip_hpel_filter_frame(ctx.h, C.byref(pic)) == 0
    _, stride, w, h, padh, padv = hp.full["y"]
    oracle_lib.x264o_plane_expand_border(hp.ptr("y"), stride, w, h, padh, padv)
    oracle_lib.x264o_frame_hpel(hp.ptr("y"), hp.ptr("h"), hp.ptr("vv"), hp.ptr("c"), stride, w, h, ctx.dims.mb_h)
    for name in ("h", "vv", "c"):
        _eq(ctx.download(pic, name), hp.arr(name), "hpel plane " + name)


def test_lowres_planes(ctx, hip_lib, oracle_lib):
    pic = ctx.new_picture()
    hp = make_clip_frame(ctx, pic, 7, oracle_lib)
    assert hip_lib.x264hip_lowres_init_frame(ctx.h, C.byref(pic)) == 0
    _, stride, w, h, _, _ = hp.full["y"]
    oracle_lib.x264o_frame_lowres(hp.ptr("y"), stride, w, h, hp.ptr("l0"), hp.ptr("lh"), hp.ptr("lv"), hp.ptr("lc"),
                                  pic.stride_lowres, pic.width_lowres, pic.lines_lowres)
    for name in ("l0", "lh", "lv", "lc"):
        got, want = ctx.download(pic, name), hp.arr(name)
        # for odd mb_w the reference pads from columns [width_lowres, stride - 64) that it never
        # writes (frame.c:298-301); both sides start from zeroed planes here, so they still agree
        _eq(got, want, "lowres " + name)
    # the source plane gets its last column / row duplicated (mc.c:314-317)
    _eq(ctx.download(pic, "y"), hp.arr("y"), "source after lowres")
    # lookahead intra cost on the lowres plane (slicetype.c:186-245)
    from x264_vs2008_amd.frame import DeviceArray
    d = ctx.dims
    n = d.mb_w * d.mb_h
    out = DeviceArray(hip_lib, n, np.int32)
    assert hip_lib.x264hip_lookahead_intra_frame(ctx.h, C.byref(pic), out.p) == 0
    ctx.sync()
    want = np.zeros(n, np.int32)
    oracle_lib.x264o_frame_lookahead_intra(hp.ptr("l0"), pic.stride_lowres, d.mb_w, d.mb_h, want.ctypes.data_as(C.c_void_p))
    got = out.get()
    assert np.array_equal(got, want), "lookahead intra cost differs at %s" % np.argwhere(got != want)[:5]
    assert got.min() >= 5 and len(np.unique(got)) > 10
    out.free()


def test_aq_var_and_ssd(ctx, hip_lib, oracle_lib):
    from x264_vs2008_amd.frame import DeviceArray
    a, b = ctx.new_picture(), ctx.new_picture()
    ha = make_clip_frame(ctx, a, 1, oracle_lib)
    hb = make_clip_frame(ctx, b, 2, oracle_lib)
    d = ctx.dims
    n = d.mb_w * d.mb_h
    out = DeviceArray(hip_lib, n, np.int32)
    assert hip_lib.x264hip_aq_var_frame(ctx.h, C.byref(a), out.p) == 0
    ctx.sync()
    want = np.zeros(n, np.int32)
    oracle_lib.x264o_frame_aq_var(ha.ptr("y"), ha.ptr("u"), ha.ptr("v"), d.stride_y, d.stride_c, d.mb_w, d.mb_h,
                                  want.ctypes.data_as(C.c_void_p))
    assert np.array_equal(out.get(), want)
    out.free()
    ssd = (C.c_int64 * 3)()
    assert hip_lib.x264hip_ssd_frame(ctx.h, C.byref(a), C.byref(b), ssd) == 0
    oracle_lib.x264o_frame_ssd.restype = C.c_int64
    for i, name in enumerate(("y", "u", "v")):
        st = d.stride_c if i else d.stride_y
        want = oracle_lib.x264o_frame_ssd(ha.ptr(name), st, hb.ptr(name), st, d.width >> (i > 0), d.height >> (i > 0))
        assert ssd[i] == want, name


@pytest.mark.parametrize("size,batch", [((200, 120), 3), ((352, 288), 2), ((1920, 1080), 1)])
def test_synthetic_source_on_the_device_equals_the_host_generator(hip_lib, size, batch):
    """x264hip_picture_synth (the bench's input: SURVEY 8(d)'s integer generator as a kernel) against x264_vs2008_amd/synth.py,
    every visible pixel and the mod-16 padding, for several batch elements with their own frame numbers."""
    _synth_equals_host(hip_lib, size, batch, 37, 12)


INT_MAX = (1 << 31) - 1


# bench.py's frame numbers: chain g's pictures start g * 4096 frames into the clip, so with 8 GPUs of 2048 chains the last chain's reach
# (7 * 2048 + 2047) * 4096 ~ 6.7e7 (weak scaling, stride 4096; strong scaling: rank + 8 * b, stride 8 * 4096) -- where (x + y + 5t) * 9 no
# longer fits an int; and the largest frame number the library accepts
@pytest.mark.parametrize("size,t0,ts", [((1920, 1080), (7 * 2048 + 2045) * 4096 + 15, 4096), ((200, 120), (7 + 8 * 2045) * 4096 + 4095, 8 * 4096),
                                         ((352, 288), INT_MAX - 2 * 1000003, 1000003), ((200, 120), INT_MAX - 2, 1)])
def test_synthetic_source_at_the_benchmarks_frame_numbers(hip_lib, size, t0, ts):
    _synth_equals_host(hip_lib, size, 3, t0, ts)


def test_synthetic_source_refuses_frame_numbers_above_int_max(hip_lib):
    """t0 + (batch - 1) * t_stride > INT_MAX: an error, and nothing is written; the last legal frame number is synthesised right."""
    from x264_vs2008_amd import synth
    c = FrameCtx(hip_lib, 200, 120, batch=3)
    try:
        pic = c.new_picture(source_only=True)
        c.synth(pic, 5, 7)
        c.sync()
        before = [c.download(pic, name, padded=True, b=b) for b in range(3) for name in ("y", "u", "v")]
        for t0, ts in ((INT_MAX - 2 * 4096 + 1, 4096), (1, INT_MAX), (INT_MAX, 1), (2, (1 << 30))):
            with pytest.raises(RuntimeError, match="exceeds INT_MAX"):
                c.synth(pic, t0, ts)
        c.sync()
        after = [c.download(pic, name, padded=True, b=b) for b in range(3) for name in ("y", "u", "v")]
        assert all(np.array_equal(a, b) for a, b in zip(before, after)), "a refused x264hip_picture_synth wrote the picture"
        c.synth(pic, INT_MAX - 2 * 4096, 4096)                   # element 2: frame INT_MAX
        c.sync()
        for name, pl in zip(("y", "u", "v"), synth.frame(200, 120, INT_MAX)):
            got = c.download(pic, name, padded=False, b=2)
            _eq(got[:pl.shape[0], :pl.shape[1]], pl, "synth %s element 2 (frame INT_MAX)" % name)
    finally:
        c.close()


def _synth_equals_host(hip_lib, size, batch, t0, ts):
    from x264_vs2008_amd import synth
    c = FrameCtx(hip_lib, *size, batch=batch)
    try:
        pic = c.new_picture(source_only=True)
        c.synth(pic, t0, ts)
        c.sync()
        w, h = size
        for b in range(batch):
            want = synth.frame(w, h, t0 + b * ts)
            for name, pl in zip(("y", "u", "v"), want):
                got = c.download(pic, name, padded=False, b=b)
                hh, ww = pl.shape
                _eq(got[:hh, :ww], pl, "synth %s element %d (frame %d)" % (name, b, t0 + b * ts))
                # x264_frame_expand_border_mod16: the last column / row repeated up to the coded size
                assert (got[:hh, ww:] == pl[:, -1:]).all() and (got[hh:, :ww] == pl[-1:, :]).all() and (got[hh:, ww:] == pl[-1, -1]).all()
    finally:
        c.close()
