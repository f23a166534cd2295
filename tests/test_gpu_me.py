"""GPU: one-wavefront-per-macroblock motion search against the CPU twin
(oracle/frame_oracle.c: pixf.sad / pixf.satd / mc.get_ref of the pinned
oracle, looped the slow way).  Vectors, costs and the SAD surface must be
identical; ties included (first vector in (my, mx) raster order)."""
import ctypes as C

import numpy as np
import pytest

from frame_util import me_setup_pair as _setup
from x264_vs2008_amd.frame import DeviceArray, MeParams, cost_mv_table

pytestmark = pytest.mark.gpu

LAMBDA_QP26 = 4          # x264_lambda_tab[26], R/encoder/analyse.c:140-150


def _run_fullpel(hip_lib, oracle_lib, ctx, cur, ref, hc, hr, rng, centers=None, mvp=None, lam=LAMBDA_QP26):
    d = ctx.dims
    n = d.mb_w * d.mb_h
    span = 4 * 2048
    tab = cost_mv_table(lam, span)
    cost_dev = DeviceArray(hip_lib, tab.shape, np.uint16, tab)
    nn = (2 * rng + 1) ** 2
    mv_dev = DeviceArray(hip_lib, (n, 9, 2), np.int16)
    c_dev = DeviceArray(hip_lib, (n, 9), np.int32)
    s_dev = DeviceArray(hip_lib, (n, nn), np.uint16)
    cen_dev = DeviceArray(hip_lib, (n, 2), np.int16, centers) if centers is not None else None
    mvp_dev = DeviceArray(hip_lib, (n, 2), np.int16, mvp) if mvp is not None else None
    p = MeParams(range=rng, cost_mv=cost_dev.ptr, cost_mv_range=span,
                 centers=cen_dev.ptr if cen_dev else None, mvp=mvp_dev.ptr if mvp_dev else None,
                 sad_surface=s_dev.ptr, mv_range=512)
    assert hip_lib.x264hip_me_fullpel_frame(ctx.h, C.byref(cur), C.byref(ref), C.byref(p), mv_dev.p, c_dev.p) == 0, \
        hip_lib.x264hip_last_error()
    ctx.sync()
    want_mv = np.zeros((n, 9, 2), np.int16); want_c = np.zeros((n, 9), np.int32)
    want_s = np.zeros((n, nn), np.uint16); valid = np.zeros((n, nn), np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    cen = np.ascontiguousarray(centers, np.int16) if centers is not None else None
    mvpa = np.ascontiguousarray(mvp, np.int16) if mvp is not None else None
    oracle_lib.x264o_frame_me_fullpel(hc.ptr("y"), hr.ptr("y"), d.mb_w, d.mb_h, d.stride_y, rng, 512, vp(tab), span,
                                      vp(cen), vp(mvpa), vp(want_mv), vp(want_c), vp(want_s), vp(valid))
    got_mv, got_c, got_s = mv_dev.get(), c_dev.get(), s_dev.get()
    assert np.array_equal(got_c, want_c), "costs differ at %s" % np.argwhere(got_c != want_c)[:5]
    assert np.array_equal(got_mv, want_mv), "vectors differ at %s" % np.argwhere(got_mv != want_mv)[:5]
    m = valid.astype(bool)
    assert m.any() and np.array_equal(got_s[m], want_s[m]), "SAD surface differs"
    return ctx, p, tab, span, got_mv, (cost_dev, mv_dev, c_dev, s_dev, cen_dev, mvp_dev)


@pytest.mark.parametrize("size,rng", [((352, 288), 16), ((352, 288), 8), ((200, 120), 24), ((640, 368), 16)])
def test_fullpel_exhaustive(hip_lib, oracle_lib, size, rng):
    ctx, cur, ref, hc, hr = _setup(hip_lib, oracle_lib, size[0], size[1], 4, 3)
    try:
        _run_fullpel(hip_lib, oracle_lib, ctx, cur, ref, hc, hr, rng)
    finally:
        ctx.close()


def test_fullpel_centres_and_predictors(hip_lib, oracle_lib):
    """Per-macroblock search centres (unaligned, some pushing the window to the mv limits)
    and qpel predictors, plus a large lambda so mv cost dominates and ties appear."""
    ctx, cur, ref, hc, hr = _setup(hip_lib, oracle_lib, 352, 288, 9, 6)
    try:
        n = ctx.dims.mb_w * ctx.dims.mb_h
        r = np.random.RandomState(5)
        centers = r.randint(-30, 31, (n, 2)).astype(np.int16)
        mvp = r.randint(-120, 121, (n, 2)).astype(np.int16)
        _run_fullpel(hip_lib, oracle_lib, ctx, cur, ref, hc, hr, 16, centers, mvp, lam=91)
    finally:
        ctx.close()


def test_fullpel_identical_frames_zero_vector(hip_lib, oracle_lib):
    """Property: searching a frame in itself finds the zero vector with SAD 0 for all partitions."""
    ctx, cur, ref, hc, hr = _setup(hip_lib, oracle_lib, 352, 288, 2, 2)
    try:
        _, _, _, _, mv, _ = _run_fullpel(hip_lib, oracle_lib, ctx, cur, ref, hc, hr, 16)
        assert not mv.any()
    finally:
        ctx.close()


@pytest.mark.parametrize("size", [(352, 288), (200, 120)])
def test_subpel_refine(hip_lib, oracle_lib, size):
    ctx, cur, ref, hc, hr = _setup(hip_lib, oracle_lib, size[0], size[1], 7, 5)
    try:
        ctx, p, tab, span, mv_full, bufs = _run_fullpel(hip_lib, oracle_lib, ctx, cur, ref, hc, hr, 16)
        d = ctx.dims
        n = d.mb_w * d.mb_h
        out_mv = DeviceArray(hip_lib, (n, 2), np.int16); out_c = DeviceArray(hip_lib, n, np.int32)
        assert hip_lib.x264hip_me_subpel_frame(ctx.h, C.byref(cur), C.byref(ref), C.byref(p), bufs[1].p, out_mv.p, out_c.p) == 0
        ctx.sync()
        want_mv = np.zeros((n, 2), np.int16); want_c = np.zeros(n, np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        oracle_lib.x264o_frame_me_subpel(hc.ptr("y"), hr.ptr("y"), hr.ptr("h"), hr.ptr("vv"), hr.ptr("c"), d.mb_w, d.mb_h,
                                         d.stride_y, 512, vp(tab), span, None, vp(np.ascontiguousarray(mv_full)),
                                         vp(want_mv), vp(want_c))
        assert np.array_equal(out_c.get(), want_c), "subpel costs differ"
        assert np.array_equal(out_mv.get(), want_mv), "subpel vectors differ"
        assert (out_mv.get() % 4 != 0).any(), "test clip produced no fractional vectors"
    finally:
        ctx.close()
