"""Helpers for frame-level parity tests: host images in the device layout
(oracle/hostpic.py) tied to a FrameCtx."""
import ctypes as C

from oracle import hostpic
from x264_vs2008_amd import synth
from x264_vs2008_amd.frame import FrameCtx


class HostPic(hostpic.HostPic):
    """Host twin of x264hip_picture; geometry cross-checked against the device context."""

    def __init__(self, ctx, pic=None):
        d = ctx.dims
        g = hostpic.Geometry(d.width, d.height)
        assert (g.mb_w, g.mb_h, g.stride_y, g.stride_c) == (d.mb_w, d.mb_h, d.stride_y, d.stride_c)
        if pic is not None:
            assert (g.stride_lowres, g.width_lowres, g.lines_lowres) == (pic.stride_lowres, pic.width_lowres, pic.lines_lowres)
        super().__init__(g)
        self.ctx, self.d = ctx, d


def make_clip_frame(ctx, pic, t, ora):
    """Upload synthetic frame t to `pic`; return the HostPic holding the same
    pixels after the reference's mod-16 edge replication."""
    d = ctx.dims
    y, u, v = synth.frame(d.width, d.height, t)
    ctx.upload(pic, y, u, v)
    hp = HostPic(ctx, pic)
    hp.load_yuv(ora, "x264o_", y, u, v)
    return hp


# the 16x16 search on whole frames (tests/golden/me16_*.npz): size, method, me_range, subme, chroma_me, qp
ME_CASES = [((352, 288), 1, 16, 7, 1, 26), ((352, 288), 0, 16, 5, 1, 30), ((200, 120), 1, 16, 2, 0, 22), ((200, 120), 1, 8, 1, 0, 36),
            ((352, 288), 1, 16, 3, 1, 40), ((200, 120), 0, 16, 0, 0, 26)]


# a context with synthetic frame t_cur as the current picture and t_ref as the reference, each on the device and on the host
def me_setup_pair(hip_lib, oracle_lib, w, h, t_cur, t_ref):
    ctx = FrameCtx(hip_lib, w, h)
    cur, ref = ctx.new_picture(), ctx.new_picture()
    hc = make_clip_frame(ctx, cur, t_cur, oracle_lib)
    hr = make_clip_frame(ctx, ref, t_ref, oracle_lib)
    # the reference picture gets borders + half-pel planes, as a reconstructed frame would
    assert hip_lib.x264hip_expand_border(ctx.h, C.byref(ref), 0) == 0, "x264hip_expand_border failed on the reference picture (frame %d)" % t_ref
    assert hip_lib.x264hip_hpel_filter_frame(ctx.h, C.byref(ref)) == 0, "x264hip_hpel_filter_frame failed on the reference picture (frame %d)" % t_ref
    _, stride, w16, h16, padh, padv = hr.full["y"]
    oracle_lib.x264o_plane_expand_border(hr.ptr("y"), stride, w16, h16, padh, padv)
    oracle_lib.x264o_frame_hpel(hr.ptr("y"), hr.ptr("h"), hr.ptr("vv"), hr.ptr("c"), stride, w16, h16, ctx.dims.mb_h)
    return ctx, cur, ref, hc, hr
