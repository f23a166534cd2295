"""GPU: the whole-plane passes on pictures of one to six macroblocks (tests/edge_cases.py: SIZES) -- x264hip_expand_border,
x264hip_hpel_filter_frame, x264hip_lowres_init_frame and x264hip_deblock_frame -- against the CPU twins (oracle/frame_oracle.c, pinned to
the reference's drivers at these sizes by tests/test_oracle_frame_golden.py).  At these sizes the 32-pixel padding is wider than the
picture, a half-resolution plane is 8 pixels wide, and the 2:1 anti-diagonal of the loop filter has one or two macroblocks.  Inputs: the
full-range ramp and the 0 / 255 noise, for the loop filter also a flat picture under blocky offsets with side information drawn as in
tests/test_gpu_deblock.py.  Byte-equal over the FULL padded planes (the loop filter: the coded planes, which are all it writes)."""
import ctypes as C

import numpy as np
import pytest

import edge_cases as E
from frame_util import HostPic
from x264_vs2008_amd.frame import DeblockParams, DeviceArray, FrameCtx

pytestmark = pytest.mark.gpu

KINDS = ("ramp", "satnoise")


@pytest.fixture(params=E.SIZES, ids=E.size_id)
def ctx(request, hip_lib):
    c = FrameCtx(hip_lib, *request.param)
    yield c
    c.close()


def _eq(got, want, what):
    assert got.shape == want.shape, "%s: shape %s, the twin %s" % (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d bytes differ, first at (row, col) %s" % (what, len(bad), bad[0]))


def load(ctx, pic, yuv, ora):
    """Upload one picture; the HostPic holding the same pixels after the reference's mod-16 edge replication."""
    ctx.upload(pic, *yuv)
    hp = HostPic(ctx, pic)
    hp.load_yuv(ora, "x264o_", *yuv)
    return hp


def pictures(ctx, t):
    d = ctx.dims
    return [(k, tuple(a[t] for a in E.content(k, d.width, d.height, t + 1))) for k in KINDS]


def test_border_on_tiny_pictures(ctx, hip_lib, oracle_lib):
    for kind, yuv in pictures(ctx, 1):
        pic = ctx.new_picture()
        hp = load(ctx, pic, yuv, oracle_lib)
        for name in ("y", "u", "v"):                   # the upload's mod-16 replication
            _eq(ctx.download(pic, name, padded=False), hp.visible(name), "%s: upload %s" % (kind, name))
        assert hip_lib.x264hip_expand_border(ctx.h, C.byref(pic), 0) == 0, hip_lib.x264hip_last_error()
        for name in ("y", "u", "v"):
            _, stride, w, h, padh, padv = hp.full[name]
            oracle_lib.x264o_plane_expand_border(hp.ptr(name), stride, w, h, padh, padv)
            _eq(ctx.download(pic, name), hp.arr(name), "%s: border %s" % (kind, name))


def test_hpel_planes_on_tiny_pictures(ctx, hip_lib, oracle_lib):
    for kind, yuv in pictures(ctx, 2):
        pic = ctx.new_picture()
        hp = load(ctx, pic, yuv, oracle_lib)
        assert hip_lib.x264hip_expand_border(ctx.h, C.byref(pic), 0) == 0, hip_lib.x264hip_last_error()
        assert hip_lib.x264hip_hpel_filter_frame(ctx.h, C.byref(pic)) == 0, hip_lib.x264hip_last_error()
        _, stride, w, h, padh, padv = hp.full["y"]
        oracle_lib.x264o_plane_expand_border(hp.ptr("y"), stride, w, h, padh, padv)
        oracle_lib.x264o_frame_hpel(hp.ptr("y"), hp.ptr("h"), hp.ptr("vv"), hp.ptr("c"), stride, w, h, ctx.dims.mb_h)
        for name in ("h", "vv", "c"):
            _eq(ctx.download(pic, name), hp.arr(name), "%s: half-pel plane %s" % (kind, name))
        if kind == "ramp":
            assert len(np.unique(hp.visible("c"))) > 8         # the filters saw a picture, not a constant


def test_lowres_planes_on_tiny_pictures(ctx, hip_lib, oracle_lib):
    for kind, yuv in pictures(ctx, 0):
        pic = ctx.new_picture()
        hp = load(ctx, pic, yuv, oracle_lib)
        assert hip_lib.x264hip_lowres_init_frame(ctx.h, C.byref(pic)) == 0, hip_lib.x264hip_last_error()
        _, stride, w, h, _, _ = hp.full["y"]
        oracle_lib.x264o_frame_lowres(hp.ptr("y"), stride, w, h, hp.ptr("l0"), hp.ptr("lh"), hp.ptr("lv"), hp.ptr("lc"),
                                      pic.stride_lowres, pic.width_lowres, pic.lines_lowres)
        for name in ("l0", "lh", "lv", "lc"):
            # odd mb_w: the reference pads from columns [width_lowres, stride - 64) that it never writes (frame.c:298-301); both sides
            # start from zeroed planes, so they still agree
            _eq(ctx.download(pic, name), hp.arr(name), "%s: lowres %s" % (kind, name))
        _eq(ctx.download(pic, "y"), hp.arr("y"), "%s: source after lowres" % kind)      # its last column / row duplicated (mc.c:314-317)


def blocky(img, r, step, amp):
    """Per-block DC offsets, so that block edges exist for the filter to find."""
    h, w = img.shape
    off = r.randint(-amp, amp + 1, ((h + step - 1) // step, (w + step - 1) // step))
    big = np.kron(off, np.ones((step, step), np.int64))[:h, :w]
    return np.clip(img.astype(np.int64) + big, 0, 255).astype(np.uint8)


def side_info(r, n, qlo, qhi):
    """Per-macroblock side information as tests/test_gpu_deblock.py draws it: intra / inter / 8x8-transform mixes, one or four vectors."""
    mb_type = r.choice([0, 0, 0, 1, 2], n).astype(np.uint8)
    qp = r.randint(qlo, qhi + 1, n).astype(np.uint8)
    t8 = (r.rand(n) < 0.4).astype(np.uint8)
    nnz = (r.rand(n, 26) < 0.3).astype(np.uint8)
    nnz[mb_type == 2] = 0
    nnz[r.rand(n) < 0.3] = 0
    for mb in np.nonzero(t8)[0]:
        for b in range(4):
            nnz[mb, 4 * b:4 * b + 4] = nnz[mb, 4 * b]
    mv = np.repeat(r.randint(-6, 7, (n, 1, 2)).astype(np.int16), 16, axis=1)
    sub = r.rand(n) < 0.3
    for mb in np.nonzero(sub)[0]:
        m8 = r.randint(-6, 7, (2, 2, 2))
        for by in range(4):
            for bx in range(4):
                mv[mb, bx + 4 * by] = m8[by >> 1, bx >> 1]
    ref = r.randint(0, 2, (n, 4)).astype(np.int8)
    ref[~sub] = ref[~sub][:, :1]
    mv[mb_type == 1] = 0
    ref[mb_type == 1] = -1
    return [np.ascontiguousarray(a) for a in (mb_type, qp, nnz, t8, mv, ref)]


# (content, blocky offsets, QP range, filter offsets): QP 0..51 over everything; the flat picture also at QPs where every edge it has is filtered
DEBLOCK = [("ramp", False, 0, 51, (0, 0, 0)), ("satnoise", False, 0, 51, (3, -2, 2)), ("flat128", True, 0, 51, (-6, 6, -4)), ("flat128", True, 30, 51, (0, 0, 0))]


def test_deblock_on_tiny_pictures(ctx, hip_lib, oracle_lib):
    d = ctx.dims
    n = d.mb_w * d.mb_h
    changed_flat = 0
    for i, (kind, blocks, qlo, qhi, (a_off, b_off, c_off)) in enumerate(DEBLOCK):
        for seed in range(3):                          # three draws of the side information per input
            r = np.random.RandomState(1000 * i + 10 * seed + d.mb_w + 4 * d.mb_h)
            y, u, v = (a[0] for a in E.content(kind, d.width, d.height, 1))
            if blocks:
                y, u, v = blocky(blocky(y, r, 4, 3), r, 16, 6), blocky(u, r, 4, 4), blocky(v, r, 4, 4)
            pic = ctx.new_picture()
            hp = load(ctx, pic, (y, u, v), oracle_lib)
            arrs = side_info(r, n, qlo, qhi)
            bufs = [DeviceArray(hip_lib, a.shape, a.dtype, a) for a in arrs]
            p = DeblockParams(mb_type=bufs[0].ptr, qp=bufs[1].ptr, nnz=bufs[2].ptr, transform8x8=bufs[3].ptr, mv=bufs[4].ptr, ref=bufs[5].ptr,
                              alpha_c0_offset=a_off, beta_offset=b_off, chroma_qp_offset=c_off)
            assert hip_lib.x264hip_deblock_frame(ctx.h, C.byref(pic), C.byref(p)) == 0, hip_lib.x264hip_last_error()
            ctx.sync()
            oracle_lib.x264o_frame_deblock(hp.ptr("y"), hp.ptr("u"), hp.ptr("v"), d.mb_w, d.mb_h, d.stride_y, d.stride_c,
                                           *[a.ctypes.data_as(C.c_void_p) for a in arrs], a_off, b_off, c_off)
            for name, src in (("y", y), ("u", u), ("v", v)):
                _eq(ctx.download(pic, name, padded=False), hp.visible(name), "%s draw %d: deblocked %s" % (kind, seed, name))
                if blocks and qlo >= 30:
                    changed_flat += int((hp.visible(name)[:src.shape[0], :src.shape[1]] != src).sum())
            for b in bufs:
                b.free()
    # offsets of up to 9 between 4x4 blocks of a flat picture at QP >= 30 (alpha >= 25, beta >= 8): the twin's filter acts on them whatever
    # the side information says about strengths 1..4; only a picture whose edges all have strength 0 stays untouched
    assert changed_flat > 0, "the loop filter changed nothing in the blocky flat pictures"
