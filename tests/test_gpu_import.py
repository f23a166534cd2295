"""GPU: x264hip_picture_import -- device-resident I420 / YV12 / NV12 surfaces, top-down or bottom-up, with any pitch and alignment, into the batch
elements of a picture in one launch.  The yardstick is x264hip_picture_upload of the equivalent I420 planes (code this entry point shares
nothing with): the coded area of Y, U and V of every element must be the same bytes, and nothing outside it may be written."""
import ctypes as C

import numpy as np
import pytest

import import_util as U
from x264_vs2008_amd.abi import Surface
from x264_vs2008_amd.frame import CSP_I420, CSP_NV12, CSP_VFLIP, CSP_YV12, DeviceArray, FrameCtx

pytestmark = pytest.mark.gpu

# 16x16: one macroblock, nothing to replicate.  2x2: everything is replication.  38x22: chroma 19x11 (odd width, 4- and 16-byte tails, coded 48x32).
# 66x34: one byte past a 64-byte row.  208x144: the suite's usual picture.
SIZES = [(16, 16), (2, 2), (38, 22), (66, 34), (208, 144)]
BATCH = 3


class Case:
    """A context of BATCH elements for one size, the test pictures and what x264hip_picture_upload makes of them (computed once, never changed)."""

    def __init__(self, lib, w, h, batch=BATCH):
        self.lib, self.w, self.h = lib, w, h
        self.ctx = FrameCtx(lib, w, h, batch=batch)
        self.yuv = [U.content(w, h, b) for b in range(batch)]
        ref = self.ctx.new_picture(source_only=True)
        U.poison(self.ctx, ref)
        for b, (y, u, v) in enumerate(self.yuv):
            self.ctx.upload(ref, y, u, v, b=b)
        self.want = {(b, n): self.ctx.download(ref, n, padded=False, b=b) for b in range(batch) for n in "yuv"}
        for a in self.want.values():
            a.setflags(write=False)
        self.pic = self.ctx.new_picture(source_only=True)

    def check(self, elements, what, pic=None):
        """The named elements hold upload's coded area; every other byte of every element is still POISON."""
        pic = self.pic if pic is None else pic
        for b in range(self.ctx.batch):
            for n in "yuv":
                inner, outer = U.interior(self.ctx, pic, n, self.ctx.download(pic, n, padded=True, b=b))
                assert (outer == U.POISON).all(), "%s: element %d plane %s: written outside the coded area at %s" % (what, b, n, np.argwhere(outer != U.POISON)[0])
                if b in elements:
                    if not np.array_equal(inner, self.want[b, n]):
                        bad = np.argwhere(inner != self.want[b, n])
                        raise AssertionError("%s: element %d plane %s: %d bytes differ from upload's, first at (row, col) %s: %d, upload has %d"
                                             % (what, b, n, len(bad), bad[0], inner[tuple(bad[0])], self.want[b, n][tuple(bad[0])]))
                else:
                    assert (inner == U.POISON).all(), "%s: element %d plane %s was not named and was written" % (what, b, n)


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: "%dx%d" % s)
def case(request, hip_lib):
    c = Case(hip_lib, *request.param)
    yield c
    c.ctx.close()


def test_upload_yardstick_replicates(case):
    """What the comparison stands on: upload's coded area is the visible picture with its last column and row replicated (numpy)."""
    d = case.ctx.dims
    for b, planes in enumerate(case.yuv):
        for n, p in zip("yuv", planes):
            w16, h16 = (d.mb_w * 16, d.lines_y) if n == "y" else (d.mb_w * 8, d.lines_c)
            assert np.array_equal(case.want[b, n], np.pad(p, ((0, h16 - p.shape[0]), (0, w16 - p.shape[1])), mode="edge"))


@pytest.mark.parametrize("flip", U.FLIPS)
@pytest.mark.parametrize("layout", sorted(U.LAYOUTS))
def test_layouts_pitches_and_alignment(case, layout, flip):
    """Every layout, top-down, bottom-up by flag and bottom-up by negative pitch, at pitch = row bytes, + 1, + 13 and x 4, with the plane
    bases 0, 1, 2, 3 and 8 bytes past a 16-byte boundary; every surface ends with its allocation."""
    ctx = case.ctx
    for pitch_mode in U.PITCHES:
        for offset in U.OFFSETS:
            what = "%dx%d %s %s pitch %s offset %d" % (case.w, case.h, layout, flip, pitch_mode, offset)
            U.poison(ctx, case.pic)
            surfaces = [U.Surface(case.lib, *case.yuv[b], layout, flip, pitch_mode, offset, last=b) for b in range(BATCH)]
            try:
                ctx.import_surfaces(case.pic, [s.entry(b) for b, s in enumerate(surfaces)])
                ctx.sync()
                case.check(range(BATCH), what)
            finally:
                for s in surfaces:
                    s.free()


def test_selected_element_is_neither_read_nor_changed(case):
    ctx = case.ctx
    U.poison(ctx, case.pic)
    ctx.select(2)
    s = U.Surface(case.lib, *case.yuv[0], "nv12", "top_down", "w+13", 1)
    try:
        ctx.import_surfaces(case.pic, [s.entry(0)])
        ctx.sync()
        got = ctx.download(case.pic, "y", padded=False)            # no b: the element selected before the import
        assert (got == U.POISON).all(), "the import went to the selected element, or changed the selection"
        case.check([0], "one entry while element 2 is selected")
    finally:
        s.free()
        ctx.select(0)


def test_subsets_keep_the_other_elements(hip_lib):
    """Batch of 4, entries for elements 2 and 0 in that order: 1 and 3 keep every byte, padding included, and 2 and 0 keep their outer padding."""
    c = Case(hip_lib, 38, 22, batch=4)
    try:
        U.poison(c.ctx, c.pic)
        before = {(b, n): c.ctx.download(c.pic, n, padded=True, b=b) for b in (1, 3) for n in "yuv"}
        s2 = U.Surface(hip_lib, *c.yuv[2], "nv12", "vflip_flag", "w+13", 3, last=1)
        s0 = U.Surface(hip_lib, *c.yuv[0], "yv12", "top_down", "w+1", 0, last=2)
        try:
            c.ctx.import_surfaces(c.pic, [s2.entry(2), s0.entry(0)])
            c.ctx.sync()
            for (b, n), a in before.items():
                assert np.array_equal(c.ctx.download(c.pic, n, padded=True, b=b), a), "element %d plane %s was not named and changed" % (b, n)
            c.check([2, 0], "subset {2, 0} of 4")
        finally:
            s2.free(); s0.free()
    finally:
        c.ctx.close()


def test_two_imports_and_expand_border_with_one_sync(hip_lib):
    """Ordering on the context's stream: two imports into two pictures and x264hip_expand_border behind each, one synchronisation at the end;
    the padded planes equal upload + expand."""
    w, h = 66, 34
    ctx = FrameCtx(hip_lib, w, h, batch=2)
    try:
        clips = [[U.content(w, h, b, t) for b in range(2)] for t in range(2)]
        want = []
        for t in range(2):
            ref = ctx.new_picture(source_only=True)
            for b, (y, u, v) in enumerate(clips[t]):
                ctx.upload(ref, y, u, v, b=b)
            ctx.check(hip_lib.x264hip_expand_border(ctx.h, C.byref(ref), 0), "expand_border")
            want.append({(b, n): ctx.download(ref, n, padded=True, b=b) for b in range(2) for n in "yuv"})
        pics = [ctx.new_picture(source_only=True) for _ in range(2)]
        surfaces = [[U.Surface(hip_lib, *clips[t][b], ("nv12", "i420")[t], ("top_down", "negative_pitch")[b], "w+13", 2 * t + b, last=b) for b in range(2)] for t in range(2)]
        try:
            for t in range(2):
                ctx.import_surfaces(pics[t], [s.entry(b) for b, s in enumerate(surfaces[t])])
            for t in range(2):
                ctx.check(hip_lib.x264hip_expand_border(ctx.h, C.byref(pics[t]), 0), "expand_border")
            ctx.sync()
            for t in range(2):
                for (b, n), a in want[t].items():
                    assert np.array_equal(ctx.download(pics[t], n, padded=True, b=b), a), "picture %d element %d plane %s differs from upload + expand" % (t, b, n)
        finally:
            for row in surfaces:
                for s in row:
                    s.free()
    finally:
        ctx.close()


def _entries(rows):
    arr = (Surface * len(rows))()
    for e, (element, csp, planes, pitches) in zip(arr, rows):
        e.element, e.csp = element, csp
        for k in range(3):
            e.plane[k], e.pitch[k] = planes[k], pitches[k]
    return arr


def test_refusals_launch_nothing(hip_lib):
    """Every refusal of include/x264hip.h: -1, a message that names the reason, and the picture as it was.  (The plane addresses are those of
    a real surface: nothing here hands the kernel a bad pointer, and nothing is launched.)"""
    w, h = 38, 22
    c = Case(hip_lib, w, h)
    lib, ctx = hip_lib, c.ctx
    nbytes = lib.x264hip_surface_bytes() * 4
    host, table = lib.x264hip_host_alloc(nbytes), DeviceArray(lib, (nbytes,), np.uint8)
    s = U.Surface(lib, *c.yuv[0], "i420", "top_down", "w", 0)
    n = U.Surface(lib, *c.yuv[1], "nv12", "top_down", "w", 0)
    try:
        U.poison(ctx, c.pic)
        good, p, q = s.entry(0), tuple(s.ptrs), tuple(s.pitches)
        nv = n.entry(1)
        cases = [
            ("n = 0", [good], 0, host, table.p, "surfaces for a batch"),
            ("n > batch", [s.entry(b % 3) for b in range(4)], 4, host, table.p, "surfaces for a batch"),
            ("element below the batch", [(-1, CSP_I420, p, q)], 1, host, table.p, "outside the batch"),
            ("element beyond the batch", [(3, CSP_I420, p, q)], 1, host, table.p, "outside the batch"),
            ("element named twice", [good, nv, s.entry(0)], 3, host, table.p, "named twice"),
            ("unknown csp", [(0, 0x0002, p, q)], 1, host, table.p, "unknown csp"),
            ("no csp", [(0, CSP_VFLIP, p, q)], 1, host, table.p, "unknown csp"),
            ("two layouts at once", [(0, CSP_I420 | CSP_NV12, p, q)], 1, host, table.p, "unknown csp"),
            ("NULL luma", [(0, CSP_I420, (None, p[1], p[2]), q)], 1, host, table.p, "is NULL"),
            ("NULL third plane of I420", [(0, CSP_I420, (p[0], p[1], None), q)], 1, host, table.p, "is NULL"),
            ("NULL third plane of YV12", [(0, CSP_YV12, (p[0], p[1], None), q)], 1, host, table.p, "is NULL"),
            ("NULL UV plane of NV12", [(1, CSP_NV12, (nv[2][0], None, None), nv[3])], 1, host, table.p, "is NULL"),
            ("luma pitch below the width", [(0, CSP_I420, p, (w - 1, q[1], q[2]))], 1, host, table.p, "smaller than a row"),
            ("negative luma pitch below the width", [(0, CSP_I420, p, (-(w - 1), q[1], q[2]))], 1, host, table.p, "smaller than a row"),
            ("chroma pitch below the width", [(0, CSP_YV12, p, (q[0], q[1], w // 2 - 1))], 1, host, table.p, "smaller than a row"),
            ("NV12 pitch of one plane's chroma", [(1, CSP_NV12, nv[2], (w, w // 2, 0))], 1, host, table.p, "smaller than a row"),
            ("NV12 pitch one below", [(1, CSP_NV12, nv[2], (w, 2 * (w // 2) - 1, 0))], 1, host, table.p, "smaller than a row"),
            ("NULL staging", [good], 1, None, table.p, "staging / table"),
            ("NULL table", [good], 1, host, None, "staging / table"),
        ]
        for what, rows, count, st, tab, needle in cases:
            rc = lib.x264hip_picture_import(ctx.h, C.byref(c.pic), _entries(rows), count, st, tab)
            msg = lib.x264hip_last_error().decode()
            assert rc == -1, "%s: returned %d" % (what, rc)
            assert "picture_import" in msg and needle in msg, "%s: the message is %r" % (what, msg)
        ctx.sync()
        c.check([], "after every refusal")
        # the same table accepted once the entries are right: the refusals are the entries', not the buffers'
        rc = lib.x264hip_picture_import(ctx.h, C.byref(c.pic), _entries([good, nv]), 2, host, table.p)
        assert rc == 0, lib.x264hip_last_error().decode()
        ctx.sync()
        c.check([0, 1], "two good entries")
    finally:
        s.free(); n.free(); table.free()
        lib.x264hip_host_free(host)
        ctx.close()
