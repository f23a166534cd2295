"""Helpers of the device-import tests (tests/test_gpu_import.py, tests/test_gpu_import_stream.py): small pictures with content that shows a wrong
replicated column or row, the layout conversions of x264hip_picture_import restated in numpy (plane swap, vertical flip, U/V interleave, pitched
rows), and device surfaces that END at the last visible byte of their allocation."""
import numpy as np

from x264_vs2008_amd.frame import CSP_I420, CSP_NV12, CSP_VFLIP, CSP_YV12, DeviceArray

LAYOUTS = {"i420": CSP_I420, "yv12": CSP_YV12, "nv12": CSP_NV12}
FLIPS = ("top_down", "vflip_flag", "negative_pitch")
PITCHES = ("w", "w+1", "w+13", "4w")
OFFSETS = (0, 1, 2, 3, 8)
GAP, POISON = 0xA5, 0x5A


def content(w, h, b, t=0):
    """I420 planes of batch element b at time t: a moving integer texture whose neighbouring columns and rows all differ; element 1 has an
    all-255 luma and an all-0 U plane, element 2 an all-0 luma and an all-255 V plane (every third element on), so that a column replicated
    from the wrong place, or from outside the surface, shows."""
    def tex(ww, hh, k):
        r, c = np.mgrid[0:hh, 0:ww]
        return ((c * 7 + r * 13 + (r * c) % 11 + 29 * b + 5 * t + 3 * ((c + 2 * t) // 5) + 61 * k) & 255).astype(np.uint8)
    y, u, v = tex(w, h, 0), tex(w // 2, h // 2, 1), tex(w // 2, h // 2, 2)
    if b % 3 == 1:
        y[:], u[:] = 255, 0
    if b % 3 == 2:
        y[:], v[:] = 0, 255
    return y, u, v


def pitch_of(row_bytes, mode):
    return {"w": row_bytes, "w+1": row_bytes + 1, "w+13": row_bytes + 13, "4w": 4 * row_bytes}[mode]


def stored_planes(y, u, v, layout):
    """The planes a surface of this layout stores, in its plane order: the conversion FROM I420 whose inverse the kernel performs."""
    if layout == "i420":
        return [y, u, v]
    if layout == "yv12":
        return [y, v, u]
    uv = np.empty((u.shape[0], 2 * u.shape[1]), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = u, v
    return [y, uv]


def pitched(img, pitch, bottom_up):
    """The bytes of a stored plane: row r at r * pitch, the rows bottom-up if asked, GAP between the rows, nothing after the last row's last byte."""
    rows = img[::-1] if bottom_up else img
    out = np.full((rows.shape[0] - 1) * pitch + rows.shape[1], GAP, np.uint8)
    for r in range(rows.shape[0]):
        out[r * pitch:r * pitch + rows.shape[1]] = rows[r]
    return out


def raw_frame(y, u, v, layout, vflip):
    """One frame of a raw file in this layout (pitch = row bytes)."""
    return b"".join(pitched(p, p.shape[1], vflip).tobytes() for p in stored_planes(y, u, v, layout))


class Surface:
    """One picture in device memory: every stored plane starts `offset` bytes past a 16-byte boundary (the allocation is 256-byte aligned), the
    planes are separated by GAP bytes, and plane `last` is the one that ends exactly where the allocation ends."""

    def __init__(self, lib, y, u, v, layout, flip, pitch_mode, offset, last=0):
        planes = stored_planes(y, u, v, layout)
        order = [k for k in range(len(planes)) if k != last % len(planes)] + [last % len(planes)]
        blobs, pos, where = [], 0, {}
        for k in order:
            pitch = pitch_of(planes[k].shape[1], pitch_mode)
            lead = (offset - pos) % 16 + 16
            blobs.append(np.full(lead, GAP, np.uint8))
            data = pitched(planes[k], pitch, flip != "top_down")
            where[k] = (pos + lead, pitch, planes[k].shape[0])
            blobs.append(data)
            pos += lead + data.size
        host = np.concatenate(blobs)
        self.dev = DeviceArray(lib, host.shape, np.uint8, host)
        assert self.dev.ptr % 16 == 0
        self.csp = LAYOUTS[layout] | (CSP_VFLIP if flip == "vflip_flag" else 0)
        self.ptrs, self.pitches = [None] * 3, [0] * 3
        for k, (at, pitch, rows) in where.items():
            if flip == "negative_pitch":        # the reference's own form of VFLIP: the pointer at the last stored row, the stride negated
                at, pitch = at + (rows - 1) * pitch, -pitch
            self.ptrs[k], self.pitches[k] = self.dev.ptr + at, pitch
        assert where[order[-1]][0] + (where[order[-1]][2] - 1) * where[order[-1]][1] + planes[order[-1]].shape[1] == host.size

    def entry(self, element):
        return (element, self.csp, tuple(self.ptrs), tuple(self.pitches))

    def free(self):
        self.dev.free()


def element_bytes(ctx, name):
    """Bytes between batch elements of a plane: the padded plane plus one row of slack, rounded to 256 (include/x264hip.h: Batching)."""
    stride, _, lines, _, padv = ctx.geometry(None, name)
    return (stride * (lines + 2 * padv + 1) + 255) // 256 * 256


def poison(ctx, pic, value=POISON):
    """Every byte of the Y, U and V planes of every element, padding included, becomes `value` (written around the library's own upload)."""
    import ctypes as C
    for i, name in enumerate("yuv"):
        stride, _, lines, padh, padv = ctx.geometry(pic, name)
        img = np.full((lines + 2 * padv) * stride, value, np.uint8)
        for b in range(ctx.batch):
            base = pic.plane[i] - (padv * stride + padh) + b * element_bytes(ctx, name)
            assert ctx.lib.x264hip_memcpy_h2d(base, img.ctypes.data_as(C.c_void_p), img.size) == 0


def interior(ctx, pic, name, full):
    """(coded area, copy of the padded plane with the coded area overwritten by POISON) of a download(padded=True)."""
    stride, w16, lines, padh, padv = ctx.geometry(pic, name)
    inner = full[padv:padv + lines, padh:padh + w16].copy()
    outer = full.copy()
    outer[padv:padv + lines, padh:padh + w16] = POISON
    return inner, outer
