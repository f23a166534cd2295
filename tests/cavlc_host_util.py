"""Helper of tests/test_cavlc_host.py: the product's CAVLC writer compiled for the host (tests/cavlc_host.cpp: csrc/cavlc_dev.h with g++,
no HIP), and one frame of harness output (oracle/refslice.py's arrays, the reference's or the CPU twin's) through it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from paths import ROOT
from x264_vs2008_amd.slice import PAYLOAD_LEAD, CavlcParams, MbState

MB_BYTES_MAX = 2624           # CV_MB_BYTES_MAX (csrc/frame_cavlc.hip): the margin of both entry points, every slice type
STATE_ARRAYS = ("mb_type", "partition", "sub_partition", "ref", "ref1", "mv", "mv1", "i4mode", "i16mode", "chroma_mode", "qp", "cbp", "t8",
                "luma", "luma_dc", "chroma_dc", "chroma_ac")
_lib = []


def host_writer():
    """The driver as a shared library, built once per session."""
    if not _lib:
        out = os.path.join(tempfile.mkdtemp(prefix="cavlc_host_"), "libcavlc_host.so")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "x264_vs2008_amd", "csrc"), os.path.join(ROOT, "tests", "cavlc_host.cpp"), "-o", out], check=True)
        lib = C.CDLL(out)
        lib.cavlc_host_write_slice.restype = C.c_int
        lib.cavlc_host_write_slice.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        _lib.append(lib)
    return _lib[0]


def restore_8x8_levels(a, twin):
    """Harness output `a` of the reference with field `luma` completed from the CPU twin's output for the same clip and parameters.
    oracle/ref_slice.c keeps the levels of 8x8 block i of a macroblock only where nnz[4 * i] is set.  It reads nnz after the writer, and
    the CAVLC writer has by then stored the totals of the block's four interleaved lists there, so a coded 8x8 block whose first list is
    empty but whose others are not is recorded as zeros.  Exactly those blocks (t8 set, cbp bit i set, nnz[4i] == 0, one of
    nnz[4i+1 .. 4i+3] not) take the twin's 64 levels; the twin's mb_type, cbp and t8 of such a macroblock must be the reference's."""
    luma = a["luma"].copy()
    for i in range(4):
        lost = (a["t8"] == 1) & ((a["cbp"] >> i & 1) == 1) & (a["nnz"][..., 4 * i] == 0) & a["nnz"][..., 4 * i + 1:4 * i + 4].any(-1)
        for k in ("mb_type", "cbp", "t8"):
            assert (twin[k][lost] == a[k][lost]).all(), "the twin's %s differs from the reference's where levels are to be restored" % k
        luma[lost, 64 * i:64 * i + 64] = twin["luma"][lost, 64 * i:64 * i + 64]
    return dict(a, luma=luma)


def write_state(st, mb_w, mb_h, slice_type, slice_qp, n_ref0=1, inter=0x33, transform8x8=0, cqm_custom=0, cap=None, margin=MB_BYTES_MAX, slots=1, fill=0):
    """One chain's state arrays ({name: array of mb_w * mb_h macroblocks}, STATE_ARRAYS) through the host writer into slot 0 of a buffer of
    `slots` slots of cap bytes filled with `fill`.  Returns (0 or the writer's stop count, the whole buffer [slots][cap], payload_len,
    mb_bits [n_mb])."""
    st = {k: np.ascontiguousarray(st[k]) for k in STATE_ARRAYS}
    cap = cap or PAYLOAD_LEAD + MB_BYTES_MAX + mb_w * mb_h * 1200
    payload, plen, bits = np.full((slots, cap), fill, np.uint8), np.zeros(1, np.int32), np.zeros(mb_w * mb_h, np.int32)
    state = MbState(**{k: st[k].ctypes.data for k in STATE_ARRAYS})
    par = CavlcParams(slice_type, n_ref0, inter, transform8x8, cqm_custom, payload.ctypes.data, cap, plen.ctypes.data, bits.ctypes.data, slice_qp)
    rc = host_writer().cavlc_host_write_slice(C.byref(state), C.byref(par), mb_w, mb_h, margin)
    return rc, payload, int(plen[0]), bits


def write_slice(a, f, p, cap=None):
    """The host writer's bytes for frame f of harness output `a`: its arrays as one chain's x264hip_mb_state, slice type / QP / list-0 size
    from the harness's frame_info, p the rs.Params the arrays were made with."""
    mb_w, mb_h = (p.width + 15) // 16, (p.height + 15) // 16
    slice_type, slice_qp, n_ref0 = (int(v) for v in a["frame_info"][f, :3])
    rc, payload, plen, _ = write_state({k: a[k][f] for k in STATE_ARRAYS}, mb_w, mb_h, slice_type, slice_qp, n_ref0, p.inter, p.transform8x8,
                                       int(p.cqm_preset != 0), cap)
    assert rc == 0, "the host writer stopped (%d) in frame %d" % (rc, f)
    return bytes(payload[0, PAYLOAD_LEAD:PAYLOAD_LEAD + plen])
