"""Helper of tests/test_cabac_pass_host.py: the product's CABAC pass compiled for the host (tests/cabac_pass_host.cpp: csrc/cabac_pass_dev.h
with g++, no HIP), and one frame of harness output (oracle/refslice.py's arrays, the reference's or the CPU twin's) through it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from paths import ROOT
from x264_vs2008_amd.abi import CabacParams, MbState
from x264_vs2008_amd.slice import MB_BYTES_MAX, PAYLOAD_LEAD

STATE_ARRAYS = ("mb_type", "partition", "sub_partition", "ref", "mv", "i4mode", "i16mode", "chroma_mode", "qp", "cbp", "t8", "nnz",
                "luma", "luma_dc", "chroma_dc", "chroma_ac")
_lib = []


def compile_driver(out, extra=()):
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "x264_vs2008_amd", "csrc"), os.path.join(ROOT, "tests", "cabac_pass_host.cpp"), "-o", out], check=True)


def host_pass():
    """The driver as a shared library, built once per session."""
    if not _lib:
        out = os.path.join(tempfile.mkdtemp(prefix="cabac_pass_host_"), "libcabac_pass_host.so")
        compile_driver(out, ("-shared", "-fPIC"))
        lib = C.CDLL(out)
        lib.cabac_pass_host_write_slice.restype = C.c_int
        lib.cabac_pass_host_write_slice.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        _lib.append(lib)
    return _lib[0]


def write_slice(a, f, p, cabac_init_idc=0, cap=None):
    """(bytes, mb_bits) of the host pass for frame f of harness output `a`: its arrays as one chain's x264hip_mb_state, slice type / QP /
    list-0 size from the harness's frame_info, p the rs.Params the arrays were made with.  The chain's frame f is the f-th coded."""
    st = {k: np.ascontiguousarray(a[k][f]) for k in STATE_ARRAYS}
    mb_w, mb_h = (p.width + 15) // 16, (p.height + 15) // 16
    cap = cap or PAYLOAD_LEAD + MB_BYTES_MAX + 128 + mb_w * mb_h * 1200
    payload, plen, bits = np.zeros(cap, np.uint8), np.zeros(1, np.int32), np.zeros(mb_w * mb_h, np.int32)
    state = MbState(**{k: st[k].ctypes.data for k in STATE_ARRAYS})
    slice_type, slice_qp, n_ref0 = (int(v) for v in a["frame_info"][f, :3])
    par = CabacParams(slice_type=slice_type, n_ref0=n_ref0, analyse_inter=p.inter, transform8x8=p.transform8x8, slice_qp=slice_qp,
                      cabac_init_idc=cabac_init_idc, i_frame=f, i_frame_stride=0, payload=payload.ctypes.data, payload_cap=cap,
                      payload_len=plen.ctypes.data, mb_bits=bits.ctypes.data)
    rc = host_pass().cabac_pass_host_write_slice(C.byref(state), C.byref(par), mb_w, mb_h)
    assert rc == 0, "the host pass stopped (%d) in frame %d" % (rc, f)
    return bytes(payload[PAYLOAD_LEAD:PAYLOAD_LEAD + int(plen[0])]), bits
