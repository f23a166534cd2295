"""Helper of tests/test_cavlc_mp_host.py: the macroblock-parallel form of the product's CAVLC writer compiled for the host
(tests/cavlc_mp_host.cpp: count, scan and place of csrc/cavlc_dev.h in reverse raster order, and cv_write_slice beside them), built the way
tests/cavlc_host_util.py builds the serial writer's driver; and the same file as a program of its own under the sanitizers."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from cavlc_host_util import MB_BYTES_MAX, STATE_ARRAYS
from paths import ROOT
from x264_vs2008_amd.slice import PAYLOAD_LEAD, CavlcParams, MbState

SOURCE = os.path.join(ROOT, "tests", "cavlc_mp_host.cpp")
FLAGS = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "x264_vs2008_amd", "csrc")]
_lib = []


def host_writers():
    """The driver as a shared library, built once per session."""
    if not _lib:
        out = os.path.join(tempfile.mkdtemp(prefix="cavlc_mp_host_"), "libcavlc_mp_host.so")
        subprocess.run(FLAGS + ["-shared", "-fPIC", SOURCE, "-o", out], check=True)
        lib = C.CDLL(out)
        for fn in (lib.cavlc_mp_host_write_slice, lib.cavlc_mp_host_write_slice_serial):
            fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        _lib.append(lib)
    return _lib[0]


def sanitized_program():
    """The same source with its own main (made-up slices, both writers, a slot that ends with its buffer) under AddressSanitizer and
    UndefinedBehaviorSanitizer: the path of the program."""
    out = os.path.join(tempfile.mkdtemp(prefix="cavlc_mp_host_"), "cavlc_mp_host")
    subprocess.run(FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DCAVLC_MP_HOST_MAIN", SOURCE, "-o", out], check=True)
    return out


def write_state_both(st, mb_w, mb_h, slice_type, slice_qp, n_ref0=1, inter=0x33, transform8x8=0, cqm_custom=0, cap=None, margin=MB_BYTES_MAX, slots=1, fill=0):
    """One chain's state arrays (cavlc_host_util.write_state's arguments) through cv_write_slice and through count / scan / place, each into
    slot 0 of a buffer of its own of `slots` slots of cap bytes filled with `fill`.  Returns two tuples (serial, macroblock-parallel) of
    (stop count, the whole buffer [slots][cap], payload_len, mb_bits [n_mb])."""
    st = {k: np.ascontiguousarray(st[k]) for k in STATE_ARRAYS}
    cap = cap or PAYLOAD_LEAD + MB_BYTES_MAX + mb_w * mb_h * 1200
    state = MbState(**{k: st[k].ctypes.data for k in STATE_ARRAYS})
    out = []
    for fn in (host_writers().cavlc_mp_host_write_slice_serial, host_writers().cavlc_mp_host_write_slice):
        payload, plen, bits = np.full((slots, cap), fill, np.uint8), np.full(1, -1, np.int32), np.full(mb_w * mb_h, -1, np.int32)
        par = CavlcParams(slice_type, n_ref0, inter, transform8x8, cqm_custom, payload.ctypes.data, cap, plen.ctypes.data, bits.ctypes.data, slice_qp)
        rc = fn(C.byref(state), C.byref(par), mb_w, mb_h, margin)
        out.append((rc, payload, int(plen[0]), bits))
    return out


def check_equal(what, serial, mp, fill):
    """The macroblock-parallel pass against cv_write_slice: the same stop decision and payload_len; where the slice was written the same bytes
    and mb_bits, the lead bytes and everything behind the slice as they were.  Returns the slice's bytes."""
    (rc0, pay0, len0, bits0), (rc1, pay1, len1, bits1) = serial, mp
    assert (rc1, len1) == (rc0, len0), "%s: count / scan / place ends with (stops %d, %d bytes), cv_write_slice with (%d, %d)" % (what, rc1, len1, rc0, len0)
    if rc0:
        assert len1 == 0
        assert (pay1 == fill).all(), "%s: the stopped pass wrote %d bytes" % (what, (pay1 != fill).sum())
        return b""
    assert np.array_equal(bits1, bits0), "%s: mb_bits differ first at macroblock %d" % (what, np.flatnonzero(bits1 != bits0)[0])
    got, want = pay1[0, PAYLOAD_LEAD:PAYLOAD_LEAD + len1], pay0[0, PAYLOAD_LEAD:PAYLOAD_LEAD + len0]
    assert np.array_equal(got, want), "%s: the bytes differ first at byte %d of %d" % (what, np.flatnonzero(got != want)[0], len0)
    assert (pay1[0, :PAYLOAD_LEAD] == fill).all() and (pay1[0, PAYLOAD_LEAD + len1:] == fill).all() and (pay1[1:] == fill).all(), "%s: bytes outside the slice were written" % what
    return bytes(got)


def write_slice_both(a, f, p, what, fill=0x5A):
    """cavlc_host_util.write_slice through both writers: frame f of harness output `a`, compared (check_equal); the slice's bytes."""
    mb_w, mb_h = (p.width + 15) // 16, (p.height + 15) // 16
    slice_type, slice_qp, n_ref0 = (int(v) for v in a["frame_info"][f, :3])
    serial, mp = write_state_both({k: a[k][f] for k in STATE_ARRAYS}, mb_w, mb_h, slice_type, slice_qp, n_ref0, p.inter, p.transform8x8,
                                  int(p.cqm_preset != 0), fill=fill)
    assert serial[0] == 0, "%s frame %d: cv_write_slice stopped" % (what, f)
    return check_equal("%s frame %d" % (what, f), serial, mp, fill)
