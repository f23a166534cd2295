"""Helper of tests/test_psy_trellis_cpu.py: the product's scalar trellis quantiser compiled for the host (tests/psy_trellis_host.cpp:
csrc/trellis_dev.h with g++, no HIP), its entry without and its entry with the psy-trellis term."""
import ctypes as C
import os
import subprocess
import tempfile

from paths import ROOT

_lib = []


def host_trellis():
    """The driver as a shared library, built once per session."""
    if not _lib:
        out = os.path.join(tempfile.mkdtemp(prefix="psy_trellis_host_"), "libpsy_trellis_host.so")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "x264_vs2008_amd", "csrc"), os.path.join(ROOT, "tests", "psy_trellis_host.cpp"), "-o", out], check=True)
        lib = C.CDLL(out)
        common = [C.c_void_p] * 6 + [C.c_int] * 5
        lib.pt_host_context_init.restype, lib.pt_host_context_init.argtypes = None, [C.c_void_p, C.c_int, C.c_int, C.c_int]
        lib.pt_host_trellis.restype, lib.pt_host_trellis.argtypes = C.c_int, common
        lib.pt_host_trellis_psy.restype, lib.pt_host_trellis_psy.argtypes = C.c_int, common + [C.c_void_p, C.c_int]
        _lib.append(lib)
    return _lib[0]
