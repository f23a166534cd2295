"""CPU: the RD trials' bit count (x264_vs2008_amd/csrc/cabac_price.h: residual blocks walked from nonzero masks that the wave ballots first)
compiled for the host, a loop over 64 lanes standing for the ballot (tests/cabac_price_host.cpp), held to cw_macroblock(rd = 1) on the same
u8 states: the count f8, all 460 states and the syntax record afterwards, over random records of every macroblock type and partition the writer
takes; and the masks to a plain loop over the coefficient arrays whose unread entries are 0xAA.  No record is excluded.  (The same file with
-DCABAC_PRICE_HOST_MAIN is a program of its own for a sanitizer build.)"""
import ctypes as C
import os
import subprocess

import pytest

from paths import ROOT

N = 20000
N_STATS = 160
T_I_4x4, T_I_8x8, T_I_16x16, T_I_PCM, T_P_L0, T_P_8x8, T_B_DIRECT, T_B_L0_L0, T_B_8x8 = 0, 1, 2, 3, 4, 5, 7, 8, 17


@pytest.fixture(scope="module")
def price_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cabac_price_host") / "libcabac_price_host.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "x264_vs2008_amd", "csrc"), os.path.join(ROOT, "tests", "cabac_price_host.cpp"), "-o", out], check=True)
    lib = C.CDLL(out)
    lib.cabac_price_host_run.restype = C.c_int
    lib.cabac_price_host_run.argtypes = [C.c_int, C.c_int, C.c_uint, C.POINTER(C.c_longlong)]
    return lib


@pytest.mark.parametrize("slice_type", [0, 1, 2], ids=["P", "B", "I"])
def test_price_equals_the_lane0_count(price_lib, slice_type):
    stats = (C.c_longlong * N_STATS)()
    bad = price_lib.cabac_price_host_run(slice_type, N, 1, stats)
    s = list(stats)
    print("slice type %d: %d records, %d differ; per type %s; sub-partitions %s; level patterns per category %s; magnitudes 1 2 14 15 16 2000: %s"
          % (slice_type, N, bad, s[0:19], s[32:45], [s[64 + 8 * c:64 + 8 * c + 6] for c in range(6)], s[128:134]))
    assert bad == 0
    # what the records covered: every type of the slice, every sub-partition, every level pattern of every block category, the unary cap and the
    # bypass escape, counts / coded-block patterns that disagree with the levels, both transforms, one and three references
    types = {0: [T_I_4x4, T_I_8x8, T_I_16x16, T_I_PCM, T_P_L0, T_P_8x8], 1: [T_I_4x4, T_I_8x8, T_I_16x16, T_I_PCM, T_B_DIRECT, T_B_8x8] + list(range(T_B_L0_L0, T_B_8x8)),
             2: [T_I_4x4, T_I_8x8, T_I_16x16, T_I_PCM]}[slice_type]
    assert sum(s[0:19]) == N and all(s[t] > 100 for t in types)
    if slice_type == 0:
        assert all(s[32 + k] > 100 for k in (0, 1, 2, 3))
    if slice_type == 1:
        assert all(s[32 + k] > 100 for k in (3, 7, 11, 12))
    assert all(s[64 + 8 * c + k] > 100 for c in range(6) for k in range(6))
    assert all(v > 1000 for v in s[128:134])
    assert s[140] > 1000 and s[141] > 20 * N and 1000 < s[142] < N - 1000 and 1000 < s[143] < N - 1000
