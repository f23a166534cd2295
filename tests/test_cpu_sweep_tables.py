"""CPU: the two tables the host side of the sweep walks (x264_vs2008_amd/csrc/sweep_tables.h) -- the device arrays of an x264hip_mb_state and
the kernel kinds of a sweep -- compiled for the host with the address and undefined-behaviour sanitizers (tests/sweep_tables_host.cpp) and held
to the lists and the arithmetic they replaced: every array of the state once, in the allocation order, with its size; and for every mix of
0..2 entries per kind, where a chain-table launch places each entry and which kernels it enqueues, in which order, on which stream."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_tables_equal_the_lists_they_replaced(tmp_path):
    exe = str(tmp_path / "sweep_tables_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "x264_vs2008_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sweep_tables_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.strip().endswith("19683 mixes, 0 failures"), r.stdout[-4000:]
