"""The reference's per-macroblock path + the harness around it (oracle/ref_slice.c) under clang's MemorySanitizer (oracle/msan_main.c,
`make -C oracle msan`): no use of uninitialised memory in configurations that once had one.  What the sanitizer found so far is pinned in the
harness and listed in DESIGN.md 4 (the lowres border columns and corner sample, the "temporal predictors" taken from an I picture's never-written
ref / mv arrays): a reference whose output depends on what its process did before cannot be a checker.  CPU only; needs /root/reference."""
import os
import subprocess
import sys

import pytest

from paths import ROOT

REF = "/root/reference/x264-snapshot-20090216-2245"
CLANG = "/opt/rocm/lib/llvm/bin/clang"


@pytest.mark.skipif(not os.path.isdir(REF) or not os.path.exists(CLANG), reason="needs the reference sources and clang (MemorySanitizer)")
@pytest.mark.parametrize("seed,chain", [(1, 1), (6, 0)])
def test_reference_stream_run_is_free_of_uninitialised_reads(tmp_path, seed, chain):
    """seed 1 / chain 1: a scene cut makes input 2 an I picture that is not an IDR; the next P picture's x264_mb_predict_mv_ref16x16 read its ref[0]
    array, which nothing had written (R/common/macroblock.c:420-441) -- on the GPU box, inside a long pytest process, that changed the reference's
    payload (471 vs 488 bytes) and failed tests/test_gpu_stream.py once."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "msan"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the MemorySanitizer build failed here: " + r.stderr[-300:])
    job = str(tmp_path / "job.bin")
    subprocess.run([sys.executable, os.path.join(ROOT, "scratch", "dump_ref_job.py"), str(seed), str(chain), job], check=True, capture_output=True)
    env = dict(os.environ, MSAN_SYMBOLIZER_PATH="/opt/rocm/lib/llvm/bin/llvm-symbolizer")
    run = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "msan", "refslice_msan"), job], capture_output=True, text=True, env=env, timeout=600)
    assert "MemorySanitizer" not in run.stderr, run.stderr[:3000]
    assert run.returncode == 0 and "rc 0" in run.stdout, (run.returncode, run.stdout[-300:])
