"""The twin (oracle/liboracle.so) against the reference's own loop (oracle/_ref/libx264ref.so, built here from the reference's
sources) on the seeded random chains of tests/fuzz_b.py -- payload bytes of every frame.  This is the first hop of the GPU's
random-chain parity (kernel == twin in tests/test_gpu_fuzz_cases.py, twin == reference here); it found a twin bug in round 2
(`--nr` during analysis).  Where the reference library is not built, the reference's side is the md5s of tests/golden/ref_offline.npz
(oracle/gen_golden_ref_offline.py)."""
import hashlib
import os

import numpy as np
import pytest

import fuzz_b
from fuzz_b import ARRAYS, SEEDS
from oracle import refslice as rs
from paths import REF_SO, ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_offline.npz")


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("seed", SEEDS)
def test_twin_equals_reference_on_random_chain(oracle_lib, seed):
    w, h, frames, kind, kw, ekw, y, u, v = fuzz_b.config(seed)
    a = rs.run2(oracle_lib, "x264o_encode_chain2", rs.make_params(w, h, frames, **kw), rs.make_ext(**ekw), y, u, v)
    if not os.path.exists(REF_SO):                   # the reference's answers as stored
        with np.load(FIXTURE) as g:
            want = [str(x) for x in g["rc%d_payload" % seed]]
            bad = [f for f in range(frames) if md5(a["payload"][f, :a["payload_len"][f]]) != want[f]]
            assert len(want) == frames and not bad, "%dx%d x%d %s %s %s: payload of frames %s differs between the twin and the reference" % (w, h, frames, kind, kw, ekw, bad)
            for k in ARRAYS:
                assert md5(a[k]) == str(g["rc%d_%s" % (seed, k)]), k
        return
    b = rs.run_reference2(rs.make_params(w, h, frames, **kw), rs.make_ext(**ekw), y, u, v)
    bad = [f for f in range(frames) if bytes(a["payload"][f, :a["payload_len"][f]]) != bytes(b["payload"][f, :b["payload_len"][f]])]
    assert not bad, "%dx%d x%d %s %s %s: payload of frames %s differs between the twin and the reference" % (w, h, frames, kind, kw, ekw, bad)
    for k in ARRAYS:
        assert (a[k] == b[k]).all(), k
