"""CPU: the reference outputs tests/test_gpu_full_batch.py holds every chain to (tests/golden/stream_batch_{med,slow}.npz, cavlc_batch_uf.npz;
the cases: tests/full_batch_util.py).
  * they still describe what that test needs: one record per input picture of every clip, I/P and B pictures mixed, for SLOW both
    direct modes among the B slices (else the batch's guards could pass on content that does not exercise them);
  * where oracle/_ref is built: oracle/gen_golden_stream.py and oracle/gen_golden_cavlc.py write them again byte for byte."""
import os

import numpy as np
import pytest

import full_batch_util as T
from oracle import refslice as rs
from oracle.gen_golden_stream import save_npz
from paths import ROOT


@pytest.mark.parametrize("name", sorted(T.FLAGS))
def test_batch_fixture_covers_what_the_full_batch_test_needs(name):
    gold = T.load_fixture(name)
    assert len(gold) == len(T.CLIPS[name])
    frames = T.FLAGS[name]["frames"]
    seqs, modes = set(), set()
    for a in gold:
        st = [int(x) for x in a["frame_info"][:frames, 0]]
        assert sorted(int(x) for x in a["frame_info2"][:frames, 0]) == list(range(frames))       # every input picture coded once
        assert all(0 < a["payload_len"][f] <= a["payload"].shape[1] for f in range(frames))
        seqs.add(tuple(st))
        modes |= {int(a["frame_info2"][f][3]) for f in range(frames) if st[f] == rs.SLICE_B}
    assert len(seqs) >= len(gold) // 2, "%s: the clips' frame-type sequences hardly differ" % name
    assert any(rs.SLICE_B in s for s in seqs) and any(rs.SLICE_B not in s for s in seqs)
    if name == "slow":
        assert modes == {0, 1}


@pytest.mark.skipif(not os.path.exists(T.REF_SO), reason="oracle/_ref/libx264ref.so not built (needs the reference tree)")
@pytest.mark.parametrize("name", sorted(T.FLAGS))
def test_batch_fixture_regenerates_byte_for_byte(tmp_path, name):
    out = {}
    for i, a in enumerate(T.reference(name)):
        for k, v in a.items():
            out["c%d_%s" % (i, k)] = v
    path = tmp_path / ("stream_batch_%s.npz" % name)
    save_npz(str(path), out)
    with open(os.path.join(ROOT, "tests", "golden", "stream_batch_%s.npz" % name), "rb") as f:
        assert path.read_bytes() == f.read()


def test_cavlc_batch_fixture_covers_the_wavefront_clips():
    gold = T.load_cavlc_fixture()
    assert len(gold) == len(T.LOCK_T0)
    for a in gold:
        assert all(0 < a["payload_len"][f] <= a["payload"].shape[1] for f in range(T.LOCK_WAVE["frames"]))
    assert len({bytes(a["payload"][0, :a["payload_len"][0]]) for a in gold}) == len(gold), "the clips' first pictures code alike"


@pytest.mark.skipif(not os.path.exists(T.REF_SO), reason="oracle/_ref/libx264ref.so not built (needs the reference tree)")
def test_cavlc_batch_fixture_regenerates_byte_for_byte(tmp_path):
    c, out = T.LOCK_WAVE, {}
    for i, t0 in enumerate(T.LOCK_T0):
        a = T.cavlc_reference(c, rs.clip(c["w"], c["h"], c["frames"], t0))
        out["c%d_payload" % i], out["c%d_payload_len" % i] = a["payload"], a["payload_len"]
    path = tmp_path / "cavlc_batch_uf.npz"
    save_npz(str(path), out)
    with open(os.path.join(ROOT, "tests", "golden", "cavlc_batch_uf.npz"), "rb") as f:
        assert path.read_bytes() == f.read()
