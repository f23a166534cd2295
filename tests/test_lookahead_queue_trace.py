"""CPU: everything the library's frame queue answers (csrc/lookahead_host.hip through x264_vs2008_amd.lookahead.Lookahead) against a
recorded trace -- tests/look_trace.py drives it with made-up costs over 200 seeded configurations (b-adapt 2 with 1 to 16 B pictures,
b-adapt 1 and 0, the pre-encode scene cut on and off, keyint limits inside a decision, CQP and CRF) and writes down every get(): its
kind, the needs in the order returned, every field of a frame handed out (f_qpm as its bits), what scenecut() returned.  The fixture
(tests/golden/look_queue_trace.npz) was recorded from the library as it was BEFORE its path search and queue state were restated, so it
pins the order of the questions a decision asks and what save() / restore() bring back, which no picture-based test sees on a CPU.

Its size (some 220 KB) is what 200 configurations of 40 to 120 pictures take: 16 000 frames handed out at 12 fields each, of which the
CRF ones' f_qpm and i_satd do not compress, and 190 000 needs at about half a byte."""
import numpy as np
import pytest

import look_trace as T
from x264_vs2008_amd import lib as L

with np.load(T.FIXTURE) as _g:
    GOLD = T.decode(_g)


def test_fixture_holds_every_configuration():
    assert sorted(GOLD) == T.SEEDS and len(T.SEEDS) >= 200


@pytest.mark.parametrize("ahead", [True, False], ids=["ran_ahead_and_restored", "never_ran_ahead"])
@pytest.mark.parametrize("group", range(8))
def test_queue_trace_equals_recorded(group, ahead):
    """ahead: between save() and restore() the queue is run on (end, put, get, end ...); otherwise the pictures are only put.  The same
    trace is expected of both: restore() must bring back all a decision can change, and queue again what was put in between."""
    lib = L.open_library()
    for seed in T.SEEDS[group::8]:
        got, want = T.run(lib, seed, ahead), GOLD[seed]
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        assert got == want, "%s: record %d of %d / %d is %s, recorded %s" % (T.config(seed), first, len(got), len(want), got[first:first + 1], want[first:first + 1])


def test_fixture_covers_what_it_is_for():
    cov = T.coverage(GOLD)
    assert set(range(6)) <= set(cov["b_runs"]), cov          # b-adapt 2 chose every run of B pictures from none to five (and longer ones)
    assert cov["cut_short"] > 0, cov                         # a path's pricing ended at the threshold
    assert cov["restores_with_puts"] > 0, cov                # restore() had pictures to queue again
    assert cov["scenecuts"] == [1, 2], cov                   # scenecut(): the same picture again, and another one
