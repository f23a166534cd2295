"""CPU: the twin (oracle/liboracle.so) against the reference's own loop on the pictures of one to six macroblocks and the flat, saturated
and full-range contents of tests/edge_cases.py -- the payload bytes of every frame and every decision array and filtered plane.  This is
the first hop of tests/test_gpu_edge_chains.py (kernel == twin there, twin == reference here).  Where oracle/_ref/libx264ref.so is built
the comparison is live; elsewhere the reference's side is the md5s of tests/golden/edge_chains.npz (oracle/gen_golden_edge.py).  The
coverage conditions of the case list are asserted on the twin's output, so that a change of seeds or options cannot quietly lose one."""
import numpy as np
import pytest

import edge_cases as E

CODED_BY_TWIN = E.TWIN + E.PLAIN + [n for n in E.REF if not E.CONFIGS[n][1]["cabac"]]       # (a CAVLC chain: the twin's decisions, no payload)


@pytest.mark.parametrize("name", CODED_BY_TWIN)
@pytest.mark.parametrize("size", E.SIZES, ids=E.size_id)
def test_twin_equals_reference_on_tiny_pictures(oracle_lib, size, name):
    src, kw, ekw, frames = E.CONFIGS[name]
    writer = src == "twin"
    for kind in E.CONTENTS:
        what = "%s %dx%d %s" % (name, size[0], size[1], kind)
        a = E.twin_chain(name, size, kind)
        if E.have_reference():
            b = E.reference_chain(name, size, kind)
            if writer:
                bad = [f for f in range(frames) if E.payload(a, f) != E.payload(b, f)]
                assert not bad, "%s: payload of frames %s differs between the twin and the reference" % (what, bad)
            for k in E.DECISIONS + E.PLANES:
                assert np.array_equal(a[k], b[k]), "%s: %s differs first at %s" % (what, k, np.argwhere(a[k] != b[k])[:3].tolist())
        else:
            pay, mbt, whole = E.recorded(name, size, kind)
            got_pay, got_mbt, got_whole = E.digests(a, name)
            if writer:
                bad = [f for f in range(frames) if bytes(got_pay[f]) != bytes(pay[f])]
                assert not bad, "%s: payload of frames %s differs between the twin and the reference" % (what, bad)
            bad = [f for f in range(frames) if bytes(got_mbt[f]) != bytes(mbt[f])]
            assert not bad, "%s: mb_type of frames %s differs between the twin and the reference" % (what, bad)
            for i, k in enumerate(E.WHOLE):
                assert bytes(got_whole[i]) == whole[k], "%s: %s differs between the twin and the reference" % (what, k)


TABLE_LOSSY = E.TABLE_LOSSY


def table_chains_equal_reference(size, name, low):
    frames = E.CONFIGS[name][3]
    for kind, qp in zip(E.CONTENTS, E.table_qps(name, low)):
        what = "%s %dx%d %s at QP %d" % (name, size[0], size[1], kind, qp)
        a = E.twin_chain(name, size, kind, qp)
        if E.have_reference():
            b = E.reference_chain(name, size, kind, qp)
            bad = [f for f in range(frames) if E.payload(a, f) != E.payload(b, f)]
            assert not bad, "%s: payload of frames %s differs between the twin and the reference" % (what, bad)
            for k in E.DECISIONS + E.PLANES:
                assert np.array_equal(a[k], b[k]), "%s: %s" % (what, k)
        else:
            pay, mbt, whole = E.recorded(name, size, kind, table="low" if low else True)
            got_pay, got_mbt, got_whole = E.digests(a, name)
            assert np.array_equal(got_pay, pay), "%s: payloads differ between the twin and the reference" % what
            assert np.array_equal(got_mbt, mbt), "%s: mb_type differs between the twin and the reference" % what
            for i, k in enumerate(E.WHOLE):
                assert bytes(got_whole[i]) == whole[k], "%s: %s differs between the twin and the reference" % (what, k)


@pytest.mark.parametrize("name", TABLE_LOSSY)
@pytest.mark.parametrize("size", E.TABLE_SIZES, ids=E.size_id)
def test_twin_equals_reference_at_the_chain_table_qps(oracle_lib, size, name):
    """tests/test_gpu_edge_table.py expects the twin run at each chain's own QP (8, 26, 51): the twin is the reference there too."""
    table_chains_equal_reference(size, name, False)


@pytest.mark.parametrize("name", TABLE_LOSSY)
@pytest.mark.parametrize("size", E.TABLE_SIZES, ids=E.size_id)
def test_twin_equals_reference_at_the_low_chain_table_qps(oracle_lib, size, name):
    """... and at the second assignment, QP 1, 2 and 3 side by side."""
    table_chains_equal_reference(size, name, True)


def test_low_qp_configurations_reach_the_escapes_qp0_and_ipcm(oracle_lib):
    """What the LOW_QP configurations are there for (edge_cases.low_qp_problems), on the twin's arrays; and the largest |level| of every
    chain is the one recorded from the reference (a CAVLC chain with the 8x8 transform: at least that, the reference's harness records such
    levels incompletely)."""
    chains = []
    for name in E.LOW_QP:
        for size in E.SIZES:
            for kind in E.CONTENTS:
                a = E.twin_chain(name, size, kind)
                chains.append((name, size, kind, a["mb_type"], a["qp"], E.max_level(a)))
                want, kw = E.recorded_max_level(name, size, kind), E.CONFIGS[name][1]
                lower_bound = not kw.get("cabac") and kw.get("transform8x8")
                assert chains[-1][5] >= want if lower_bound else chains[-1][5] == want, "%s %dx%d %s: largest |level| %d, the reference's %d" % (
                    (name,) + size + (kind, chains[-1][5], want))
    bad = E.low_qp_problems(chains)
    assert not bad, "the low-QP configurations lost what they are there for:\n  " + "\n  ".join(bad)


def test_case_list_reaches_every_macroblock_type_and_kernel_kind(oracle_lib):
    chains = [(name, size, kind, E.twin_chain(name, size, kind)["mb_type"]) for name in CODED_BY_TWIN for size in E.SIZES for kind in E.CONTENTS]
    bad = E.coverage_problems(chains)
    assert not bad, "the case list lost coverage:\n  " + "\n  ".join(bad)
    assert E.kinds_selected() == set(range(7)), "the configurations no longer select every kernel kind of the sweep: %s" % sorted(E.kinds_selected())


def test_contents_are_what_the_case_list_says():
    """Fixed seeds (not Python's hash), the extremes really are extreme, chroma derived from luma."""
    for size in E.SIZES:
        for kind in E.CONTENTS:
            y, u, v = E.content(kind, size[0], size[1], 3)
            y2, _, _ = E.content(kind, size[0], size[1], 3)
            assert np.array_equal(y, y2) and y.shape == (3, size[1], size[0]) and u.shape == v.shape == (3, size[1] // 2, size[0] // 2)
            assert np.array_equal(u, y[:, ::2, ::2]) and np.array_equal(v, 255 - y[:, 1::2, 1::2])
            if kind in ("checker", "flip", "vstripe", "satnoise"):
                assert set(np.unique(y).tolist()) == {0, 255}, kind
    assert len({E.seed_of(k, w, h) for k in E.CONTENTS for w, h in E.SIZES}) == len(E.CONTENTS) * len(E.SIZES)
