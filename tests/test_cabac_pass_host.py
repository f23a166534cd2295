"""Without a GPU: the product's CABAC pass (x264_vs2008_amd/csrc/cabac_pass_dev.h over mb_vocab.h, mbsyn.h and cabac_dev.h, the text
frame_cabac.hip's kernel inlines) compiled for the host by tests/cabac_pass_host_util.py and run on one frame's state arrays at a time; the
slice's bytes and the bit position after every macroblock must be the REFERENCE's.

  * fixtures: the cases of tests/cabac_pass_cases.py; the state arrays come from the CPU twin (oracle/liboracle.so: x264o_encode_chain2
    with write = 0, which runs no writer), bytes and positions from tests/golden/cabac_pass_*.npz (the reference's loop with its writer);
  * live, where oracle/_ref/libx264ref.so is built: the same cases on other clips, arrays and bytes both from the reference's own loop.

Conventions: nothing is converted.  Both harnesses record a macroblock's QP as x264_macroblock_cache_save leaves it (a skipped macroblock
and one without coefficients carry the QP before them).  The reference's arrays, read behind its writer, also carry
x264_cabac_mb_qp_delta's side effect (an I_16x16 without any coefficient takes the previous QP); the twin without a writer keeps that
macroblock's own QP.  The pass applies the rule itself, so both code the same bits wherever the decisions agree: on every case but one (the
live test compares them).  The one is aq_empty_i16, made so that empty I_16x16 macroblocks follow macroblocks of another QP: there the loop
without a writer decides differently from the next macroblock on, so that case's arrays come from the twin with its writer (what a sweep
without a writer leaves, since it applies the side effect itself), and test_pass_applies_the_writers_qp_side_effect_itself hands the pass
the same arrays with those macroblocks' QPs replaced by other values."""
import os

import numpy as np
import pytest

import cabac_pass_cases as cc
from cabac_pass_host_util import write_slice
from paths import REF_SO

needs_reference = pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libx264ref.so not built (needs the reference's sources)")


def check_frames(name, a, want, c):
    p = cc.params_of(c)
    for f in range(c["n"]):
        got, bits = write_slice(dict(a, frame_info=want["frame_info"]), f, p)
        w = bytes(want["payload"][f, :want["payload_len"][f]])
        assert got == w, "%s frame %d: the host pass's slice differs (%d vs %d bytes)" % (name, f, len(got), len(w))
        bad = np.flatnonzero(bits != want["mb_bits"][f])
        assert not len(bad), "%s frame %d: the position after macroblock %d differs (%d vs %d)" % (name, f, bad[0], bits[bad[0]], want["mb_bits"][f][bad[0]])


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_host_pass_equals_reference_fixture(oracle_lib, name):
    c = cc.CASES[name]
    check_frames(name, cc.twin_arrays(oracle_lib, c), cc.fixture(name), c)


@needs_reference
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_host_pass_equals_reference_live(oracle_lib, name):
    c = cc.CASES[name]
    a = cc.reference(c, live=True)
    check_frames(name, a, a, c)
    twin = cc.twin_arrays(oracle_lib, c, live=True)
    if c.get("twin_write"):
        assert np.array_equal(twin["qp"], a["qp"]), "%s: the twin's qp differs from the reference's" % name
    for k in ("mb_type", "partition", "sub_partition", "ref", "mv", "cbp", "t8", "luma"):
        assert np.array_equal(twin[k], a[k]), "%s: the twin's %s differs from the reference's" % (name, k)


def test_pass_applies_the_writers_qp_side_effect_itself(oracle_lib):
    """A state that does not carry x264_cabac_mb_qp_delta's side effect codes the same bits: every I_16x16 macroblock without coefficients of
    aq_empty_i16 gets another QP than the one before it (the reference's arrays hold the previous one there), the bytes stay the reference's."""
    c = cc.CASES["aq_empty_i16"]
    a = cc.twin_arrays(oracle_lib, c)
    empty = cc.empty_i16(a)
    assert empty.sum() >= 8 and empty[0].any() and empty[1:].any()
    check_frames("aq_empty_i16", dict(a, qp=np.where(empty, (a["qp"] + 7) % 52, a["qp"]).astype(np.int8)), cc.fixture("aq_empty_i16"), c)


def test_mb_bytes_max_is_stated_alike():
    """The worst case of one macroblock, before which the in-loop writer and the pass stop: slice_kernel.h, cabac_pass_dev.h (frame_cabac.hip
    asserts these two equal when it compiles) and slice.py."""
    import re
    from paths import ROOT
    from x264_vs2008_amd import slice as sl
    csrc = os.path.join(ROOT, "x264_vs2008_amd", "csrc")
    sw = int(re.search(r"#define SW_MB_BYTES_MAX (\d+)", open(os.path.join(csrc, "slice_kernel.h")).read()).group(1))
    cp = int(re.search(r"#define CP_MB_BYTES_MAX (\d+)", open(os.path.join(csrc, "cabac_pass_dev.h")).read()).group(1))
    assert sw == cp == sl.MB_BYTES_MAX
    assert "static_assert(CP_MB_BYTES_MAX == SW_MB_BYTES_MAX" in open(os.path.join(csrc, "frame_cabac.hip")).read()


def test_cases_reach_every_branch(oracle_lib):
    """The branches of the I / P syntax the cases must reach together, counted over the twin's arrays: every intra type (I_16x16 with and
    without AC), the three P_L0 shapes, P_8x8 with each sub-type, P_SKIP, a reference index above 0, an inter macroblock with the 8x8 transform,
    chroma cbp 0 / 1 / 2, a non-zero mb_qp_delta, under adaptive quantisation an I_16x16 or inter macroblock without coefficients right
    behind a QP change, an I_16x16 without coefficients whose own QP (which the twin, running no writer, keeps) is not the QP before it -- the
    macroblock x264_cabac_mb_qp_delta's side effect changes --, a coded macroblock on each picture edge."""
    total = {}
    for name, c in cc.CASES.items():
        for k, v in cc.coverage(cc.twin_arrays(oracle_lib, c, write=0), c).items():
            total[k] = total.get(k, 0) + v
    assert len(total) == 24 and all(v > 0 for v in total.values()), "syntax branches the cases never reach: %s" % [k for k, v in total.items() if not v]
    assert sum("aq_mode" in c.get("ext", {}) for c in cc.CASES.values()) == 3


def test_qp1_cases_reach_the_exp_golomb_tail(oracle_lib):
    """The QP 1 cases are there for levels beyond 2900 in a slice that is lossy at QP 0 (an I slice of a QP 1 chain): each size has them."""
    for size in cc.QP1_SIZES:
        top, qp0 = 0, False
        for kind in cc.QP1_KINDS:
            a = cc.twin_arrays(oracle_lib, cc.CASES["qp1_%dx%d_%s" % (size + (kind,))])
            top = max(top, max(int(np.abs(a[k].astype(np.int32)).max()) for k in ("luma", "luma_dc", "chroma_dc", "chroma_ac")))
            qp0 |= bool((a["frame_info"][:, 1] == 0).any())
        assert top >= cc.QP1_LEVEL and qp0, "%dx%d: largest |level| %d, a slice at QP 0: %s" % (size + (top, qp0))
