"""Without a GPU: the product's CAVLC writer (x264_vs2008_amd/csrc/cavlc_dev.h over mb_vocab.h, the text the kernels of frame_cavlc.hip
inline) compiled for the host by tests/cavlc_host_util.py and run on one frame's state arrays at a time; the slice's bytes must be the
REFERENCE's.

  * fixtures: the I / P configurations of tests/cavlc_util.py on the fixtures' clips; the state arrays come from the CPU twin
    (oracle/liboracle.so: x264o_encode_chain2 with cabac = 0, which runs no writer), the bytes from tests/golden/cavlc_*.npz;
  * live, where oracle/_ref/libx264ref.so is built: the same configurations on other clips and every B case of tests/cavlc_b_util.py,
    arrays and bytes both from the reference's own loop (oracle/ref_slice.c).

Conventions: one field is converted, luma of 8x8-transform macroblocks, which the reference's harness records incompletely under CAVLC
(cavlc_host_util.restore_8x8_levels names the rule; the missing levels come from the CPU twin's run of the same case, whose decisions are
the reference's).  The other candidates were checked and need nothing -- the QP of skipped macroblocks and of an I_16x16 without
coefficients, ref / mv of a list a B block does not use: both harnesses record them as a sweep leaves them in the x264hip_mb_state, read
after x264_macroblock_cache_save (a macroblock without coefficients carries the QP before it, an unused list reference -1 and vector 0)
and after cavlc_qp_delta's side effect on an empty I_16x16.  Every frame of every case is compared."""
import os

import numpy as np
import pytest

import cavlc_b_util as B
from cavlc_host_util import restore_8x8_levels, write_slice
from cavlc_util import CONFIGS, reference
from oracle import refslice as rs
from paths import GOLDEN, REF_SO

needs_reference = pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libx264ref.so not built (needs /root/reference)")


def check_frames(name, a, p, want):
    for f, w in enumerate(want):
        got = write_slice(a, f, p)
        assert got == w, "%s frame %d: the host writer's slice differs (%d vs %d bytes)" % (name, f, len(got), len(w))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_host_writer_equals_reference_fixture(oracle_lib, name):
    c = CONFIGS[name]
    gold = np.load(os.path.join(GOLDEN, "cavlc_%s.npz" % name))
    p = rs.make_params(c["w"], c["h"], c["n"], **c["kw"])
    a = rs.run2(oracle_lib, "x264o_encode_chain2", p, rs.make_ext(write=0, **c.get("ext", {})), *rs.clip(c["w"], c["h"], c["n"], 0))
    check_frames(name, a, p, [bytes(gold["payload"][f, :gold["payload_len"][f]]) for f in range(c["n"])])


def twin_arrays(oracle_lib, p, ext, clip):
    return rs.run2(oracle_lib, "x264o_encode_chain2", p, rs.make_ext(write=0, **ext), *clip)


@needs_reference
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_host_writer_equals_reference_live(oracle_lib, name):
    c = CONFIGS[name]
    p = rs.make_params(c["w"], c["h"], c["n"], **c["kw"])
    clip, want, a = reference(c, t0=37)
    a = restore_8x8_levels(a, twin_arrays(oracle_lib, p, c.get("ext", {}), clip))
    check_frames(name, a, p, want)


@needs_reference
@pytest.mark.parametrize("name", sorted(B.B_CASES))
def test_host_writer_equals_reference_b_slices(oracle_lib, name):
    size, frames, _, kw, ekw = B.B_CASES[name]
    p = rs.make_params(size[0], size[1], frames, **kw)
    clip, a = B.reference(name)
    assert (a["frame_info"][:, 0] == rs.SLICE_B).any()
    a = restore_8x8_levels(a, twin_arrays(oracle_lib, p, ekw, clip))
    check_frames(name, a, p, [bytes(a["payload"][f, :a["payload_len"][f]]) for f in range(frames)])


@needs_reference
def test_b_cases_reach_every_branch_of_the_b_syntax():
    total = {}
    for name in B.B_CASES:
        for k, v in B.coverage(B.reference(name)[1]).items():
            total[k] = total.get(k, 0) + v
    assert len(total) == 10 and all(v > 0 for v in total.values()), "B-slice syntax branches the cases never reach: %s" % [k for k, v in total.items() if not v]
