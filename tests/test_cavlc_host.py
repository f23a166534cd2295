"""Without a GPU: the product's CAVLC writer (x264_vs2008_amd/csrc/cavlc_dev.h over mb_vocab.h, the text the kernels of frame_cavlc.hip
inline) compiled for the host by tests/cavlc_host_util.py and run on one frame's state arrays at a time; the slice's bytes must be the
REFERENCE's.

  * fixtures: the I / P configurations of tests/cavlc_util.py on the fixtures' clips; the state arrays come from the CPU twin
    (oracle/liboracle.so: x264o_encode_chain2 with cabac = 0, which runs no writer), the bytes from tests/golden/cavlc_*.npz;
  * live, where oracle/_ref/libx264ref.so is built: the same configurations on other clips and every B case of tests/cavlc_b_util.py,
    arrays and bytes both from the reference's own loop (oracle/ref_slice.c);
  * lossy QP 1: tests/edge_cases.py's cavlc_qp1_high / cavlc_qp1_base chains, whose level codes pass 4095 (High profile's growing prefix, the
    Baseline clamp), against the reference's recorded digests;
  * hand-built worst-case macroblocks (tests/cavlc_synth.py), which no quantiser produces: the per-macroblock bound CV_MB_BYTES_MAX
    measured, the bytes read back by an independent reader (tests/cavlc_reader.py), and a full payload slot.

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
import cavlc_synth as S
import edge_cases as E
from cavlc_host_util import MB_BYTES_MAX, restore_8x8_levels, write_slice, write_state
from cavlc_reader import read_i16_slice
from cavlc_util import CONFIGS, QP1_CONFIGS, QP1_SIZES, reference
from oracle import refslice as rs
from paths import GOLDEN, REF_SO, ROOT
from x264_vs2008_amd.slice import PAYLOAD_LEAD

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


# ---- lossy QP 1: level codes in the extended escape (edge_cases' cavlc_qp1_high: the growing prefix; cavlc_qp1_base: the Baseline clamp) --------

@pytest.mark.parametrize("name", QP1_CONFIGS)
@pytest.mark.parametrize("size", QP1_SIZES, ids=E.size_id)
def test_host_writer_equals_reference_at_qp1(oracle_lib, size, name):
    """The tiny-picture chains of tests/edge_cases.py at QP 1: state arrays from the CPU twin, the bytes' md5 from the reference's record in
    tests/golden/edge_chains.npz -- so a GPU mismatch on these chains is the kernel's and not the shared text's."""
    frames, top = E.CONFIGS[name][3], 0
    for kind in E.CONTENTS:
        a = E.twin_chain(name, size, kind)
        top = max(top, E.max_level(a))
        want = E.recorded(name, size, kind)[0]
        for f in range(frames):
            got = write_slice(a, f, E.params(name, size))
            assert E.md5(np.frombuffer(got, np.uint8)) == bytes(want[f]), "%s %dx%d %s frame %d: the host writer's slice (%d bytes) differs from the reference's%s" % (
                (name,) + size + (kind, f, len(got), E.writer_branch(name, size, kind)))
    assert top >= E.CAVLC_ESCAPE_LEVEL, "no level code in the extended escape: largest |level| %d" % top


# ---- the per-macroblock bound, measured on what no quantiser produces ---------------------------------------------------------------------

def synth_slice(kind, levels, high, **kw):
    return write_state(S.state(kind, levels), S.MB_W, S.MB_H, **{**S.params(kind, high), "cap": PAYLOAD_LEAD + (S.N + 1) * MB_BYTES_MAX, **kw})


@pytest.mark.parametrize("high", (1, 0), ids=("high", "baseline"))
@pytest.mark.parametrize("levels", ("min", "alt"))
@pytest.mark.parametrize("kind", sorted(S.KINDS))
def test_worst_case_macroblocks_stay_within_the_derived_bound(kind, levels, high):
    """Every element at the longest code the derivation beside CV_MB_BYTES_MAX lists: the writer does not stop, no macroblock exceeds the
    bound, and in High profile the levels alone take 384 x 36 bits.  Measured (bits of the largest macroblock; High / Baseline):
    i16 14049 / 10977, i4 14091 / 11018, p8 15138 / 12066, b8 14615 / 11542 with -32768 throughout; with +-32767 in turn the same."""
    rc, _, plen, bits = synth_slice(kind, levels, high)
    sizes = S.mb_sizes(bits)
    print("%s %s %s: macroblocks of %s bits, slice %d bytes" % (kind, levels, "High" if high else "Baseline", sizes.tolist(), plen))
    assert rc == 0 and plen > 0, "the writer stopped"
    assert sizes.max() <= 8 * MB_BYTES_MAX, "a macroblock of %d bits: beyond CV_MB_BYTES_MAX" % sizes.max()
    if high:
        assert sizes.max() >= S.HIGH_MB_BITS_MIN
    assert (plen - 1) * 8 < bits[-1] + 1 <= plen * 8


def test_mb_bytes_max_is_stated_alike_for_cavlc():
    import re
    text = open(os.path.join(ROOT, "x264_vs2008_amd", "csrc", "frame_cavlc.hip")).read()
    assert int(re.search(r"#define CV_MB_BYTES_MAX (\d+)", text).group(1)) == MB_BYTES_MAX
    assert "CV_MARGIN_FRAME" not in text


def equal_states(got, want, keys):
    for k in keys:
        assert np.array_equal(got[k], want[k]), "%s read back differs first at %s" % (k, np.argwhere(got[k] != want[k])[:3].tolist())


READ_BACK = ("i16mode", "chroma_mode", "qp", "cbp", "luma", "luma_dc", "chroma_dc", "chroma_ac")


@pytest.mark.parametrize("high", (1, 0), ids=("high", "baseline"))
def test_reader_reads_back_levels_in_the_reference_pinned_range(high):
    """The reader itself, first: levels in -2000..2000 (a third zero, some +-1: every table and both trailing-one paths), the range in which the
    writer is held to the reference's bytes by the QP 1 chains."""
    st = S.state("i16", "rand")
    rc, payload, plen, bits = synth_slice("i16", "rand", high)
    assert rc == 0
    got, pos = read_i16_slice(bytes(payload[0, PAYLOAD_LEAD:PAYLOAD_LEAD + plen]), S.MB_W, S.MB_H, S.SLICE_QP)
    equal_states(got, st, READ_BACK)
    assert np.array_equal(pos, bits)


@pytest.mark.parametrize("levels", ("min", "alt"))
def test_high_profile_escape_round_trips_the_extreme_levels(levels):
    """-32768 and +-32767 through the growing prefix (prefix 19) and back.  Not covered, and known not to round trip: a remaining code of
    exactly 1 << (prefix - 3) -- 4096 at prefix 15, a first level of 2065 at suffix length 0 -- stays at that prefix (the loop's condition
    is `>`, as the reference's, R/encoder/cavlc.c:87) and is written as 0: it reads back as 17.  The writer keeps the reference's bytes."""
    st = S.state("i16", levels)
    rc, payload, plen, bits = synth_slice("i16", levels, 1)
    assert rc == 0
    got, pos = read_i16_slice(bytes(payload[0, PAYLOAD_LEAD:PAYLOAD_LEAD + plen]), S.MB_W, S.MB_H, S.SLICE_QP)
    equal_states(got, st, READ_BACK)
    assert np.array_equal(pos, bits)


def clamped(block):
    """What a decoder reads where the Baseline writer clamped: the levels of one block in scan order, all of them beyond the escape, coded from
    the last one down with suffixLength 1, 2, .. 6; each comes back with levelCode = (15 << suffixLength) + 4094 + (1 if negative), the first
    of them (no trailing ones before it) with 2 more."""
    out, coded = np.zeros_like(block), [i for i in range(len(block) - 1, -1, -1) if block[i]]
    assert len(coded) > 10
    for k, i in enumerate(coded):
        s = min(1 + k, 6)
        code = (15 << s) + 4094 + int(block[i] < 0) + 2 * (k == 0)
        out[i] = (code + 2) >> 1 if code % 2 == 0 else (-code - 1) >> 1
    return out


@pytest.mark.parametrize("levels", ("min", "alt"))
def test_baseline_clamp_reads_back_as_the_clamped_code(levels):
    """Below High profile the escape has no room beyond 4095: the writer codes 4094 + (code & 1), as the reference does after logging its
    overflow.  The round trip is lossy by design; what reads back is exactly that code."""
    st = S.state("i16", levels)
    rc, payload, plen, _ = synth_slice("i16", levels, 0)
    assert rc == 0
    got, _ = read_i16_slice(bytes(payload[0, PAYLOAD_LEAD:PAYLOAD_LEAD + plen]), S.MB_W, S.MB_H, S.SLICE_QP)
    equal_states(got, st, ("i16mode", "chroma_mode", "qp", "cbp"))
    for m in range(S.N):
        assert np.array_equal(got["luma_dc"][m], clamped(st["luma_dc"][m])), "macroblock %d: luma DC" % m
        for i in range(16):
            assert np.array_equal(got["luma"][m, 16 * i + 1:16 * i + 16], clamped(st["luma"][m, 16 * i + 1:16 * i + 16])), "macroblock %d: luma AC block %d" % (m, i)
        for i in range(8):
            assert np.array_equal(got["chroma_ac"][m, 16 * i + 1:16 * i + 16], clamped(st["chroma_ac"][m, 16 * i + 1:16 * i + 16])), "macroblock %d: chroma AC block %d" % (m, i)


# ---- a full slot: the writer checks for space at the start of a macroblock only, so the margin must be a macroblock's worst case ------------

def frame_margin():
    """The bytes x264hip_cavlc_write_frame keeps free behind the macroblock an I or P slice is about to write, as csrc/frame_cavlc.hip states
    them: CV_MB_BYTES_MAX unless the entry point sets a margin of its own."""
    import re
    text = open(os.path.join(ROOT, "x264_vs2008_amd", "csrc", "frame_cavlc.hip")).read()
    own = re.search(r"a\.margin = (\w+);", text)
    return int(re.search(r"#define %s (\d+)" % (own.group(1) if own else "CV_MB_BYTES_MAX"), text).group(1))


@pytest.mark.parametrize("kind", ("i16", "p8"))
def test_full_slot_stops_the_writer_and_leaves_the_next_slot_alone(kind):
    """Two slots, the second full of 0xA5, a payload_cap with which the fourth macroblock begins 1040 bytes before the slot's end.  With a
    macroblock's worst case kept free -- the margin of both entry points, for every slice type -- the writer stops there and the second slot
    stays as it was.  With the 1024 bytes x264hip_cavlc_write_frame once kept free for I and P slices it writes that macroblock, 700 and
    more bytes of it into the next slot: the space check runs at the start of a macroblock only, so nothing smaller than the worst case will do."""
    _, _, _, bits = synth_slice(kind, "min", 1)
    cap = S.full_slot_cap(bits)
    assert frame_margin() == MB_BYTES_MAX
    rc, payload, plen, _ = synth_slice(kind, "min", 1, cap=cap, slots=2, fill=0xA5, margin=frame_margin())
    assert (payload[1] == 0xA5).all(), "the writer wrote %d bytes behind its slot" % (np.flatnonzero(payload[1] != 0xA5).max() + 1)
    assert rc == 1 and plen == 0
    assert (payload[0, PAYLOAD_LEAD:] != 0xA5).any()
    _, payload, _, _ = synth_slice(kind, "min", 1, cap=cap, slots=2, fill=0xA5, margin=1024)
    assert np.flatnonzero(payload[1] != 0xA5).max() >= 700, "a margin of 1024 bytes no longer overruns: the case has lost its point"
