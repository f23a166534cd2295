"""Without a GPU: the macroblock-parallel form of the CAVLC writer (x264_vs2008_amd/csrc/cavlc_dev.h: cv_total, cv_mb in its counting and its
placing mode, cv_skip_run, cv_slice_end, cv_slot_too_small -- the text the kernels k_cavlc_mp_* of frame_cavlc.hip inline) compiled for the host by
tests/cavlc_mp_host_util.py.  tests/cavlc_mp_host.cpp runs count, scan and place for one slice, visiting the macroblocks in REVERSE raster
order in the count and in the place phase, so that any value the text still carried from macroblock to macroblock would show; payload,
payload_len and mb_bits must be cv_write_slice's on the same arrays, the bytes the REFERENCE's, and no byte outside the slice may change
(every buffer starts filled with a pattern: the pass relies on nothing the caller zeroed).  The cases are those of tests/test_cavlc_host.py."""
import os
import subprocess

import numpy as np
import pytest

import cavlc_b_util as B
import cavlc_synth as S
import edge_cases as E
from cavlc_host_util import MB_BYTES_MAX, restore_8x8_levels
from cavlc_mp_host_util import check_equal, sanitized_program, write_slice_both, write_state_both
from cavlc_reader import read_i16_slice
from cavlc_util import CONFIGS, QP1_CONFIGS, QP1_SIZES, reference
from oracle import refslice as rs
from paths import GOLDEN, REF_SO
from x264_vs2008_amd.slice import PAYLOAD_LEAD

needs_reference = pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libx264ref.so not built (needs /root/reference)")
FILL = 0x5A


def check_frames(name, a, p, want):
    for f, w in enumerate(want):
        got = write_slice_both(a, f, p, name, FILL)
        assert got == w, "%s frame %d: the slice differs from the reference's (%d vs %d bytes)" % (name, f, len(got), len(w))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_count_scan_place_equals_serial_and_reference_fixture(oracle_lib, name):
    c = CONFIGS[name]
    gold = np.load(os.path.join(GOLDEN, "cavlc_%s.npz" % name))
    p = rs.make_params(c["w"], c["h"], c["n"], **c["kw"])
    a = rs.run2(oracle_lib, "x264o_encode_chain2", p, rs.make_ext(write=0, **c.get("ext", {})), *rs.clip(c["w"], c["h"], c["n"], 0))
    check_frames(name, a, p, [bytes(gold["payload"][f, :gold["payload_len"][f]]) for f in range(c["n"])])


@needs_reference
@pytest.mark.parametrize("name", sorted(B.B_CASES))
def test_count_scan_place_equals_serial_and_reference_b_slices(oracle_lib, name):
    size, frames, _, kw, ekw = B.B_CASES[name]
    p = rs.make_params(size[0], size[1], frames, **kw)
    clip, a = B.reference(name)
    assert (a["frame_info"][:, 0] == rs.SLICE_B).any()
    a = restore_8x8_levels(a, rs.run2(oracle_lib, "x264o_encode_chain2", p, rs.make_ext(write=0, **ekw), *clip))
    check_frames(name, a, p, [bytes(a["payload"][f, :a["payload_len"][f]]) for f in range(frames)])


@pytest.mark.parametrize("name", QP1_CONFIGS)
@pytest.mark.parametrize("size", QP1_SIZES, ids=E.size_id)
def test_count_scan_place_equals_serial_and_reference_at_qp1(oracle_lib, size, name):
    """Long bit strings in neighbouring macroblocks: the tiny-picture chains of tests/edge_cases.py at QP 1, the bytes' md5 from the
    reference's record in tests/golden/edge_chains.npz."""
    frames = E.CONFIGS[name][3]
    for kind in E.CONTENTS:
        a = E.twin_chain(name, size, kind)
        want = E.recorded(name, size, kind)[0]
        for f in range(frames):
            got = write_slice_both(a, f, E.params(name, size), "%s %dx%d %s" % ((name,) + size + (kind,)), FILL)
            assert E.md5(np.frombuffer(got, np.uint8)) == bytes(want[f]), "%s %dx%d %s frame %d: the slice (%d bytes) differs from the reference's" % (
                (name,) + size + (kind, f, len(got)))


# ---- hand-built worst-case macroblocks (tests/cavlc_synth.py): more than 15,000 bits in one macroblock, next to its like ---------------------

def synth_both(kind, levels, high, **kw):
    return write_state_both(S.state(kind, levels), S.MB_W, S.MB_H, **{**S.params(kind, high), "cap": PAYLOAD_LEAD + (S.N + 1) * MB_BYTES_MAX, "fill": FILL, **kw})


@pytest.mark.parametrize("high", (1, 0), ids=("high", "baseline"))
@pytest.mark.parametrize("levels", ("min", "alt"))
@pytest.mark.parametrize("kind", sorted(S.KINDS))
def test_worst_case_macroblocks_are_placed_like_the_serial_writer_writes_them(kind, levels, high):
    serial, mp = synth_both(kind, levels, high)
    assert serial[0] == 0
    check_equal("%s %s" % (kind, levels), serial, mp, FILL)
    sizes = S.mb_sizes(mp[3])
    if high:
        assert sizes.max() >= S.HIGH_MB_BITS_MIN, "the case has lost its point: a largest macroblock of %d bits" % sizes.max()


@pytest.mark.parametrize("levels", ("rand", "min", "alt"))
def test_placed_slices_read_back(levels):
    """The independent reader (tests/cavlc_reader.py) on the placed bytes: the levels come back, and the positions are mb_bits."""
    st = S.state("i16", levels)
    serial, mp = synth_both("i16", levels, 1)
    check_equal("i16 %s" % levels, serial, mp, FILL)
    _, payload, plen, bits = mp
    got, pos = read_i16_slice(bytes(payload[0, PAYLOAD_LEAD:PAYLOAD_LEAD + plen]), S.MB_W, S.MB_H, S.SLICE_QP)
    for k in ("i16mode", "chroma_mode", "qp", "cbp", "luma", "luma_dc", "chroma_dc", "chroma_ac"):
        assert np.array_equal(got[k], st[k]), "%s read back differs first at %s" % (k, np.argwhere(got[k] != st[k])[:3].tolist())
    assert np.array_equal(pos, bits)


# ---- the slot: full, and too small ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ("i16", "p8"))
def test_full_slot_stops_both_writers_alike(kind):
    """tests/test_cavlc_host.py's full slot -- two slots, a payload_cap with which the fourth macroblock begins 1040 bytes before the slot's end,
    a macroblock's worst case kept free: cv_write_slice stops there, and so does the scan, by a comparison on the offsets.  The stopped pass has
    placed nothing at all."""
    _, mp = synth_both(kind, "min", 1)
    cap = S.full_slot_cap(mp[3])
    serial, mp = synth_both(kind, "min", 1, cap=cap, slots=2)
    assert serial[0] == 1 and serial[2] == 0
    check_equal(kind, serial, mp, FILL)


@pytest.mark.parametrize("kind", ("i16", "p8"))
@pytest.mark.parametrize("spare", (0, 1, 2, 7, 8))
def test_the_stop_decision_is_the_serial_writers_at_every_slot_size_around_the_boundary(kind, spare):
    """Slots from the smallest that holds the slice under the space check upwards and downwards by single bytes: the check compares the byte the
    last macroblock STARTS in with payload_cap - lead - margin, so the decision flips between two neighbouring sizes; both sides of the flip."""
    _, mp = synth_both(kind, "min", 1)
    start_last = int(mp[3][-2]) >> 3                               # the byte the last macroblock starts in
    flip = start_last + PAYLOAD_LEAD + MB_BYTES_MAX                # the smallest payload_cap that passes the check
    seen = set()
    for cap in (flip - 1 - spare, flip + spare):
        serial, mp2 = synth_both(kind, "min", 1, cap=cap, slots=2)
        check_equal("%s cap %d" % (kind, cap), serial, mp2, FILL)
        seen.add(serial[0])
    assert seen == {0, 1}, "the slot sizes no longer straddle the boundary"


def test_smallest_slot_of_the_entry_points_is_too_small_for_a_noisy_slice():
    """X264HIP_PAYLOAD_LEAD + 2624 + 128 bytes for six worst-case macroblocks: stopped, length 0, by both."""
    serial, mp = synth_both("i4", "alt", 1, cap=PAYLOAD_LEAD + MB_BYTES_MAX + 128, slots=2)
    assert serial[0] == 1
    check_equal("i4", serial, mp, FILL)


# ---- the same source as a program under the sanitizers -------------------------------------------------------------------------------------------

def test_program_under_address_and_undefined_behaviour_sanitizers():
    """tests/cavlc_mp_host.cpp with its own main: made-up I and P slices (skip runs at both ends of the slice, a slice of skips only), a slot whose
    end is the buffer's and no multiple of 4, both writers compared; the sanitizers watch every byte the placing sink touches."""
    r = subprocess.run([sanitized_program()], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "DIFFERENT" not in r.stdout and r.stdout.count("equal") == 41
