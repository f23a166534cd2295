"""GPU: the macroblock-parallel CAVLC pass (x264hip_cavlc_write_frame_mp / _chains_mp: count, scan, place -- every lane writes) against the
serial pass (one lane per slice) on the same encoder options: payload bytes, payload_len and mb_bits of every chain and frame are equal, and
where a fixture holds the REFERENCE's bytes they are those.  The pictures are the smallest at which the kernels can still go wrong:

  * tests/edge_cases.py's one- to six-macroblock pictures (a slice of one macroblock and the trailing bits, no row above, top-right off the
    picture), three chains, so chain offsets other than 0;
  * 272x64 = 17x4 = 68 macroblocks, one more wavefront step of the scan than 64: a skip run that crosses macroblock 64, and a slice that is
    a skip run and the trailing bits only;
  * 396 macroblocks, sub-8x8 vectors, per-macroblock QP (cavlc_util.CONFIGS against their fixtures), QP 1 (long bit strings side by side);
  * B slices in lock step, and I, P and B entries in one chain table (StreamEncoder);
  * the refusals, and a slot too small.
Every payload buffer holds the frame before when a pass writes it: nothing relies on zeroed memory."""
import ctypes as C
import os

import numpy as np
import pytest

import cavlc_b_util as B
import edge_cases as E
from cavlc_host_util import MB_BYTES_MAX
from cavlc_mp_util import P_SKIP, run_lockstep, run_stream, same_frames
from cavlc_util import CONFIGS, QP1_CONFIGS
from oracle import refslice as rs
from oracle.gen_golden_slice import case_inputs
from paths import GOLDEN, REF_SO
from x264_vs2008_amd import slice as sl
from x264_vs2008_amd.frame import DeviceArray, cqm_init
from x264_vs2008_amd.stream import StreamEncoder

pytestmark = pytest.mark.gpu
needs_reference = pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libx264ref.so not built (needs the reference tree)")

EDGE_KW = dict(qp=22, me_method=rs.ME_HEX, subme=2, n_refs=1, inter=0x11, intra=0x3, cabac=0, deblock=1)
EDGE_CONTENTS = ("noise", "satnoise", "flat0")


@pytest.mark.parametrize("size", E.SIZES, ids=E.size_id)
def test_edge_pictures_i_and_p_slices(hip_lib, size):
    """An I and two P slices of three chains (noise, saturated noise, flat) on pictures of 1x1 to 3x2 macroblocks."""
    cqm = cqm_init(hip_lib)
    clips = [E.clip(kind, size, 3) for kind in EDGE_CONTENTS]
    want = run_lockstep(hip_lib, cqm, size, clips, 3, EDGE_KW, False)
    got = run_lockstep(hip_lib, cqm, size, clips, 3, EDGE_KW, True)
    assert all(len(p) > 0 for fr in want for p in fr["payload"])
    same_frames(got, want, "%dx%d" % size)


# ---- the step of 64 macroblocks ------------------------------------------------------------------------------------------------------------------
# 272x64: 17x4 = 68 macroblocks.  Frame 0 is flat (an I slice), frame 1 repeats it (every macroblock P_SKIP: the slice is ue(68) and the
# trailing bits, two bytes), frame 2 repeats it but for noise in macroblocks 0 and 66 (a run of the 65 skipped macroblocks 1 .. 65 between two
# coded ones: it starts in the scan's first step of 64 and ends in its second).  QP 30, chosen on the serial path: flat content predicts
# exactly whatever the vectors around the two noisy macroblocks are, so the conditions do not hang on the QP; they are checked below on the
# state of BOTH runs, and the test fails if they ever stop holding.
STEP_SIZE, STEP_KW = (272, 64), dict(qp=30, me_method=rs.ME_HEX, subme=2, n_refs=1, inter=0x11, intra=0x3, cabac=0, deblock=1)


def step_clip():
    r = np.random.default_rng(64)
    y, u, v = np.full((3, 64, 272), 128, np.uint8), np.full((3, 32, 136), 128, np.uint8), np.full((3, 32, 136), 128, np.uint8)
    for mb in (0, 66):
        my, mx = divmod(mb, 17)
        y[2, 16 * my:16 * my + 16, 16 * mx:16 * mx + 16] = r.integers(0, 256, (16, 16))
        u[2, 8 * my:8 * my + 8, 8 * mx:8 * mx + 8] = r.integers(0, 256, (8, 8))
        v[2, 8 * my:8 * my + 8, 8 * mx:8 * mx + 8] = r.integers(0, 256, (8, 8))
    return y, u, v


def test_skip_runs_across_the_64_macroblock_step(hip_lib):
    cqm = cqm_init(hip_lib)
    want = run_lockstep(hip_lib, cqm, STEP_SIZE, [step_clip()], 3, STEP_KW, False)
    got = run_lockstep(hip_lib, cqm, STEP_SIZE, [step_clip()], 3, STEP_KW, True)
    for run in (want, got):
        t1, t2 = run[1]["mb_type"][0], run[2]["mb_type"][0]
        assert (t1 == P_SKIP).all(), "frame 1 holds coded macroblocks: %s" % np.flatnonzero(t1 != P_SKIP).tolist()
        assert (t2[1:66] == P_SKIP).all() and t2[0] != P_SKIP and t2[66] != P_SKIP, "frame 2: no run of skipped macroblocks 1 .. 65 between coded 0 and 66: %s" % t2.tolist()
    assert want[1]["payload"][0] == bytes([0b00000010, 0b00101100]), "ue(68) and the trailing bits: %s" % want[1]["payload"][0].hex()
    same_frames(got, want, "272x64")


# ---- the existing configurations against the reference's bytes -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("uf_cif", "p_all_partitions", "aq_strong_high_qp"))
def test_configurations_equal_serial_pass_and_reference_fixture(hip_lib, name):
    """396 macroblocks; sub-8x8 vectors, three references, the 8x8 transform; per-macroblock QP with mb_qp_delta."""
    c = CONFIGS[name]
    gold = np.load(os.path.join(GOLDEN, "cavlc_%s.npz" % name))
    kw, clip, cqm = dict(c["kw"], **c.get("ext", {})), rs.clip(c["w"], c["h"], c["n"], 0), cqm_init(hip_lib)
    want = run_lockstep(hip_lib, cqm, (c["w"], c["h"]), [clip], c["n"], kw, False)
    got = run_lockstep(hip_lib, cqm, (c["w"], c["h"]), [clip], c["n"], kw, True)
    same_frames(got, want, name)
    for f in range(c["n"]):
        assert got[f]["payload"][0] == bytes(gold["payload"][f, :gold["payload_len"][f]]), "%s frame %d: the payload differs from the reference's" % (name, f)


@pytest.mark.parametrize("name", QP1_CONFIGS)
def test_qp1_chains_equal_serial_pass_and_reference_record(hip_lib, cqm, name):
    """tests/edge_cases.py's chains at QP 1 on 40x24, nine contents side by side: macroblocks of thousands of bits next to each other, level
    codes in the extended escape (High profile's growing prefix, the Baseline clamp); the bytes' md5 from the reference's record."""
    size = (40, 24)
    _, kw, ekw, frames = E.CONFIGS[name]
    clips = [E.clip(kind, size, frames) for kind in E.CONTENTS]
    kw = dict(kw, **(ekw or {}))
    want = run_lockstep(hip_lib, cqm, size, clips, E.order_of(name), kw, False)
    got = run_lockstep(hip_lib, cqm, size, clips, E.order_of(name), kw, True)
    same_frames(got, want, name)
    for b, kind in enumerate(E.CONTENTS):
        md5s = E.recorded(name, size, kind)[0]
        for f in range(frames):
            assert E.md5(np.frombuffer(got[f]["payload"][b], np.uint8)) == bytes(md5s[f]), "%s %s frame %d: the payload differs from the reference's" % (name, kind, f)


# ---- B slices; I, P and B entries in one chain table ----------------------------------------------------------------------------------------------

B_NAME = "spatial_w_t8_ref3"
_b_chain = {}


def b_chain(hip_lib):
    """The B case's chain through both passes, (serial, macroblock-parallel, coding order): computed once, left unchanged.  The clip is the
    case's own (gen_golden_slice.case_inputs, what cavlc_b_util.reference feeds the reference): no reference library is needed for it."""
    if not _b_chain:
        size, frames, kind, kw, ekw = B.B_CASES[B_NAME]
        clip = case_inputs(size, frames, kind)
        order = sl.coding_order(frames, kw.get("keyint", 0), ekw["bframes"])
        kw, cqm = dict(kw, **ekw), cqm_init(hip_lib)
        _b_chain["runs"] = (run_lockstep(hip_lib, cqm, size, [clip], order, kw, False), run_lockstep(hip_lib, cqm, size, [clip], order, kw, True), order)
    return _b_chain["runs"]


def test_b_chain_equals_serial_pass(hip_lib):
    """A lock-step chain with B slices (spatial direct, weighted bi-prediction, 8x8 transform, three references): needs the clip only."""
    want, got, order = b_chain(hip_lib)
    assert sum(stype == sl.SLICE_B for _, stype in order) >= 3
    same_frames(got, want, B_NAME)


@needs_reference
def test_b_chain_equals_reference(hip_lib):
    name, frames = B_NAME, B.B_CASES[B_NAME][1]
    _, a = B.reference(name)
    _, got, _ = b_chain(hip_lib)
    assert (a["frame_info"][:, 0] == rs.SLICE_B).sum() >= 3
    for f in range(frames):
        assert got[f]["payload"][0] == bytes(a["payload"][f, :a["payload_len"][f]]), "%s coded frame %d: the payload differs from the reference's" % (name, f)
        assert np.array_equal(got[f]["mb_bits"][0], a["mb_bits"][f])


def test_stream_with_adaptive_b_frames_crf_and_a_scene_cut(hip_lib):
    """--no-cabac --crf 23 --bframes 3 --b-adapt 1 --direct auto on two chains whose clips differ: their frame types part, so steps hold I, P and
    B entries in one table of x264hip_cavlc_write_chains_mp."""
    c, cqm = B.STREAMS["crf_badapt1_direct_auto"], cqm_init(hip_lib)
    want, mixed = run_stream(hip_lib, cqm, c, (5, 31), False)
    got, _ = run_stream(hip_lib, cqm, c, (5, 31), True)
    types = {st for chain in want for _, st, _, _, _, _ in chain}
    assert types == {sl.SLICE_I, sl.SLICE_P, sl.SLICE_B} and mixed > 0, "slice types %s, %d steps with more than one type in the table" % (types, mixed)
    for b in range(2):
        assert len(got[b]) == len(want[b]) == c["frames"]
        for k, (g, w) in enumerate(zip(got[b], want[b])):
            what = "chain %d coded frame %d (input %d, %s)" % (b, k, w[0], "PBI"[w[1]])
            assert g[:3] == w[:3] and g[4] == w[4], "%s: frame, type, QP, payload_len %s, the serial pass %s" % (what, g[:3] + (g[4],), w[:3] + (w[4],))
            assert np.array_equal(g[5], w[5]), "%s: mb_bits" % what
            assert g[3] == w[3], "%s: payload bytes" % what


# ---- refusals, and a slot too small ---------------------------------------------------------------------------------------------------------------

def test_cavlc_mp_goes_with_the_cavlc_pass_only(hip_lib):
    cqm = cqm_init(hip_lib)
    for kw in (dict(cabac=1, write=1), dict(cabac=0, write=0), dict(cabac=0, write=1, subme=6)):
        with pytest.raises(ValueError, match="cavlc_mp"):
            sl.ChainEncoder(hip_lib, 32, 32, cqm, cavlc_mp=True, **kw)
    with pytest.raises(ValueError, match="cavlc_mp"):
        StreamEncoder(hip_lib, 32, 32, cqm, cabac=1, cavlc_mp=True)


def test_slot_too_small_and_refusals(hip_lib):
    """A noisy 40x24 picture at QP 4 (six macroblocks of several hundred bytes: the last one starts 2478 bytes into the slice) into a slot of
    X264HIP_PAYLOAD_LEAD + 2624 + 128 bytes through x264hip_cavlc_write_chains_mp, and into one of 4096 bytes -- the smallest that entry point
    takes, as the serial one -- through x264hip_cavlc_write_frame_mp: the call succeeds, x264hip_slice_sweep_status reports the abort,
    payload_len is 0, and neither the slot nor the neighbouring chain's slot, both filled with a pattern, has changed.  Then what the entry
    points refuse before any launch: the serial calls' messages."""
    lib, cqm = hip_lib, cqm_init(hip_lib)
    y, u, v = E.clip("noise", (40, 24), 1)
    caps = dict(frame=4096, chains=sl.PAYLOAD_LEAD + MB_BYTES_MAX + 128)
    cap = max(caps.values())
    enc = sl.ChainEncoder(lib, 40, 24, cqm, write=1, **dict(EDGE_KW, qp=4))
    bufs, tab_host = [], lib.x264hip_host_alloc(lib.x264hip_chain_cavlc_bytes())
    try:
        enc.upload(y[0], u[0], v[0])
        _, qp, state = enc.encode_frame()
        enc.status()
        roomy = len(enc.payloads()[0])
        start_last = int(enc.rd_bufs["mb_bits"].get()[0, -2]) >> 3
        assert start_last > cap - sl.PAYLOAD_LEAD - MB_BYTES_MAX, "the last macroblock starts at byte %d of %d: the case has lost its point" % (start_last, roomy)
        ctx = enc.ctx
        scratch = DeviceArray(lib, (lib.x264hip_cavlc_mp_scratch_bytes(ctx.h, 1),), np.uint8)
        tab_dev = DeviceArray(lib, (lib.x264hip_chain_cavlc_bytes(),), np.uint8)
        plen = DeviceArray(lib, (2,), np.int32)
        guard = DeviceArray(lib, (2, cap), np.uint8)
        bufs += [scratch, tab_dev, plen, guard]

        def params(**k):
            return sl.CavlcParams(**dict(dict(slice_type=sl.SLICE_I, n_ref0=0, analyse_inter=0x11, transform8x8=0, cqm_custom=0, payload=guard.ptr, payload_cap=cap,
                                              payload_len=plen.ptr, mb_bits=None, slice_qp=qp), **k))

        def launch(entry, st, cp, scratch_p=scratch.p, chain=0, tab=tab_host):
            if entry == "frame":
                return lib.x264hip_cavlc_write_frame_mp(ctx.h, C.byref(st), C.byref(cp), scratch_p)
            e = (sl.ChainCavlc * 1)(sl.ChainCavlc(chain=chain, state=C.addressof(st), params=C.addressof(cp)))
            return lib.x264hip_cavlc_write_chains_mp(ctx.h, e, 1, tab, tab_dev.p, scratch_p)

        for entry in ("frame", "chains"):
            guard.set(np.full((2, cap), 0xA5, np.uint8))
            plen.set(np.full(2, -1, np.int32))
            ctx.check(lib.x264hip_mb_state_clear_progress(ctx.h, C.byref(state.st)), "mb_state_clear_progress")
            assert launch(entry, state.st, params(payload_cap=caps[entry])) == 0, "%s: %s" % (entry, lib.x264hip_last_error().decode())
            status = lib.x264hip_slice_sweep_status(ctx.h, C.byref(state.st))
            assert status == -1 and "out of payload space" in lib.x264hip_last_error().decode(), entry
            assert int(plen.get()[0]) == 0, entry
            assert (guard.get() == 0xA5).all(), "%s: the stopped pass wrote into the slots" % entry
        ctx.check(lib.x264hip_mb_state_clear_progress(ctx.h, C.byref(state.st)), "mb_state_clear_progress")
        bare = sl.DeviceState(ctx, levels=False)
        no_l1 = sl.MbState.from_buffer_copy(state.st)
        no_l1.mv1 = None
        try:
            for entry in ("frame", "chains"):
                for st, k, word in ((state.st, dict(payload=None), "payload buffers"), (state.st, dict(payload_len=None), "payload buffers"),
                                    (bare.st, {}, "coefficient levels"), (no_l1, dict(slice_type=sl.SLICE_B), "list-1 arrays"), (state.st, dict(slice_type=3), "slice type"),
                                    (state.st, dict(payload_cap=4095 if entry == "frame" else sl.PAYLOAD_LEAD + MB_BYTES_MAX - 1),
                                     "payload_cap" if entry == "frame" else "smaller than one macroblock")):
                    assert launch(entry, st, params(**k)) == -1 and word in lib.x264hip_last_error().decode(), (entry, k, lib.x264hip_last_error().decode())
                assert launch(entry, state.st, params(), scratch_p=None) == -1 and "scratch" in lib.x264hip_last_error().decode()
            assert launch("chains", state.st, params(), chain=1) == -1 and "chain 1" in lib.x264hip_last_error().decode()
            assert launch("chains", state.st, params(), tab=None) == -1 and "missing" in lib.x264hip_last_error().decode()
        finally:
            bare.free()
        assert lib.x264hip_slice_sweep_status(ctx.h, C.byref(state.st)) == 0 and (guard.get() == 0xA5).all()
    finally:
        enc.sync()
        for d in bufs:
            d.free()
        lib.x264hip_host_free(tab_host)
        enc.close()
