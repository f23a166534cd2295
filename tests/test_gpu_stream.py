"""End to end: a batch of chains through the StreamEncoder -- the lookahead's cost kernel, the library's slice-type decision and rate
control, the chain-table sweep with every chain coding its own kind of frame at its own QP -- against the REFERENCE's encoder run on the
same clips (oracle/ref_slice.c refslice_encode_stream: x264_encoder_encode's queue around x264_slicetype_decide, x264_ratecontrol_start
and the slice loop).  Compared: the order frames are coded in, their types, QPs and the slice_data() bytes of every one.

  * golden: tests/golden/stream_*.npz made by oracle/gen_golden_stream.py from the reference;
  * live: the same configurations with other clips where oracle/_ref/libx264ref.so is built.

The configurations and the drivers (run_stream, check, ...) are in tests/stream_util.py."""
import os

import numpy as np
import pytest

import look_cases as K
from oracle import refslice as rs
from paths import REF_SO, ROOT
from stream_util import CONFIGS, SEEDS, STEP_ONLY, chains, check, mixed_config, random_config, run_async, run_stream

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pipeline", [False, True])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_stream_equals_reference_fixture(hip_lib, name, pipeline):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "stream_%s.npz" % name))
    cs = chains(name, SEEDS[name])
    got = run_stream(hip_lib, cs, pipeline)
    for i, c in enumerate(cs):
        a = {k: gold["c%d_%s" % (i, k)] for k in ("frame_info", "frame_info2", "payload", "payload_len")}
        check(got[i], a, c, "%s chain %d" % (name, i))
        for f in range(c["frames"]):                     # a B slice header's direct_spatial_mv_pred (--direct auto: it follows the running scores)
            if int(a["frame_info"][f][0]) == rs.SLICE_B:
                assert run_stream.direct_spatial[i][f] == int(a["frame_info2"][f][3]), "%s chain %d coded frame %d: direct mode" % (name, i, f)


@pytest.mark.parametrize("name", sorted(set(CONFIGS) - STEP_ONLY))
def test_async_stream_equals_reference_fixture(hip_lib, name):
    """Chains stepping on their own (AsyncStreamEncoder): each chain's frames, in its coding order, are the lock-step encoder's and the reference's."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "stream_%s.npz" % name))
    cs = chains(name, SEEDS[name])
    got, sizes = run_async(hip_lib, cs)
    for i, c in enumerate(cs):
        a = {k: gold["c%d_%s" % (i, k)] for k in ("frame_info", "frame_info2", "payload", "payload_len")}
        check(got[i], a, c, "%s chain %d (async)" % (name, i))
    assert sum(sizes) == len(cs) * cs[0]["frames"]


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libx264ref.so not built (needs /root/reference)")
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_stream_equals_reference_live(hip_lib, name):
    cs = chains(name, [s + 40 for s in SEEDS[name]])
    got = run_stream(hip_lib, cs)
    for i, c in enumerate(cs):
        check(got[i], K.reference_records(c), c, "%s chain %d" % (name, i))


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libx264ref.so not built (needs /root/reference)")
@pytest.mark.parametrize("seed", list(range(14)))
def test_stream_random_configuration_equals_reference(hip_lib, seed):
    """Seeded option sets (references, partitions, subme 2..8, trellis, psy-rd, AQ, weightb, spatial / temporal direct, b-adapt 0 / 1 / 2, CQP / CRF,
    scene cuts, keyint) through the StreamEncoder, two chains with different clips, against the reference's whole encoder."""
    c = random_config(seed)
    cs = []
    for k in range(2):
        ck = dict(c)
        ck.update(t0=c["t0"] + 61 * k, slow=[c["slow"], 1 + (c["slow"] % 3)][k])
        cs.append(ck)
    got = run_stream(hip_lib, cs, pipeline=bool(seed & 1))
    for i, ck in enumerate(cs):
        check(got[i], K.reference_records(ck), ck, "seed %d chain %d %s" % (seed, i, {k: ck[k] for k in ("subme", "n_refs", "bframes", "b_adapt", "crf", "trellis", "direct_pred", "aq", "inter")}))


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libx264ref.so not built (needs /root/reference)")
@pytest.mark.parametrize("seed", [11, 14, 19, 36, 37, 209, 226])
def test_stream_post_encode_scenecut_equals_reference(hip_lib, seed):
    """No --pre-scenecut (the reference's default): x264_encoder_encode looks at every coded P picture and, where an intra picture would have been as
    good, gives the attempt up and codes again -- the picture as I or IDR, or the B picture before it as the P, with the queues rearranged
    (R/encoder/encoder.c:1603-1699).  Clips with scene changes and repeated pictures, two chains per encoder so that one chain's second attempt
    runs while the other has nothing to do: frame order, types, QPs, payloads, and the frame_num each slice header carries (restarted only by a
    scene-cut IDR) against the reference's encoder."""
    from x264_vs2008_amd import mux
    c = dict(K.config(seed), pre_scenecut=0, subme=5, n_refs=2, inter=0x13)
    if c["scenecut_threshold"] < 0:
        c["scenecut_threshold"] = 40
    cs = [dict(c), dict(c, t0=c["t0"] + 61, cut=max(c["cut"] - 2, 0))]
    # odd seeds: the encoder knows the clip's length and runs the next call's lookahead AHEAD of the verdicts, beside the sweep, with a copy of the judged
    # chains' queues to come back to (x264hip_lookahead_save / _restore)
    got = run_stream(hip_lib, cs, pipeline=bool(seed & 1))
    resets, gave_up = run_stream.resets, 0
    for i, ck in enumerate(cs):
        a = K.reference_records(ck)
        check(got[i], a, ck, "seed %d chain %d" % (seed, i))
        gave_up += int(a["stat"][:ck["frames"], 3].sum())
        # the muxer's own frame_num bookkeeping against the reference's h->i_frame_num
        p = mux.encoder_params(hip_lib, width=ck["w"], height=ck["h"], rc_method=mux.RC_CQP, qp_constant=ck["qp"], bframe=ck["bframes"], keyint_max=ck["keyint"])
        m = mux.AnnexB(hip_lib, p)
        for f, (frame, st, qp, payload) in enumerate(got[i]):
            poc = int(a["frame_info"][f][3])
            ftype = (mux.TYPE_IDR if poc == 0 else mux.TYPE_I) if st == rs.SLICE_I else mux.TYPE_P if st == rs.SLICE_P else mux.TYPE_B
            m.frame(frame=frame, ftype=ftype, qp=qp, payload=payload, frame_num_reset=resets[i][f])
            used = m.frame_num - (0 if ftype == mux.TYPE_B else 1)
            assert used == int(a["look_cost"][f][7]), "seed %d chain %d coded frame %d: frame_num %d, the reference %d" % (seed, i, f, used, int(a["look_cost"][f][7]))
    assert gave_up > 0, "seed %d: no attempt was given up -- the clip does not test the scene cut" % seed


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libx264ref.so not built (needs /root/reference)")
@pytest.mark.parametrize("seed", [3, 13, 21, 26, 35, 203])
def test_stream_direct_auto_equals_reference(hip_lib, seed):
    """--direct auto: every B macroblock predicts BOTH direct modes (the other one first, then the frame's; R/encoder/analyse.c:2476-2496) and credits each
    with the skip it would give; the running scores pick every B frame's mode and decay as x264_encoder_frame_end lets them (encoder.c:113-118,
    1777-1790).  Clips with B frames (fixed pattern and b-adapt 1 / 2), below and with the RD levels, two chains with different content: order, types,
    QPs, payloads -- and the direct_spatial_mv_pred bit of every B slice header -- against the reference's encoder."""
    base = K.config(seed)
    c = dict(base, direct_pred=3, bframes=max(base["bframes"], 2), subme=[4, 6, 7, 5, 8, 7][seed % 6], n_refs=2, inter=0x113 if seed % 2 else 0x13, trellis=seed % 3 == 0)
    cs = [dict(c), dict(c, t0=c["t0"] + 61, slow=1 + (c["slow"] % 3))]
    got = run_stream(hip_lib, cs)
    n_b, modes = 0, set()
    for i, ck in enumerate(cs):
        a = K.reference_records(ck)
        check(got[i], a, ck, "seed %d chain %d" % (seed, i))
        for f in range(ck["frames"]):
            if int(a["frame_info"][f][0]) == rs.SLICE_B:
                n_b += 1
                modes.add(int(a["frame_info2"][f][3]))
                assert run_stream.direct_spatial[i][f] == int(a["frame_info2"][f][3]), "seed %d chain %d coded frame %d: direct mode" % (seed, i, f)
    assert n_b > 0


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libx264ref.so not built (needs /root/reference)")
@pytest.mark.parametrize("seed", [67, 68, 69, 91, 93, 99, 122, 139, 160, 203, 227, 238])
def test_stream_mixed_round3_options_equal_reference(hip_lib, seed):
    """Seeds of scratch/fuzz_stream_new.py (760 configurations equal) that combine --direct auto with given-up P pictures, with and without the lookahead
    running ahead of the verdicts: order, types, QPs, payloads and every B slice's direct mode against the reference's encoder."""
    cs, pipe = mixed_config(seed)
    got = run_stream(hip_lib, cs, pipeline=pipe)
    for i, ck in enumerate(cs):
        a = K.reference_records(ck)
        check(got[i], a, ck, "seed %d chain %d" % (seed, i))
        for f in range(ck["frames"]):
            if int(a["frame_info"][f][0]) == rs.SLICE_B:
                assert run_stream.direct_spatial[i][f] == int(a["frame_info2"][f][3]), "seed %d chain %d coded frame %d: direct mode" % (seed, i, f)
