"""GPU: lossless (--qp 0) through the frame queue and the command line -- the lookahead scoring with SAD (mbcmp when lossless), the scene cut
decided in the lookahead or after the encode (given-up P pictures coded again), every frame type at QP 0 -- against the REFERENCE's whole
encoder (oracle/ref_slice.c refslice_encode_stream at qp 0; fixtures tests/golden/ll_stream_*.npz and ll_cli.npz, made by
tests/lossless_cases.py; live where oracle/_ref/libx264ref.so is built).

Without the feature the stream and command-line tests fail with "lossless is not built in the raster variant" and the lookahead test with the
cost kernel's "only the SATD lookahead is built" (test_lossy_sad_lookahead_stays_refused pins what must NOT change and passes either way)."""
import hashlib
import os

import numpy as np
import pytest

import look_cases as K
import lossless_cases as LC
from conftest import GOLDEN
from mux_cases import write_clip
from paths import REF_SO
from stream_util import run_stream
from x264_vs2008_amd import encode as E
from x264_vs2008_amd import lookahead as LA
from x264_vs2008_amd import mux
from x264_vs2008_amd.frame import FrameCtx

pytestmark = pytest.mark.gpu


def check(got, a, c, what):
    """stream_util.check with the payloads held by their md5."""
    frames = c["frames"]
    assert len(got) == frames, "%s: %d frames coded, the reference codes %d" % (what, len(got), frames)
    for f, (frame, st, qp, payload) in enumerate(got):
        ref = (int(a["frame_info2"][f][0]), int(a["frame_info"][f][0]), int(a["frame_info"][f][1]))
        assert (frame, st, qp) == ref, "%s coded frame %d: (input, slice, qp) %s, the reference %s" % (what, f, (frame, st, qp), ref)
        assert qp == 0
        assert len(payload) == int(a["payload_len"][f]) and hashlib.md5(payload).hexdigest() == str(a["payload_md5"][f]), \
            "%s coded frame %d (input %d, slice %d): payload differs (%d bytes, the reference %d)" % (what, f, frame, st, len(payload), int(a["payload_len"][f]))


@pytest.mark.parametrize("pipeline", [False, True])
@pytest.mark.parametrize("name", sorted(LC.LL_STREAMS))
def test_lossless_stream_equals_reference_fixture(hip_lib, name, pipeline):
    """Two chains with different clips, each with a real cut: frame order, types, QPs and payload bytes."""
    gold = np.load(os.path.join(GOLDEN, "ll_stream_%s.npz" % name))
    cs = LC.LL_STREAMS[name]
    got = run_stream(hip_lib, cs, pipeline)
    gave_up, intra_mid = 0, 0
    for i, c in enumerate(cs):
        a = {k: gold["c%d_%s" % (i, k)] for k in ("frame_info", "frame_info2", "payload_md5", "payload_len", "stat")}
        check(got[i], a, c, "%s chain %d" % (name, i))
        gave_up += int(a["stat"][:, 3].sum())
        intra_mid += int((a["frame_info"][1:, 0] == 2).sum())
    assert intra_mid > 0, "no scene cut was acted on: the clips do not test it"
    if not cs[0]["pre_scenecut"]:
        assert gave_up > 0, "no attempt was given up: the clips do not test the post-encode scene cut"


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libx264ref.so not built (the fixtures hold the same configurations)")
@pytest.mark.parametrize("name", sorted(LC.LL_STREAMS))
def test_lossless_stream_equals_reference_live(hip_lib, name):
    cs = [dict(c, t0=c["t0"] + 47) for c in LC.LL_STREAMS[name]]
    got = run_stream(hip_lib, cs)
    for i, c in enumerate(cs):
        check(got[i], LC.stream_fixture(K.reference_records(c), c["frames"]), c, "%s chain %d (live)" % (name, i))


def test_lossless_lookahead_costs_and_vectors_equal_the_references_queue(hip_lib):
    """x264hip_lookahead_intra_frame_sad + x264hip_lookahead_cost_frames with lossless = 1, task by task: every P picture of the pre-scenecut
    streams scored against its predecessor -- the frame's score, its intra macroblock count and intra cost (fenc->i_cost_est[1][0], i_intra_mbs[1],
    i_cost_est[0][0]) and every half-resolution vector the search leaves for the main encode, as x264_slicetype_decide's queue had them."""
    gold = np.load(os.path.join(GOLDEN, "ll_stream_presc.npz"))
    cs = LC.LL_STREAMS["presc"]
    c0, frames = cs[0], cs[0]["frames"]
    clips = [K.clip(c["w"], c["h"], frames, c["cut"], c["t0"], c["slow"]) for c in cs]
    ctx = FrameCtx(hip_lib, c0["w"], c0["h"], batch=len(cs))
    dev = LA.LookaheadDevice(ctx, n_slots=frames, bframes=0, me_method=c0["me"], me_range=16, subme=c0["subme"], lossless=1)
    try:
        for f in range(frames):
            pic = dev.begin_frame(f)
            for b, (y, u, v) in enumerate(clips):
                ctx.upload(pic, y[f], u[f], v[f], b=b)
            dev.prepare(f)
        checked = 0
        for i in range(len(cs)):
            info, info2, cost, lm = (gold["c%d_%s" % (i, k)] for k in ("frame_info", "frame_info2", "look_cost", "look_mv"))
            for f in range(frames):
                b = int(info2[f][0])
                if int(info[f][0]) != 0 or int(cost[f][0]) < 0:       # P pictures the queue scored (an I picture's vectors are never offered)
                    continue
                res = dev.run([(i, b, b - 1, b, 1, 0)])
                assert tuple(int(x) for x in res[0]) == (int(cost[f][0]), int(cost[f][2]), int(cost[f][3])), \
                    "chain %d picture %d: (score, intra macroblocks, intra cost) %s, the reference %s" % (i, b, tuple(int(x) for x in res[0]), (int(cost[f][0]), int(cost[f][2]), int(cost[f][3])))
                if lm[f][0, 0, 0] != 0x7fff:
                    mv = dev.mv_host(i, b, 0, 1)
                    assert np.array_equal(mv, lm[f][0]), "chain %d picture %d: %d half-resolution vectors differ" % (i, b, int((mv != lm[f][0]).any(1).sum()))
                    checked += 1
        assert checked >= frames
    finally:
        dev.close()


def test_lossy_sad_lookahead_stays_refused(hip_lib):
    """subme < 2 without lossless: still refused, with the message it always had."""
    ctx = FrameCtx(hip_lib, 128, 96, batch=1)
    dev = LA.LookaheadDevice(ctx, n_slots=3, bframes=1, subme=1)
    for f in range(2):
        dev.begin_frame(f)
    with pytest.raises(RuntimeError, match="SATD"):
        dev.run([(0, 1, 0, 1, 1, 0)])
    dev.close()


@pytest.mark.parametrize("y4m", [True, False])
def test_cli_qp0_with_default_options(hip_lib, tmp_path, y4m):
    """`python -m x264_vs2008_amd.encode --qp 0 -o out.264 in.y4m` (and the same from a raw file): the reference's default options -- subme 6, the
    frame queue with the post-encode scene cut -- with what x264_validate_parameters does to them at QP 0.  The file is the reference encoder's
    payloads inside this library's headers (profile 244 SPS), as tests/test_gpu_encode_cli.py builds its expectations."""
    c = LC.CLI_CLIP
    src = str(tmp_path / ("in.y4m" if y4m else "in_%dx%d.yuv" % (c["w"], c["h"])))
    out = str(tmp_path / "out.264")
    write_clip(src, c["w"], c["h"], c["n"], t0=c["t0"], y4m=y4m)
    extra = [] if y4m else ["--fps", "25/1"]          # (a y4m carries its rate: F25:1)
    assert E.main(LC.CLI_ARGS.split() + extra + ["-o", out, src]) == 0
    p = LC.cli_params(hip_lib)
    assert p.d_lossless and p.d_profile_idc == 244
    got = open(out, "rb").read()
    gold = np.load(os.path.join(GOLDEN, "ll_cli.npz"))
    refs = [("fixture", {k: gold[k] for k in gold.files})]
    if os.path.exists(REF_SO):
        refs.append(("live", LC.cli_reference(p)))
    for what, a in refs:
        m, want = mux.AnnexB(hip_lib, p), b""
        for f in range(c["n"]):
            st, qp, _, poc = (int(x) for x in a["frame_info"][f])
            ft = (mux.TYPE_IDR if poc == 0 else mux.TYPE_I) if st == 2 else mux.TYPE_P
            want += m.frame(frame=int(a["frame_info2"][f][0]), ftype=ft, qp=qp, payload=bytes(a["payload"][f, :a["payload_len"][f]]))
        assert got == want, "%s: %d vs %d bytes" % (what, len(got), len(want))
