"""Sub-8x8 P partitions under the RD levels (--partitions all with --subme 6..9) on the GPU: the refinement kernels with the chain's record
of cache leftovers (x264hip_slice_rd.mb_carry) against the REFERENCE -- decisions, per-macroblock QP, reconstruction and payload bytes.

  * the two chains of the reference that only pinned the twin so far (tests/golden/slice2_rd8_sub8x8.npz, slice2_rd9_sub8x8_nodec.npz: keyint 4,
    so the carry crosses an I frame), alone and as three chains of one launch;
  * the cases of tests/sub8_rd_cases.py: subme 6-9, trellis 1 / 2, psy-rd on / off, AQ, psy-trellis (k_psy_raster's refinement kernel), UMH,
    1 and 3 mixed references, chroma_me = 0, dct_decimate = 0, pictures of one to six macroblocks -- live where oracle/_ref is built, from
    tests/golden/sub8rd_*.npz otherwise;
  * the chain table: StreamEncoder (CRF, no B frames, the post-encode scene cut giving P attempts up) against the reference's whole encoder,
    and the command line through both of its paths;
  * what stays refused: no mb_carry, lossless, B frames (a B slice handed mb_carry, ChainEncoder / StreamEncoder with bframes), the async
    encoder, the sharded clip, a chain table that mixes entries with and without mb_carry."""
import os

import numpy as np
import pytest

import sub8_rd_cases as SC
from oracle import refslice as rs
from oracle.gen_golden_slice import CASES2_TWIN, case_inputs
from paths import GOLDEN
from slice_util import check_frame, run_chain2
from x264_vs2008_amd import encode as E
from x264_vs2008_amd import mux
from x264_vs2008_amd import slice as sl
from x264_vs2008_amd.frame import DeviceArray, cqm_init
from x264_vs2008_amd.stream import AsyncStreamEncoder, StreamEncoder

pytestmark = pytest.mark.gpu
OLD = {c[0]: c for c in CASES2_TWIN if "sub8x8" in c[0]}


def check_all(d, gold, f, n_refs, b=0, what=""):
    """One frame of one chain: every state array, both reconstructions, the statistics (slice_util.check_frame), and the payload bytes."""
    pcm = gold["mb_type"][f] == rs.I_PCM
    if pcm.any():
        # the harness copies rec_* out between x264_macroblock_encode and the writer (oracle/ref_slice.c), and an I_PCM macroblock's reconstruction -- the
        # source -- reaches fdec in the writer: inside such a macroblock rec_* holds the last trial's pixels, not the reconstruction.  fin_* (whole frame,
        # compared in full) is taken after it; an I_PCM macroblock has QP 0 and its inside is never filtered, so fin_* is its reconstruction
        mb_w = gold["rec_y"].shape[2] // 16
        m = pcm.reshape(-1, mb_w)
        d, gold = dict(d), dict(gold)
        for nm, k in (("y", 16), ("u", 8), ("v", 8)):
            mm = np.repeat(np.repeat(m, k, 0), k, 1)
            rec = gold["rec_" + nm].copy()
            rec[f] = np.where(mm, 0, rec[f])
            gold["rec_" + nm] = rec
            dd = d["rec_" + nm].copy()
            dd[b] = np.where(mm, 0, dd[b])
            d["rec_" + nm] = dd
    check_frame(d, gold, f, n_refs, b=b)
    want = bytes(gold["payload"][f, :int(gold["payload_len"][f])])
    assert d["payload"][b] == want, "%sframe %d: payload differs (%d vs %d bytes)" % (what, f, len(d["payload"][b]), len(want))


def slices_of(gold):
    return gold["frame_info"][:, 0].tolist()


@pytest.mark.parametrize("name", sorted(OLD))
def test_reference_chains_with_the_carry(hip_lib, cqm, name):
    _, size, frames, kind, kw, ekw = OLD[name]
    with np.load(os.path.join(GOLDEN, "slice2_%s.npz" % name)) as z:
        gold = {k: z[k] for k in z.files}
    y, u, v = case_inputs(size, frames, kind)
    out = run_chain2(hip_lib, cqm, size, frames, y, u, v, kw, dict(ekw, mb_carry=True))
    for f in range(frames):
        check_all(out[f], gold, f, kw["n_refs"])
    assert int(((gold["mb_type"] == rs.P_8x8)[..., None] & (gold["sub_partition"] != 3)).sum()) > 0


@pytest.mark.parametrize("name", sorted(OLD))
def test_three_chains_in_one_launch(hip_lib, cqm, name):
    """batch = 3: every chain against its own slot of the carry."""
    _, size, frames, kind, kw, ekw = OLD[name]
    with np.load(os.path.join(GOLDEN, "slice2_%s.npz" % name)) as z:
        gold = {k: z[k] for k in z.files}
    y, u, v = case_inputs(size, frames, kind)
    out = run_chain2(hip_lib, cqm, size, frames, y, u, v, kw, dict(ekw, mb_carry=True), batch=3)
    for f in range(frames):
        for b in range(3):
            check_all(out[f], gold, f, kw["n_refs"], b=b, what="chain %d " % b)


@pytest.mark.parametrize("name", sorted(SC.CHAINS))
def test_new_reference_cases(hip_lib, cqm, name):
    c = SC.CHAINS[name]
    gold = SC.want(name)
    assert not SC.condition_problems(name, gold), SC.condition_problems(name, gold)
    y, u, v = SC.clip_of(c)
    out = run_chain2(hip_lib, cqm, c["size"], c["frames"], y, u, v, c["kw"], dict(c["ext"], mb_carry=True))
    for f in range(c["frames"]):
        check_all(out[f], gold, f, c["kw"]["n_refs"])
    assert rs.SLICE_I in slices_of(gold) and rs.SLICE_P in slices_of(gold)


def stream_encoder(hip_lib, c, cls=StreamEncoder, batch=1, **more):
    kw, e = c["kw"], c["ext"]
    return cls(hip_lib, c["size"][0], c["size"][1], cqm_init(hip_lib), batch=batch, crf=e["crf"], b_adapt=0, bframe_bias=0, keyint_min=0,
               scenecut_threshold=e["scenecut_threshold"], pre_scenecut=e["pre_scenecut"], me_range=16, aq_mode=e["aq_mode"], aq_strength=e["aq_strength"],
               trellis=e.get("trellis", 0), psy_rd=e.get("psy_rd", 0.0), bframes=0, qp_min=0, **kw, **more)


@pytest.mark.parametrize("name", sorted(SC.STREAMS))
def test_stream_encoder_equals_the_reference_encoder(hip_lib, name):
    """The chain table: StreamEncoder turns the carry on itself; two chains code the same clip, each against its own slot.  Where the post-encode scene
    cut gives a P attempt up, the attempt's leftovers are what the I frame coded in its place starts from."""
    c = SC.STREAMS[name]
    gold = SC.want(name)
    assert not SC.condition_problems(name, gold), SC.condition_problems(name, gold)
    y, u, v = SC.clip_of(c)
    frames, B = c["frames"], 2
    enc = stream_encoder(hip_lib, c, batch=B)
    assert "mb_carry" in enc.rd_bufs
    got = [[] for _ in range(B)]

    def fill(pic, f):
        for b in range(B):
            enc.src_ctx.upload(pic, y[f], u[f], v[f], b=b)
    try:
        fed, idle = 0, 0
        for _ in range(4 * frames + 40):
            coded = enc.step(fill if fed < frames else None)
            fed += fed < frames
            idle = 0 if coded else idle + (fed >= frames and enc.flushing)
            if idle >= 2:
                break
            if coded:
                enc.sync()
                enc.status()
                pl = enc.payloads()
                for cd in coded:
                    got[cd.chain].append((cd.frame, cd.slice_type, cd.qp, pl[cd.chain]))
        assert enc.n_given_up >= B * int(c.get("given_up", 0))
    finally:
        enc.close()
    for b in range(B):
        assert len(got[b]) == frames, "chain %d: %d frames coded, the reference codes %d" % (b, len(got[b]), frames)
        for f, (frame, st, qp, payload) in enumerate(got[b]):
            ref = (int(gold["frame_info2"][f][0]), int(gold["frame_info"][f][0]), int(gold["frame_info"][f][1]))
            assert (frame, st, qp) == ref, "chain %d coded frame %d: (input, slice, qp) %s, the reference %s" % (b, f, (frame, st, qp), ref)
            want = bytes(gold["payload"][f, :int(gold["payload_len"][f])])
            assert payload == want, "chain %d coded frame %d (input %d, slice %d, qp %d): payload differs (%d vs %d bytes)" % (b, f, frame, st, qp, len(payload), len(want))


class Clip:
    def __init__(self, y, u, v):
        self.planes = (y, u, v)

    def read(self, t):
        return tuple(p[t] for p in self.planes)


class Sink:
    def __init__(self):
        self.parts = []

    def write(self, b):
        self.parts.append(bytes(b))


@pytest.mark.parametrize("name,args", [("s7_umh_1ref", "--qp 18 --scenecut -1 --bframes 0 --ref 1 --me umh --subme 7 --8x8dct --partitions all --trellis 1 --psy-rd 1.0:0"),
                                       ("stream_cut_s8", "--crf 17 --bframes 0 --ref 2 --me hex --subme 8 --8x8dct --partitions all --trellis 1 --aq-mode 1 --psy-rd 1.0:0")])
def test_command_line_paths(hip_lib, name, args):
    """encode.py with --partitions all at the RD levels: without the frame queue (constant QP, no scene cut: ChainEncoder) and with it (CRF and the default
    scene cut: StreamEncoder) -- the file is the reference's payloads inside this library's headers."""
    from mux_cases import mux_reference_stream
    c = SC.CHAINS.get(name) or SC.STREAMS[name]
    (w, h), n = c["size"], c["frames"]
    o = E.build_parser().parse_args(args.split() + ["-o", "x", "in_%dx%d.yuv" % (w, h)])
    p = mux.encoder_params(hip_lib, width=w, height=h, fps_num=25, fps_den=1, **E.param_fields(o))
    assert p.inter & 0x20 and p.subpel_refine >= 6 and E.needs_lookahead(p) == (name in SC.STREAMS)
    assert (p.subpel_refine, p.frame_reference, p.trellis, p.aq_mode) == (c["kw"]["subme"], c["kw"]["n_refs"], c["ext"]["trellis"], c["ext"].get("aq_mode", 0))       # (constant QP has no AQ)
    gold = SC.want(name)
    sink = Sink()
    assert E.encode_streams(hip_lib, p, [Clip(*SC.clip_of(c))], n, [sink]) == n
    got, want = b"".join(sink.parts), mux_reference_stream(hip_lib, p, gold, n)
    assert got == want, "%d vs %d bytes" % (len(got), len(want))


# ---- what stays refused ------------------------------------------------------------------------------------------------------------
RD = dict(qp=24, subme=7, me_method=1, n_refs=1, inter=0x33, intra=0x3, transform8x8=1, cabac=1, write=1)


def test_refused_without_the_carry_and_lossless(hip_lib, cqm):
    y, u, v = case_inputs((48, 32), 1, "moving")
    for kw, needle in ((dict(RD), "sub-8x8"), (dict(RD, qp=0, mb_carry=True), "lossless")):
        enc = sl.ChainEncoder(hip_lib, 48, 32, cqm, **kw)
        try:
            enc.upload(y[0], u[0], v[0])
            with pytest.raises(RuntimeError, match=needle):
                enc.encode_frame()
        finally:
            enc.close()


def test_b_frames_are_refused(hip_lib, cqm):
    """The cut line: the B kernels do not keep the reference's leftovers, so the sweep refuses a B slice handed mb_carry and the encoders refuse bframes."""
    with pytest.raises(ValueError, match="bframes"):
        sl.ChainEncoder(hip_lib, 48, 32, cqm, **dict(RD, inter=0x133), bframes=2, mb_carry=True)
    with pytest.raises(ValueError, match="bframes"):
        sl.ChainEncoder(hip_lib, 48, 32, cqm, **dict(RD, inter=0x133), bframes=2, lanes=2, mb_carry=True)
    with pytest.raises(ValueError, match="bframes"):
        StreamEncoder(hip_lib, 48, 32, cqm, crf=23.0, **dict(RD, inter=0x133), bframes=2)
    y, u, v = case_inputs((48, 32), 3, "moving")
    # the record handed to the sweeps behind ChainEncoder's back: with sub-8x8 RD in the chain's P slices the B slice is refused (the B slice's own
    # level does not matter: at subme 6 it is below the RD levels); in a chain that never reads the record (no 0x20) the B slice is coded
    for inter, refused in ((0x133, True), (0x113, False)):
        enc = sl.ChainEncoder(hip_lib, 48, 32, cqm, **dict(RD, inter=inter, subme=6), bframes=1)
        try:
            enc.rd_bufs["mb_carry"] = DeviceArray(hip_lib, (1, 160), np.uint8, np.zeros((1, 160), np.uint8))
            for disp, stype in ((0, sl.SLICE_I), (2, sl.SLICE_P)):
                enc.upload(y[disp], u[disp], v[disp])
                enc.encode_frame(stype=stype, disp=disp)
                enc.finish_frame()
            enc.upload(y[1], u[1], v[1])
            if refused:
                with pytest.raises(RuntimeError, match="B slice"):
                    enc.encode_frame(stype=sl.SLICE_B, disp=1)
            else:
                enc.encode_frame(stype=sl.SLICE_B, disp=1)
                enc.status()
        finally:
            enc.close()


def test_async_encoder_and_sharded_clip_refuse(hip_lib, cqm):
    from x264_vs2008_amd import shard
    with pytest.raises(ValueError, match="mb_carry"):
        AsyncStreamEncoder(hip_lib, 48, 32, cqm, n_frames=4, crf=23.0, **RD)
    y, u, v = case_inputs((48, 32), 4, "moving")
    with pytest.raises(ValueError, match="mb_carry"):
        shard.encode_clip(hip_lib, cqm, [(y[t], u[t], v[t]) for t in range(4)], 2, **{k: v_ for k, v_ in RD.items() if k != "write"})


def test_chain_table_mixing_entries_with_and_without_the_carry_is_refused(hip_lib):
    """Two chains of a StreamEncoder step without sub-8x8 partitions -- no entry needs the record, so sweep_build refuses none of them -- the first
    entry's x264hip_slice_rd with mb_carry, the second's without: the table itself is refused."""
    c = SC.STREAMS["stream_crf_s9"]
    c = dict(c, kw=dict(c["kw"], inter=0x13))
    y, u, v = SC.clip_of(c)
    enc = stream_encoder(hip_lib, c, batch=2)
    assert "mb_carry" not in enc.rd_bufs
    enc.rd_bufs["mb_carry"] = DeviceArray(hip_lib, (2, 160), np.uint8, np.zeros((2, 160), np.uint8))
    real, n = enc.slice_rd, [0]

    def every_other(rb, *a):
        n[0] += 1
        return real({k: v_ for k, v_ in rb.items() if k != "mb_carry"} if n[0] % 2 == 0 else rb, *a)
    enc.slice_rd = every_other

    def fill(pic, f):
        for b in range(2):
            enc.src_ctx.upload(pic, y[f], u[f], v[f], b=b)
    try:
        with pytest.raises(RuntimeError, match="in every entry or in none"):
            for f in range(4):
                enc.step(fill)
    finally:
        enc.close()
