"""Noise reduction (--nr) in B slices and under the post-encode scene cut, on the GPU, bit for bit against the reference -- live where
oracle/_ref/libx264ref.so is built, tests/golden/nr_b_*.npz otherwise (tests/nr_b_cases.py):

  * lock-step B chains (ChainEncoder): both strengths, one and two B frames between the anchors, below and at the RD levels, the CAVLC
    pass, trellis, psy-RD and adaptive quantisation, weighted and temporal direct prediction, mixed references;
  * pictures of one, two and six macroblocks; chains of a batch against their own single-chain runs;
  * x264hip_noise_reduction_update_chains: the listed chains against a numpy restatement of x264_noise_reduction_update, every other
    chain untouched, what it refuses;
  * StreamEncoder: the pre- and the post-encode scene cut (given-up attempts keep their additions to the sums, one update per returned
    frame), CAVLC, chains of different lengths in one batch, BASELINE's MED flag set, and the command line with its defaults;
  * what stays refused: lossless B slices, AsyncStreamEncoder with --nr."""
import ctypes as C

import numpy as np
import pytest

import edge_cases as ec
import nr_b_cases as nb
from oracle import refslice as rs
from x264_vs2008_amd import encode as E
from x264_vs2008_amd import mux
from x264_vs2008_amd import slice as sl
from x264_vs2008_amd.abi import NrState
from x264_vs2008_amd.frame import DeviceArray, FrameCtx, cqm_init
from x264_vs2008_amd.stream import AsyncStreamEncoder, StreamEncoder

pytestmark = pytest.mark.gpu
STATE = ("mb_type", "qp", "mv", "ref", "cbp", "t8", "partition", "sub_partition", "luma", "luma_dc", "chroma_dc", "chroma_ac")


def get1(enc, state, name, shape, dt):
    out = np.zeros(shape, dt)
    assert enc.ctx.lib.x264hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), getattr(state.st, name), out.nbytes) == 0
    return out


def run_chains(hip_lib, cqm, c, clips):
    """The case's chain on every clip of `clips` (one batch): per chain the arrays of oracle/refslice.py's output, frames in coding order.
    fin_* of a B frame (never filtered, never kept) is its reconstruction."""
    kw = {k: v for k, v in c["kw"].items() if k != "cqm_preset"}
    B, (w, h), frames = len(clips), c["size"], c["frames"]
    enc = sl.ChainEncoder(hip_lib, w, h, cqm, batch=B, write=1, **kw, **c["ext"])
    order = sl.coding_order(frames, kw.get("keyint", 0), c["ext"]["bframes"])
    n = ((w + 15) // 16) * ((h + 15) // 16)
    out = [{k: [] for k in STATE + ("mv1", "ref1", "payload", "frame_info", "frame_info2") + tuple(p + q for p in ("rec_", "fin_") for q in "yuv")} for _ in clips]
    try:
        for disp, stype in order:
            for b, (y, u, v) in enumerate(clips):
                enc.upload(y[disp], u[disp], v[disp], b=b)
            st, qp, state = enc.encode_frame(stype=stype, disp=disp)
            enc.status()                                   # (raises on an abort flag)
            got = {k: state.get(k) for k in STATE}
            got["mv1"], got["ref1"] = get1(enc, state, "mv1", (B, n, 16, 2), np.int16), get1(enc, state, "ref1", (B, n, 4), np.int8)
            pays = enc.payloads()
            rec = {pl: [enc.ctx.download(enc.last[0], pl, padded=False, b=b) for b in range(B)] for pl in "yuv"}
            enc.finish_frame()
            enc.ctx.sync()
            for b in range(B):
                o = out[b]
                for k in STATE + ("mv1", "ref1"):
                    o[k].append(got[k][b])
                o["payload"].append(pays[b])
                o["frame_info"].append((st, qp))
                o["frame_info2"].append((disp,))
                for pl in "yuv":
                    o["rec_" + pl].append(rec[pl][b])
                    o["fin_" + pl].append(rec[pl][b] if stype == sl.SLICE_B else enc.ctx.download(enc.refs[0][0], pl, padded=False, b=b))
    finally:
        enc.close()
    for o in out:
        pay = o.pop("payload")
        o["payload_len"] = np.array([len(p) for p in pay], np.int32)
        o["payload"] = np.zeros((frames, max(len(p) for p in pay)), np.uint8)
        for f, p in enumerate(pay):
            o["payload"][f, :len(p)] = np.frombuffer(p, np.uint8)
        for k in list(o):
            if k not in ("payload", "payload_len"):
                o[k] = np.stack([np.asarray(x) for x in o[k]])
    return out


def check_chain(name, got, want):
    """One chain's arrays against digest()'s form of the reference's: slice types, QPs and display order, payload bytes, decisions, levels,
    both vector lists, reconstruction and filtered planes of every frame."""
    g = nb.digest(got, cavlc=nb.is_cavlc(name))
    frames = len(want["payload_len"])
    stypes = want["frame_info"][:, 0]
    assert g["frame_info"][:, 0].tolist() == stypes.tolist() and g["frame_info2"][:, 0].tolist() == want["frame_info2"][:, 0].tolist(), name
    for f in range(frames):
        tag = "%s frame %d (%s)" % (name, f, "PBI"[int(stypes[f])])
        assert int(g["frame_info"][f, 1]) == int(want["frame_info"][f, 1]), tag + ": slice QP"
        for k in ("mb_type", "qp"):
            assert np.array_equal(g[k][f], want[k][f]), "%s: %s differs first at %s" % (tag, k, np.argwhere(g[k][f] != want[k][f])[:4].tolist())
        for k in nb.CHAIN_DIGESTS:
            if (stypes[f] == sl.SLICE_I and k in ("mv", "ref")) or (stypes[f] != sl.SLICE_B and k in ("mv1", "ref1")):
                continue                                   # (never written, never read)
            assert bytes(g[k + "_md5"][f]) == bytes(want[k + "_md5"][f]), "%s: %s differs" % (tag, k)
        a, b = nb.payload(g, f), nb.payload(want, f)
        assert a == b, "%s: payload differs (%d vs %d bytes)" % (tag, len(a), len(b))


# ---- 1. lock-step B chains against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(nb.LOCK))
def test_b_chains_with_nr_match_the_reference(hip_lib, cqm, name):
    c, want = nb.LOCK[name], nb.want(name)
    assert not nb.condition_problems(name, want), nb.condition_problems(name, want)      # --nr bites in a B frame of this case
    check_chain(name, run_chains(hip_lib, cqm, c, [nb.clip_of(c)])[0], want)


# ---- 2. the smallest pictures ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(nb.SMALL))
def test_b_chains_with_nr_on_the_smallest_pictures(hip_lib, cqm, name):
    c = nb.SMALL[name]
    check_chain(name, run_chains(hip_lib, cqm, c, [nb.clip_of(c)])[0], nb.want(name))


# ---- 3. chains of a batch stay independent ---------------------------------------------------------------------------------------------------
def test_chains_of_a_batch_keep_their_own_sums(hip_lib, cqm):
    c = dict(nb.LOCK["s5_nr400_b2"], kw=dict(nb.LOCK["s5_nr400_b2"]["kw"], noise_reduction=150))
    clips = [rs.clip(c["size"][0], c["size"][1], c["frames"], t0) for t0 in (0, 13, 29)]
    batch = run_chains(hip_lib, cqm, c, clips)
    for b, clip in enumerate(clips):
        alone = run_chains(hip_lib, cqm, c, [clip])[0]
        for f in range(c["frames"]):
            assert nb.payload(batch[b], f) == nb.payload(alone, f), "chain %d frame %d: payload differs from the single-chain run" % (b, f)
        for k in ("mb_type", "qp", "luma", "fin_y"):
            assert np.array_equal(batch[b][k], alone[k]), "chain %d: %s" % (b, k)
    assert len({nb.payload(batch[b], 2) for b in range(3)}) == 3


# ---- 4. x264hip_noise_reduction_update_chains ------------------------------------------------------------------------------------------------
W4 = np.array([800, 320, 800, 320, 320, 128, 320, 128, 800, 320, 800, 320, 320, 128, 320, 128], np.uint64)      # x264_dct4_weight2_tab
W8K = np.array([256, 201, 656, 227, 410, 363], np.uint64)                                                             # x264_dct8_weight2_tab's W(i)
K8 = np.array([0, 3, 4, 3, 0, 3, 4, 3, 3, 1, 5, 1, 3, 1, 5, 1, 4, 5, 2, 5, 4, 5, 2, 5, 3, 1, 5, 1, 3, 1, 5, 1], np.int64)
W8 = W8K[K8[np.arange(64) & 31]]


def nr_update_numpy(s, cnt, off, strength):
    """x264_noise_reduction_update, R/encoder/macroblock.c:890-911, on one chain's sum [2][64] uint32, count [2] uint32, offset [2][64] uint16."""
    s, cnt, off = s.copy(), cnt.copy(), off.copy()
    for cat in range(2):
        size, w = (64, W8) if cat else (16, W4)
        if cnt[cat] > (1 << 16 if cat else 1 << 18):
            s[cat, :size] >>= 1
            cnt[cat] >>= 1
        sv = s[cat, :size].astype(np.uint64)
        off[cat, :size] = ((np.uint64(strength) * np.uint64(cnt[cat]) + sv // np.uint64(2)) // (sv * w // np.uint64(256) + np.uint64(1))).astype(np.uint16)
    return s, cnt, off


def test_update_chains_updates_the_listed_chains_and_no_other(hip_lib):
    B, strength = 4, 137
    ctx = FrameCtx(hip_lib, 64, 48, batch=B)
    nr = NrState()
    ctx.check(hip_lib.x264hip_nr_state_alloc(ctx.h, C.byref(nr)), "nr_state_alloc")
    r = np.random.default_rng(20)
    s = r.integers(0, 1 << 27, (B, 2, 64), dtype=np.uint32)
    s[:, 0, 16:] = 0
    off = r.integers(0, 1 << 12, (B, 2, 64)).astype(np.uint16)
    off[:, 0, 16:] = 0
    cnt = np.array([[(1 << 18) + 16, 4096],           # chain 0 (listed): the 4x4 count above its threshold
                    [3 << 18, 100],                   # chain 1 (not listed): above TWICE its threshold -- an update too many would show
                    [1024, (1 << 16) + 4],            # chain 2 (listed): the 8x8 count above its threshold
                    [0, 0]], np.uint32)               # chain 3 (not listed): nothing coded yet
    s[3], off[3] = 0, 0
    lst = DeviceArray(hip_lib, (B,), np.int32)

    def put(a, p):
        assert hip_lib.x264hip_memcpy_h2d(p, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0

    def get():
        ctx.sync()
        out = []
        for a, p in ((s, nr.sum), (cnt, nr.count), (off, nr.offset)):
            o = np.zeros_like(a)
            assert hip_lib.x264hip_memcpy_d2h(o.ctypes.data_as(C.c_void_p), p, o.nbytes) == 0
            out.append(o)
        return out

    def call(state, chains, n, dev=True):
        if chains is not None:
            lst.set(np.array(list(chains) + [0] * (B - len(chains)), np.int32))
        rc = hip_lib.x264hip_noise_reduction_update_chains(ctx.h, C.byref(state) if state is not None else None, strength, lst.p if dev else None, n)
        return rc, hip_lib.x264hip_last_error().decode()

    try:
        ctx.sync()
        for a, p in ((s, nr.sum), (cnt, nr.count), (off, nr.offset)):
            put(a, p)
        rc, msg = call(nr, [2, 0], 2)
        assert rc == 0, msg
        s1, c1, o1 = get()
        for b in (0, 2):
            ws, wc, wo = nr_update_numpy(s[b], cnt[b], off[b], strength)
            assert np.array_equal(s1[b], ws) and np.array_equal(c1[b], wc) and np.array_equal(o1[b], wo), "chain %d" % b
        assert c1[0, 0] == cnt[0, 0] >> 1 and c1[2, 1] == cnt[2, 1] >> 1 and c1[0, 1] == cnt[0, 1] and c1[2, 0] == cnt[2, 0]
        for b in (1, 3):
            assert s1[b].tobytes() == s[b].tobytes() and c1[b].tobytes() == cnt[b].tobytes() and o1[b].tobytes() == off[b].tobytes(), "chain %d was touched" % b
        before = [a.tobytes() for a in (s1, c1, o1)]
        rc, msg = call(nr, [], 0)                          # an empty list: nothing changes
        assert rc == 0 and [a.tobytes() for a in get()] == before, msg
        rc, msg = call(nr, None, 0, dev=False)
        assert rc == 0 and [a.tobytes() for a in get()] == before, msg
        # refused before any launch
        for state, chains, n, dev, word in ((None, [0], 1, True, "no state"), (NrState(), [0], 1, True, "no state"), (nr, [0], -1, True, "chains of a batch"),
                                            (nr, [0], B + 1, True, "chains of a batch"), (nr, None, 2, False, "without a list")):
            rc, msg = call(state, chains, n, dev)
            assert rc == -1 and word in msg, (n, dev, msg)
            assert [a.tobytes() for a in get()] == before, word
        # an index outside the batch inside the list: skipped, the entry beside it is served
        rc, msg = call(nr, [B, -1, 7 * B], 3)
        assert rc == 0 and [a.tobytes() for a in get()] == before, msg
        rc, msg = call(nr, [B, 1], 2)
        assert rc == 0, msg
        s2, c2, o2 = get()
        ws, wc, wo = nr_update_numpy(s[1], cnt[1], off[1], strength)
        assert np.array_equal(s2[1], ws) and np.array_equal(c2[1], wc) and np.array_equal(o2[1], wo)
        for b in (0, 2, 3):
            assert s2[b].tobytes() == s1[b].tobytes() and c2[b].tobytes() == c1[b].tobytes() and o2[b].tobytes() == o1[b].tobytes(), "chain %d was touched" % b
    finally:
        lst.free()
        hip_lib.x264hip_nr_state_free(ctx.h, C.byref(nr))
        ctx.close()


# ---- 5. streams ------------------------------------------------------------------------------------------------------------------------------
def spy_on_updates(hip_lib, monkeypatch):
    """Every x264hip_noise_reduction_update_chains call from here on leaves the chains it lists (read back from the device list) in the
    returned list; the lock-step update must not be called at all."""
    real, calls = hip_lib.x264hip_noise_reduction_update_chains, []

    def spy(h, nr, strength, lst, n):
        a = np.zeros(max(n, 1), np.int32)
        assert hip_lib.x264hip_memcpy_d2h(a.ctypes.data_as(C.c_void_p), lst, 4 * n) == 0
        calls.append(a[:n].tolist())
        return real(h, nr, strength, lst, n)

    def never(*a):
        raise AssertionError("StreamEncoder called the all-chains update")
    monkeypatch.setattr(hip_lib, "x264hip_noise_reduction_update_chains", spy)
    monkeypatch.setattr(hip_lib, "x264hip_noise_reduction_update", never)
    return calls


def run_stream(hip_lib, cs, limits=None, **more):
    """The chains `cs` (one encoder configuration, their own clips) through the StreamEncoder: per chain [(input frame, slice type, qp,
    payload)] in coding order, the encoder's count of given-up attempts, and per step that coded something (chains that coded, launches)."""
    c, frames = cs[0], max(x["frames"] for x in cs)
    clips = [nb.stream_clip(dict(x, frames=frames)) for x in cs]
    enc = StreamEncoder(hip_lib, c["w"], c["h"], cqm_init(hip_lib), batch=len(cs), limits=limits, crf=c["crf"], b_adapt=c["b_adapt"], bframe_bias=c["bframe_bias"],
                        keyint_min=c["keyint_min"], scenecut_threshold=c["scenecut_threshold"], pre_scenecut=c["pre_scenecut"], qp=c["qp"], me_method=c["me"],
                        me_range=16, subme=c["subme"], n_refs=c["n_refs"], inter=c["inter"], intra=0x3, transform8x8=1, cabac=c["cabac"], deblock=1,
                        keyint=c["keyint"], aq_mode=c["aq"], aq_strength=1.0, bframes=c["bframes"], weightb=c["weightb"], direct_pred=c.get("direct_pred", 1),
                        qp_min=0, noise_reduction=c["noise_reduction"], **more)
    got, steps = [[] for _ in cs], []

    def fill(pic, f):
        for b, (y, u, v) in enumerate(clips):
            enc.src_ctx.upload(pic, y[f], u[f], v[f], b=b)

    try:
        fed, idle = 0, 0
        for _ in range(4 * frames + 40):
            before = enc.n_sweeps
            coded = enc.step(fill if fed < frames else None)
            if coded:
                steps.append(([cd.chain for cd in coded], enc.n_sweeps - before))
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
        given_up = enc.n_given_up
    finally:
        enc.close()
    return got, given_up, steps


def check_stream(name, got, want):
    assert len(got) == len(want["payload_len"]), "%s: %d frames coded, the reference codes %d" % (name, len(got), len(want["payload_len"]))
    for f, (frame, st, qp, pay) in enumerate(got):
        ref = (int(want["frame_info2"][f][0]), int(want["frame_info"][f][0]), int(want["frame_info"][f][1]))
        assert (frame, st, qp) == ref, "%s coded frame %d: (input, slice, qp) %s, the reference %s" % (name, f, (frame, st, qp), ref)
        assert pay == nb.payload(want, f), "%s coded frame %d (input %d, slice %d, qp %d): payload differs (%d vs %d bytes)" % (
            name, f, frame, st, qp, len(pay), int(want["payload_len"][f]))


@pytest.mark.parametrize("name", sorted(nb.STREAMS))
def test_streams_with_nr_match_the_reference_encoder(hip_lib, monkeypatch, name):
    c, want = nb.STREAMS[name], nb.want(name)
    assert not nb.condition_problems(name, want), nb.condition_problems(name, want)
    updates = spy_on_updates(hip_lib, monkeypatch)
    got, given_up, steps = run_stream(hip_lib, [c])
    check_stream(name, got[0], want)
    assert given_up == int(want["stat"][:, 3].sum()) and (given_up >= 1 or not nb.given_up(name))
    # one update per returned frame, behind the step's last launch: a given-up attempt is a second launch of its step without a second update
    assert updates == [[0]] * c["frames"] and sum(n for _, n in steps) == c["frames"] + given_up


def test_stream_chains_of_different_lengths_equal_their_single_stream_runs(hip_lib, monkeypatch):
    """Chain 1 is fed two pictures fewer than chain 0: it codes nothing in some steps of the flush, where its tables must stay as they
    are -- the update's list names the chains that coded a frame for good in the step, and no other."""
    cs = nb.STAGGER
    updates = spy_on_updates(hip_lib, monkeypatch)
    got, _, steps = run_stream(hip_lib, cs, limits=[x["frames"] for x in cs])
    assert [sorted(u) for u in updates] == [sorted(chains) for chains, _ in steps] and [0] in updates and [0, 1] in [sorted(u) for u in updates]
    for b, c in enumerate(cs):
        alone, _, _ = run_stream(hip_lib, [c])
        assert len(got[b]) == c["frames"] == len(alone[0])
        for f, (x, y) in enumerate(zip(got[b], alone[0])):
            assert x[:3] == y[:3] and x[3] == y[3], "chain %d coded frame %d: %s in the batch, %s alone (%d vs %d bytes)" % (b, f, x[:3], y[:3], len(x[3]), len(y[3]))
    assert any(st == sl.SLICE_B for _, st, _, _ in got[1])


# ---- 5e / 6. the command line ----------------------------------------------------------------------------------------------------------------
def mux_want(hip_lib, p, want):
    """The Annex B stream around the reference's payloads (mux_cases.mux_reference_stream on digest()'s arrays)."""
    import mux_cases as M
    return M.mux_reference_stream(hip_lib, p, want, len(want["payload_len"]))


@pytest.mark.parametrize("name", sorted(nb.CLI))
def test_command_line_with_nr_writes_the_reference_encoder_stream(hip_lib, tmp_path, name):
    """cli_med: BASELINE's MED flag set plus --nr 100; cli_default: --nr 100 --crf 23 --bframes 2 and nothing about scene cuts, i.e. the
    post-encode scene cut."""
    import mux_cases as M
    c = nb.CLI[name]
    src, out = str(tmp_path / "in.y4m"), str(tmp_path / "o.264")
    M.write_clip(src, c["w"], c["h"], c["frames"], t0=c["t0"], y4m=True)
    assert E.main(c["args"].split() + ["-o", out, src]) == 0
    p = nb.cli_params(c, hip_lib)
    assert p.noise_reduction == 100 and p.bframe >= 2 and not p.pre_scenecut and p.scenecut_threshold == 40
    E.check_built(p)
    want = nb.want(name)
    assert not nb.condition_problems(name, want), nb.condition_problems(name, want)
    got = open(out, "rb").read()
    wanted = mux_want(hip_lib, p, want)
    assert got == wanted, "%s: %d vs %d bytes" % (name, len(got), len(wanted))


# ---- 7. what stays refused -------------------------------------------------------------------------------------------------------------------
def test_lossless_b_slices_and_the_async_encoder_stay_refused(hip_lib, cqm):
    y, u, v = ec.clip("noise", (40, 24), 2)
    enc = sl.ChainEncoder(hip_lib, 40, 24, cqm, qp=0, subme=5, me_method=1, n_refs=1, inter=0x113, intra=0x3, transform8x8=1, cabac=1, write=1, bframes=1, noise_reduction=80)
    try:
        assert enc.nr is None                              # x264_validate_parameters: lossless turns --nr off
        for disp, stype in ((0, sl.SLICE_I), (2, sl.SLICE_P)):
            enc.upload(y[0], u[0], v[0])
            enc.encode_frame(stype=stype, disp=disp)
            enc.finish_frame()
        enc.upload(y[1], u[1], v[1])
        with pytest.raises(RuntimeError, match="B slices"):
            enc.encode_frame(stype=sl.SLICE_B, disp=1)
    finally:
        enc.close()
    with pytest.raises(ValueError, match="--nr"):
        AsyncStreamEncoder(hip_lib, 96, 80, cqm_init(hip_lib), batch=1, n_frames=4, crf=23.0, qp=26, subme=5, cabac=1, bframes=1, inter=0x113, intra=0x3,
                           keyint=250, noise_reduction=100)
    with pytest.raises(ValueError, match="lanes"):         # B frames on lanes run beside the next anchor: the sums would race
        sl.ChainEncoder(hip_lib, 96, 80, cqm, qp=26, subme=5, me_method=1, n_refs=1, inter=0x113, intra=0x3, cabac=1, write=1, bframes=2, lanes=2, noise_reduction=80)
