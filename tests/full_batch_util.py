"""Helpers of the device-filling batch tests (tests/test_gpu_full_batch.py, whose docstring says what is tested and why), of the CPU
checks of their fixtures (tests/test_stream_batch_fixtures.py) and of the recipes that write those fixtures (oracle/gen_golden_stream.py,
oracle/gen_golden_cavlc.py): bench.py's flag sets and batches, the clips and their scramble over the chains, the drivers for the
stream encoder and the lock-step sweeps, and the reference's side."""
import ctypes as C
import os
import time

import numpy as np

import look_cases as K
from oracle import refslice as rs
from paths import REF_SO, ROOT  # noqa: F401  (REF_SO: the fixture tests skip their regeneration without it)
from slice_util import STATE
from stream_util import check, encoder_for
from x264_vs2008_amd import slice as sl
from x264_vs2008_amd.frame import cqm_init

BATCH_LIMIT = 4096                     # x264hip_frame_ctx_new
B_OVER = BATCH_LIMIT - 3               # more chains than resident raster waves, not a multiple of 8

# bench.py's stream mode (analysis_options + rd_options): MED is its default, SLOW its --preset slow; 112x96 (7 x 6 macroblocks, odd mb_w)
_COMMON = dict(w=112, h=96, frames=13, crf=23.0, qp=26, bframes=3, weightb=1, inter=0x113, trellis=1, psy_rd=1.0, mixed_refs=1, aq=1, chroma_me=1,
               pre_scenecut=0, scenecut_threshold=40, keyint=250, keyint_min=0, bframe_bias=0)
FLAGS = {
    # crf 23, ref 3, bframes 3, b-adapt 1, hex, subme 7, 8x8dct, trellis 1, weightb, mixed-refs, direct spatial, AQ, the post-encode scene cut
    "med": dict(_COMMON, n_refs=3, b_adapt=1, me=rs.ME_HEX, subme=7, direct_pred=1),
    # --preset slow: ref 5, b-adapt 2, umh, subme 8, --direct auto
    "slow": dict(_COMMON, n_refs=5, b_adapt=2, me=rs.ME_UMH, subme=8, direct_pred=3),
}
BENCH_BATCH = {"med": 2048, "slow": 1024}          # bench.py --batch's default for the flag set
PIPELINE = {"med": True, "slow": False}            # MED with n_frames given: the lookahead runs ahead of the verdicts (x264hip_lookahead_save / _restore)
# the clips, (cut, t0, slow): no scene change, an early one, a late one; static and repeated pictures; so that the frame-type sequences differ
# (MED's clip 2 has a given-up P attempt)
CLIPS = {
    "med": [(0, 11, 1), (4, 57, 1), (9, 123, 2), (5, 260, 1), (0, 301, 3), (7, 18, 1), (3, 190, 2), (11, 333, 1)],
    "slow": [(0, 29, 1), (5, 71, 1), (10, 144, 2), (0, 222, 3), (6, 305, 1), (4, 9, 2), (8, 377, 1), (0, 250, 2)],
}
LIVE_CLIPS = {                     # the live variant: other places of the clip (MED: three with a given-up P attempt)
    "med": [(0, 1011, 1), (4, 1094, 1), (5, 2012, 2), (8, 1789, 2), (0, 1449, 3), (7, 1203, 1), (3, 1264, 2), (9, 1456, 2)],
    "slow": [(0, 1029, 1), (5, 1108, 1), (10, 1218, 2), (0, 1333, 3), (6, 1453, 1), (4, 1194, 2), (8, 1599, 1), (0, 1509, 2)],
}


def case(name, k, live=False):
    cut, t0, slow = (LIVE_CLIPS if live else CLIPS)[name][k]
    return dict(FLAGS[name], cut=cut, t0=t0, slow=slow)


def clip_of(B, n_clips, seed=20090216):
    """Chain b's clip: a fixed scramble (the same for every B up to its length)."""
    return np.random.default_rng(seed).integers(0, n_clips, BATCH_LIMIT)[:B]


def resident_raster_waves(hip_lib):
    """Waves of the raster kernels (amdgpu_waves_per_eu(2)) the device holds at once: CUs x 4 SIMDs x 2."""
    cus = hip_lib.x264hip_device_cus()
    assert cus > 0, hip_lib.x264hip_last_error().decode()
    return cus * 4 * 2


def run_full_batch(hip_lib, c, clips, owner, pipeline):
    """The StreamEncoder over len(owner) chains, chain b fed clips[owner[b]].  The distinct pictures are uploaded once per input number and fanned
    out on the device (x264hip_picture_copy_element).  Returns (per chain [(frame, slice type, qp, payload)], per chain frame_num restarts,
    per chain direct modes, per step (chains coded, slice types coded, chains that gave up an attempt)); run_full_batch.launches: per sweep the
    chains of its I / P and of its B chain-table launch."""
    B, frames = len(owner), c["frames"]
    enc = encoder_for(hip_lib, c, B, pipeline)
    try:
        stage = enc.src_ctx.new_picture(source_only=True)
        owner = [int(k) for k in owner]

        def fill(pic, f):
            for k, (y, u, v) in enumerate(clips):
                enc.src_ctx.upload(stage, y[f], u[f], v[f], b=k)
            for b, k in enumerate(owner):
                enc.src_ctx.copy_element(pic, b, stage, k)

        gave = []
        give_up = enc._give_up

        def counted_give_up(ci):
            gave.append(ci)
            give_up(ci)
        enc._give_up = counted_give_up
        launches = []                                   # per sweep: chains in its I / P chain-table launch, chains in its B launch
        sweep = enc._sweep

        def counted_sweep(frames_):
            out = sweep(frames_)
            n_b = sum(cd.slice_type == rs.SLICE_B for cd in out)
            launches.append((len(out) - n_b, n_b))
            return out
        enc._sweep = counted_sweep
        got = [[] for _ in range(B)]
        resets, direct, steps = [[] for _ in range(B)], [[] for _ in range(B)], []
        fed, idle = 0, 0
        for _ in range(4 * frames + 40):
            n_gave = len(gave)
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
                    resets[cd.chain].append(int(cd.frame_num_reset))
                    direct[cd.chain].append(int(cd.direct_spatial))
                steps.append((len(coded), {cd.slice_type for cd in coded}, len(set(gave[n_gave:]))))
        free, total = C.c_size_t(), C.c_size_t()
        hip_lib.x264hip_mem_info(C.byref(free), C.byref(total))
        run_full_batch.device_bytes = total.value - free.value        # what the device holds with the encoder still open
        run_full_batch.launches = launches
        return got, resets, direct, steps
    finally:
        enc.close()


def frame_nums(hip_lib, c, got, resets, a):
    """The frame_num every coded frame's slice header carries (the muxer's bookkeeping, as test_gpu_stream checks it against the reference)."""
    from x264_vs2008_amd import mux
    p = mux.encoder_params(hip_lib, width=c["w"], height=c["h"], rc_method=mux.RC_CQP, qp_constant=c["qp"], bframe=c["bframes"], keyint_max=c["keyint"])
    m = mux.AnnexB(hip_lib, p)
    out = []
    for f, ((frame, st, qp, payload), reset) in enumerate(zip(got, resets)):
        poc = int(a["frame_info"][f][3])                   # (the order and types are the reference's: check() has passed)
        ftype = (mux.TYPE_IDR if poc == 0 else mux.TYPE_I) if st == rs.SLICE_I else mux.TYPE_P if st == rs.SLICE_P else mux.TYPE_B
        m.frame(frame=frame, ftype=ftype, qp=qp, payload=payload, frame_num_reset=reset)
        out.append(m.frame_num - (0 if ftype == mux.TYPE_B else 1))
    return out


def full_batch(hip_lib, name, B, refs, what):
    """Runs flag set `name` over B chains and compares every chain with refs[clip] (the reference's records: frame_info, frame_info2, payload,
    payload_len, frame_num).  Prints the degeneracy guards' evidence; asserts them."""
    c0 = FLAGS[name]
    live = what == "live"
    cs = [case(name, k, live) for k in range(len(CLIPS[name]))]
    clips = [K.clip(c["w"], c["h"], c["frames"], c["cut"], c["t0"], c["slow"]) for c in cs]
    owner = clip_of(B, len(cs))
    # the scramble really mixes: the ends, both sides of the first wave generation and every group of 8 chains code more than one clip
    ends = [owner[b] for b in (0, B - 1, 2047, 2048) if b < B]
    assert len(set(ends)) > 1 and all(len(set(owner[g:g + 8])) > 1 for g in range(0, B - 1, 8)), "%s B=%d: the scramble leaves the ends or a group of 8 chains on one clip" % (name, B)
    assert np.bincount(owner, minlength=len(cs)).min() >= 100, "every clip is coded by at least 100 chains"
    t = time.perf_counter()
    got, resets, direct, steps = run_full_batch(hip_lib, c0, clips, owner, PIPELINE[name])
    spent = time.perf_counter() - t
    mixed = [i for i, (_, kinds, _) in enumerate(steps) if rs.SLICE_B in kinds and len(kinds) > 1]
    split = [i for i, (n, _, g) in enumerate(steps) if 0 < g < n]
    print("\n%s B=%d (%s): %.1f s, %.1f GB of device memory in use, %d steps; chains per step %s; steps with I/P and B chains in one table: %d; steps where some chains gave up an "
          "attempt and others did not: %d (%s chains); chains per raster launch (I/P, B) %s" % (name, B, what, spent, run_full_batch.device_bytes / 1e9, len(steps), [n for n, _, _ in steps], len(mixed), len(split),
                                                          [steps[i][2] for i in split], run_full_batch.launches))
    first = {}
    modes = set()
    for b in range(B):
        k = int(owner[b])
        a, c = refs[k], cs[k]
        label = "%s B=%d chain %d (clip %d, %s)" % (name, B, b, k, what)
        check(got[b], a, c, label)
        for f in range(c["frames"]):
            if int(a["frame_info"][f][0]) == rs.SLICE_B:
                modes.add(direct[b][f])
                assert direct[b][f] == int(a["frame_info2"][f][3]), "%s coded frame %d: direct mode %d, the reference %d" % (label, f, direct[b][f], int(a["frame_info2"][f][3]))
        if k not in first:                                  # frame_num of the first chain of every clip through the muxer against the reference's
            first[k] = b
            fn = frame_nums(hip_lib, c, got[b], resets[b], a)
            want = [int(x) for x in a["frame_num"][:c["frames"]]]
            assert fn == want, "%s: frame_num %s, the reference %s" % (label, fn, want)
        else:                                               # ... and every other chain of the clip restarts frame_num where that one does
            assert resets[b] == resets[first[k]], "%s: frame_num restarts %s, chain %d of the same clip %s" % (label, resets[b], first[k], resets[first[k]])
    # the guards: the batch did not degenerate into lock step
    assert mixed, "%s B=%d: no step had I/P and B chains in the same chain table" % (name, B)
    if name == "med":
        assert split, "%s B=%d: no step where some chains gave up an attempt and others did not" % (name, B)
    if B > BENCH_BATCH["med"]:
        resident = resident_raster_waves(hip_lib)
        widest = max(max(l) for l in run_full_batch.launches)
        print("%s B=%d: widest raster launch %d chains, %d raster waves resident" % (name, B, widest, resident))
        assert widest > resident, "%s B=%d: no raster launch had more chains than the %d resident raster waves" % (name, B, resident)
    if name == "slow":
        assert modes == {0, 1}, "%s B=%d: direct modes seen in B slice headers %s, both expected" % (name, B, sorted(modes))
    return spent


def load_fixture(name):
    with np.load(os.path.join(ROOT, "tests", "golden", "stream_batch_%s.npz" % name)) as z:
        return [{k: z["c%d_%s" % (i, k)] for k in ("frame_info", "frame_info2", "payload", "payload_len", "frame_num")} for i in range(len(CLIPS[name]))]


def reference(name, live=False):
    """The reference's whole encoder on every clip of the flag set (what oracle/gen_golden_stream.py stores)."""
    out = []
    for k in range(len(CLIPS[name])):
        a = K.reference_records(case(name, k, live))
        out.append(dict(frame_info=a["frame_info"], frame_info2=a["frame_info2"], payload=a["payload"], payload_len=a["payload_len"],
                        frame_num=a["look_cost"][:, 7].astype(np.int32)))
    return out


# ---- the lock-step sweeps ------------------------------------------------------------------------------------------------------------
# bench.py --stream 0: constant QP, the fixed B pattern (--bframes 3), B frames on lanes of their own (--lanes -1), the RD set with trellis
LOCK_RASTER = dict(w=112, h=96, frames=8, lanes=3,
                   kw=dict(qp=26, me_method=rs.ME_HEX, me_range=16, subme=7, n_refs=3, inter=0x113, intra=0x3, transform8x8=1, mixed_refs=1, cabac=1,
                           deblock=1, keyint=12, fast_pskip=1, dct_decimate=1, chroma_me=1),
                   ekw=dict(trellis=1, psy_rd=1.0, aq_mode=1, aq_strength=1.0, bframes=3, weightb=1, direct_pred=1))
# bench.py --preset cif: the UF flag set (--qp 26 --no-cabac --me dia --subme 0 --partitions none --no-deblock --ref 1, mv range 128), the
# wavefront variant, payloads from the CAVLC writer; 176x144 (11 x 9 macroblocks: 9 blocks per chain)
LOCK_WAVE = dict(w=176, h=144, frames=6, lanes=0,
                 kw=dict(qp=26, me_method=rs.ME_DIA, me_range=16, subme=0, n_refs=1, inter=0, intra=0x1, transform8x8=0, mixed_refs=0, cabac=0, deblock=0,
                         keyint=250, fast_pskip=1, dct_decimate=1, chroma_me=1, mv_range=128),
                 ekw=dict())
LOCK_T0 = [0, 13, 29, 47, 71, 101, 137, 173]       # the K clips: rs.clip from these frame numbers
LOCK_T0_LIVE = [t + 500 for t in LOCK_T0]


def lock_sample(B, n=64, seed=7):
    """The chains whose decisions and planes are compared: both ends, both sides of 2048, the last group of 8, and a seeded rest."""
    must = {0, 1, 7, 8, B - 1, B - 2, B - 8, 2046, 2047, 2048, 2049}
    rest = np.random.default_rng(seed).choice(B, n, replace=False)
    return sorted({b for b in must if 0 <= b < B} | {int(b) for b in rest})


def run_lockstep(hip_lib, cfg, clips, owner, sample):
    """ChainEncoder over len(owner) chains in lock step, chain b fed clips[owner[b]] (uploaded once, fanned out on the device).  Returns per frame in
    coding order: (slice type, qp), every chain's payload, the sample's decision arrays and its planes ("rec" of a B frame, "fin" of an anchor)."""
    w, h, frames, kw, ekw = cfg["w"], cfg["h"], cfg["frames"], cfg["kw"], cfg["ekw"]
    B = len(owner)
    enc = sl.ChainEncoder(hip_lib, w, h, cqm_init(hip_lib), batch=B, write=1, lanes=cfg["lanes"], **kw, **ekw)
    assert enc.raster == (cfg is LOCK_RASTER) and enc.cavlc == (cfg is LOCK_WAVE), "the encoder chose raster=%s cavlc=%s for this flag set" % (enc.raster, enc.cavlc)
    order = sl.coding_order(frames, kw["keyint"], ekw["bframes"]) if ekw.get("bframes") else [(t, None) for t in range(frames)]
    out = []
    try:
        stage = enc.ctx.new_picture(source_only=True)
        for disp, stype in order:
            for ln in enc.lanes:                       # a B frame still in flight on a lane may be reading the source picture
                ln["ctx"].sync()
            for k, (y, u, v) in enumerate(clips):
                enc.ctx.upload(stage, y[disp], u[disp], v[disp], b=k)
            fenc = enc.fenc
            for b, k in enumerate(owner):
                enc.ctx.copy_element(fenc, b, stage, int(k))
            st, qp, state = enc.encode_frame(stype=stype, disp=disp) if stype is not None else enc.encode_frame()
            enc.sync()
            enc.status()
            pays = enc.payloads()
            dec = {k: state.get(k)[sample] for k in STATE}
            recon = enc.last[0]
            enc.finish_frame()
            enc.sync()
            kind = "rec" if st == sl.SLICE_B else "fin"
            planes = {nm: np.stack([enc.ctx.download(recon, nm, padded=False, b=b) for b in sample]) for nm in ("y", "u", "v")}
            out.append(((st, qp), pays, dec, kind, planes))
        return out
    finally:
        enc.close()


def twin(oracle_lib, cfg, clip):
    """The CPU twin of the sweep on one clip: x264o_encode_chain2 (raster variant, payload included) or x264o_encode_chain (wavefront variant)."""
    p = rs.make_params(cfg["w"], cfg["h"], cfg["frames"], **cfg["kw"])
    if cfg is LOCK_RASTER:
        return rs.run2(oracle_lib, "x264o_encode_chain2", p, rs.make_ext(**cfg["ekw"]), *clip)
    return rs.run(oracle_lib, "x264o_encode_chain", p, *clip)


def cavlc_reference(cfg, clip):
    """slice_data() of every frame from the reference's own CAVLC writer inside its loop (as tests/test_gpu_cavlc.py)."""
    a = rs.run_reference2(rs.make_params(cfg["w"], cfg["h"], cfg["frames"], **cfg["kw"]), rs.make_ext(write=1), *clip)
    return dict(payload=a["payload"], payload_len=a["payload_len"])


def load_cavlc_fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "cavlc_batch_uf.npz")) as z:
        return [{k: z["c%d_%s" % (i, k)] for k in ("payload", "payload_len")} for i in range(len(LOCK_T0))]


def lockstep(hip_lib, oracle_lib, cfg, B, t0s, payload_refs, what):
    w, h, frames = cfg["w"], cfg["h"], cfg["frames"]
    clips = [rs.clip(w, h, frames, t0) for t0 in t0s]
    owner = clip_of(B, len(clips))
    assert np.bincount(owner, minlength=len(clips)).min() >= 100, "B=%d: every clip is coded by at least 100 chains" % B
    sample = lock_sample(B)
    assert len(sample) >= 64 and {0, B - 1, 2047} <= set(sample) and (B <= 2048 or 2048 in sample), "B=%d: the sample of chains misses an end or the first wave generation's end: %s" % (B, sample)
    twins = [twin(oracle_lib, cfg, c) for c in clips]
    t = time.perf_counter()
    out = run_lockstep(hip_lib, cfg, clips, owner, sample)
    spent = time.perf_counter() - t
    label = "%s B=%d" % ("raster" if cfg is LOCK_RASTER else "wavefront", B)
    print("\n%s (%s payloads): %.1f s; %d frames %s; every chain's payload, decisions and planes of %d chains (%s ... %s)" %
          (label, what, spent, len(out), "".join("PBI"[st] for (st, _), *_ in out), len(sample), sample[:4], [b for b in sample if 2040 <= b <= 2050] + sample[-3:]))
    for f, ((st, qp), pays, dec, kind, planes) in enumerate(out):
        for k, want in enumerate(twins):               # every clip's twin agrees on the frame's type and QP
            assert (st, qp) == (int(want["frame_info"][f][0]), int(want["frame_info"][f][1])), "%s frame %d: (slice, qp) %s, the twin's %s" % (label, f, (st, qp), tuple(want["frame_info"][f][:2]))
        for b in range(B):
            ref = payload_refs[owner[b]]
            want = bytes(ref["payload"][f, :int(ref["payload_len"][f])])
            assert pays[b] == want, "%s chain %d (clip %d) frame %d (%s): payload differs (%d vs %d bytes)" % (label, b, owner[b], f, "PBI"[st], len(pays[b]), len(want))
        for i, b in enumerate(sample):
            want = twins[owner[b]]
            for key in STATE:
                if st == sl.SLICE_I and key in ("mv", "ref"):
                    continue                           # (not written in an I slice: the pool picture's state keeps what it held)
                g, r = dec[key][i], want[key][f]
                assert np.array_equal(g.reshape(r.shape), r), "%s chain %d (clip %d) frame %d (%s): %s differs first at %s" % (
                    label, b, owner[b], f, "PBI"[st], key, np.argwhere(g.reshape(r.shape) != r)[:3].tolist())
            for nm in ("y", "u", "v"):
                g, r = planes[nm][i], want[kind + "_" + nm][f]
                assert np.array_equal(g, r), "%s chain %d (clip %d) frame %d (%s): %s_%s differs at %s" % (label, b, owner[b], f, "PBI"[st], kind, nm, np.argwhere(g != r)[:3].tolist())
    return spent
