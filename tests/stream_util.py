"""Helpers of the stream tests (tests/test_gpu_stream.py and the tests built on it), the smoke run and oracle/gen_golden_stream.py: the
fixture configurations and their clips' seeds, seeded random configurations, and the drivers that put a batch of chains through the
StreamEncoder (run_stream) or the AsyncStreamEncoder (run_async) and hold a chain to the reference's records (check)."""
import numpy as np

import look_cases as K
from x264_vs2008_amd.frame import cqm_init
from x264_vs2008_amd.stream import StreamEncoder


def encoder_for(hip_lib, c, batch, pipeline=False):
    return StreamEncoder(hip_lib, c["w"], c["h"], cqm_init(hip_lib), batch=batch, n_frames=c["frames"] if pipeline else None, crf=c["crf"], b_adapt=c["b_adapt"], bframe_bias=c["bframe_bias"],
                         keyint_min=c["keyint_min"], scenecut_threshold=c["scenecut_threshold"], pre_scenecut=c["pre_scenecut"],
                         qp=c["qp"], me_method=c["me"], me_range=16, subme=c["subme"], n_refs=c.get("n_refs", 2), inter=c.get("inter", 0x33), intra=0x3,
                         transform8x8=1, cabac=1, deblock=1, keyint=c["keyint"], mixed_refs=c.get("mixed_refs", 0), chroma_me=c.get("chroma_me", 1),
                         trellis=c.get("trellis", 0), psy_rd=c.get("psy_rd", 0.0), aq_mode=c["aq"], aq_strength=1.0, bframes=c["bframes"],
                         weightb=c["weightb"], direct_pred=c.get("direct_pred", 1), qp_min=0)


def run_stream(hip_lib, cs, pipeline=False):
    """cs: the chains' configurations (one encoder configuration, different clips).  Returns per chain [(frame, slice type, qp, payload)].
    pipeline: the encoder is told how many pictures there are and prepares every next call's lookahead beside the sweep in flight."""
    c0, frames = cs[0], cs[0]["frames"]
    clips = [K.clip(c["w"], c["h"], frames, c["cut"], c["t0"], c["slow"]) for c in cs]
    enc = encoder_for(hip_lib, c0, len(cs), pipeline)
    got = [[] for _ in cs]
    run_stream.resets = [[] for _ in cs]               # per coded frame: the encoder says "scene-cut IDR: frame_num restarts" (Coded.frame_num_reset)
    run_stream.direct_spatial = [[] for _ in cs]       # ... and the direct mode a B slice's header carries

    def fill(pic, f):
        for b, (y, u, v) in enumerate(clips):
            enc.src_ctx.upload(pic, y[f], u[f], v[f], b=b)

    fed, idle = 0, 0
    for _ in range(4 * frames + 40):
        coded = enc.step(fill if fed < frames else None)
        fed += fed < frames
        idle = 0 if coded else idle + (fed >= frames and enc.flushing)
        if idle >= 2:                                    # (a clip shorter than the lookahead's delay is coded by the flush alone)
            break
        if coded:
            enc.sync()
            enc.status()
            pl = enc.payloads()
            for cd in coded:
                got[cd.chain].append((cd.frame, cd.slice_type, cd.qp, pl[cd.chain]))
                run_stream.resets[cd.chain].append(int(cd.frame_num_reset))
                run_stream.direct_spatial[cd.chain].append(int(cd.direct_spatial))
    enc.close()
    return got


def check(got, a, c, what):
    frames = c["frames"]
    assert len(got) == frames, "%s: %d frames coded, the reference codes %d" % (what, len(got), frames)
    for f, (frame, st, qp, payload) in enumerate(got):
        ref = (int(a["frame_info2"][f][0]), int(a["frame_info"][f][0]), int(a["frame_info"][f][1]))
        assert (frame, st, qp) == ref, "%s coded frame %d: (input, slice, qp) %s, the reference %s" % (what, f, (frame, st, qp), ref)
        want = bytes(a["payload"][f, :a["payload_len"][f]])
        assert payload == want, "%s coded frame %d (input %d, slice %d, qp %d): payload differs (%d vs %d bytes)" % (what, f, frame, st, qp, len(payload), len(want))


def run_async(hip_lib, cs, launches=3, drift=2):
    """The same through the AsyncStreamEncoder: every chain's frames as its own kernels finish.  Returns per chain [(frame, slice type, qp, payload)]."""
    import ctypes as C
    from x264_vs2008_amd.stream import AsyncStreamEncoder
    c0, frames = cs[0], cs[0]["frames"]
    clips = [K.clip(c["w"], c["h"], frames, c["cut"], c["t0"], c["slow"]) for c in cs]
    c = c0
    enc = AsyncStreamEncoder(hip_lib, c["w"], c["h"], cqm_init(hip_lib), batch=len(cs), n_frames=frames, launches=launches, drift=drift, crf=c["crf"],
                             b_adapt=c["b_adapt"], bframe_bias=c["bframe_bias"], keyint_min=c["keyint_min"], scenecut_threshold=c["scenecut_threshold"],
                             pre_scenecut=c["pre_scenecut"], qp=c["qp"], me_method=c["me"], me_range=16, subme=c["subme"], n_refs=c.get("n_refs", 2),
                             inter=c.get("inter", 0x33), intra=0x3, transform8x8=1, cabac=1, deblock=1, keyint=c["keyint"], mixed_refs=c.get("mixed_refs", 0),
                             chroma_me=c.get("chroma_me", 1), trellis=c.get("trellis", 0), psy_rd=c.get("psy_rd", 0.0), aq_mode=c["aq"], aq_strength=1.0,
                             bframes=c["bframes"], weightb=c["weightb"], direct_pred=c.get("direct_pred", 1), qp_min=0)
    cap = min(1 << 16, enc.payload_cap - 64)          # (PAYLOAD_LEAD bytes of every chain's slot precede the payload)
    pin = hip_lib.x264hip_host_alloc(len(cs) * frames * (cap + 64))
    recs = [[] for _ in cs]

    def fill(pic, f):
        for b, (y, u, v) in enumerate(clips):
            enc.src_ctx.upload(pic, y[f], u[f], v[f], b=b)

    def on_launch(coded, ctx, ev_b):
        for cd in coded:
            k = len(recs[cd.chain])
            base = pin + (cd.chain * frames + k) * (cap + 64)
            enc.payload_async_of(cd, k, ctx, ev_b, base, base + 64, cap)
            recs[cd.chain].append((cd.frame, cd.slice_type, cd.qp, base))

    enc.run(fill, on_launch)
    enc.status()
    got = [[(f, st, qp, C.string_at(base + 64, C.c_int32.from_address(base).value)) for f, st, qp, base in r] for r in recs]
    sizes = list(enc.launch_sizes)
    enc.close()
    hip_lib.x264hip_host_free(pin)
    return got, sizes


CONFIGS = {
    "badapt1_crf_aq": dict(w=128, h=96, frames=14, bframes=3, b_adapt=1, crf=23.0, subme=5, me=1, weightb=1, aq=1, n_refs=2),
    "badapt2_crf_rd": dict(w=112, h=96, frames=13, bframes=2, b_adapt=2, crf=28.0, subme=7, me=2, weightb=0, aq=0, n_refs=3, mixed_refs=1, trellis=1, inter=0x13),
    "scenecut_cqp": dict(w=96, h=80, frames=12, bframes=0, b_adapt=0, crf=None, subme=6, me=1, weightb=0, aq=1, keyint=8, inter=0x13),
    "temporal_crf": dict(w=128, h=80, frames=12, bframes=1, b_adapt=1, crf=20.0, subme=4, me=0, weightb=1, aq=0, direct_pred=2),
    # the reference's default scene cut (after the encode: given-up P pictures coded again, queues rearranged) and --direct auto: fixtures, so that
    # both are held to the reference where oracle/_ref is not built too
    "postsc_crf": dict(w=112, h=96, frames=13, bframes=2, b_adapt=1, crf=24.0, subme=5, me=1, weightb=1, aq=1, n_refs=2, inter=0x13, pre_scenecut=0),
    "direct_auto_crf": dict(w=128, h=96, frames=13, bframes=3, b_adapt=1, crf=22.0, subme=6, me=1, weightb=1, aq=0, n_refs=2, inter=0x113, direct_pred=3),
}
SEEDS = {"badapt1_crf_aq": [0, 3, 9], "badapt2_crf_rd": [4, 7], "scenecut_cqp": [5, 11, 12], "temporal_crf": [1, 6], "postsc_crf": [4, 13, 20], "direct_auto_crf": [3, 21]}
STEP_ONLY = {"postsc_crf", "direct_auto_crf"}          # (the step-less scheduler keeps neither the verdict loop nor the running scores)


def chains(name, seeds):
    cs = []
    for s in seeds:
        c = K.config(s)
        c.update(pre_scenecut=1, scenecut_threshold=40, keyint=250, keyint_min=0, bframe_bias=0, qp=26)
        c.update(CONFIGS[name])
        cs.append(c)
    return cs


def random_config(seed):
    """A seeded encoder configuration over what the stream path accepts, on top of look_cases.config's clip and lookahead options."""
    r = np.random.default_rng(91000 + seed)
    c = K.config(seed)
    subme = int(r.choice([2, 4, 5, 6, 7, 7, 8]))
    c.update(w=16 * int(r.integers(5, 10)), h=16 * int(r.integers(5, 8)), frames=int(r.integers(8, 13)), subme=subme,
             n_refs=int(r.integers(1, 4)), mixed_refs=int(r.random() < 0.5), inter=int(r.choice([0x13, 0x11, 0x10, 0x33])) if subme < 6 else int(r.choice([0x13, 0x11, 0x10])),
             trellis=int(r.choice([0, 1, 2])), psy_rd=float(r.choice([0.0, 1.0])), direct_pred=int(r.choice([1, 1, 2])), chroma_me=int(r.random() < 0.7),
             pre_scenecut=1, scenecut_threshold=int(r.choice([40, -1])), qp=int(r.integers(18, 36)))
    return c


def mixed_config(seed):
    """Two chains of a seeded configuration over round 3's additions on top of random_config: --direct auto / temporal / spatial, the post- or pre-encode scene
    cut (or none), B patterns fixed / b-adapt 1 / 2, clips with and without scene changes; and whether the encoder runs its lookahead ahead (pipeline)."""
    r = np.random.default_rng(77000 + seed)
    c = random_config(seed)
    c.update(pre_scenecut=int(r.random() < 0.4), scenecut_threshold=int(r.choice([40, 40, 60, -1])), direct_pred=int(r.choice([1, 2, 3, 3])),
             bframes=int(r.choice([0, 1, 2, 3])), b_adapt=int(r.choice([0, 1, 2])), cut=int(r.choice([0, 4, 7])))
    if c["bframes"] == 0:
        c["b_adapt"] = 0
    if c["subme"] == 8 and c["bframes"] and c["inter"] & 0x20:
        c["inter"] &= ~0x20
    cs = [dict(c), dict(c, t0=c["t0"] + 61, slow=1 + (c["slow"] % 3), cut=max(c["cut"] - 2, 0))]
    return cs, bool(r.random() < 0.5)
