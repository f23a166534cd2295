"""The cases of sub-8x8 P partitions under the RD levels (--partitions all with --subme 6..9; x264hip_slice_rd.mb_carry), shared by
tests/test_gpu_sub8_rd.py and tests/test_cpu_sub8_rd.py, and -- under __main__ -- the generator of their fixtures tests/golden/sub8rd_<name>.npz
from the REFERENCE's own loop and whole encoder (oracle/refslice.py: refslice_encode_chain2 / refslice_encode_stream; needs
oracle/_ref/libx264ref.so).

    python tests/sub8_rd_cases.py [name ...]

A fixture holds the reference's arrays of the case whole (the pictures are a few macroblocks).  One condition is checked on the REFERENCE's arrays
when a fixture is made and again by the tests from the stored data (condition_problems): over the P slices of a case at least 8 blocks of
P_8x8 macroblocks have a sub-partition below 8x8 -- smooth clips rarely pick one -- and over all cases each of 4x4, 8x4 and 4x8 occurs.  The
smallest pictures (the first macroblock of every frame reads what the previous frame left; a one-macroblock picture reads nothing else) are held
to the same count: moving noise over 13 frames.  Two cases have I_PCM macroblocks in front of P_8x8 macroblocks with sub-partitions (pcm_then_sub),
and the streams marked given_up have attempts the post-encode scene cut gives up.  B chains are not among the
cases: the sweep refuses a B slice of a chain with mb_carry."""
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import edge_cases as ec
from oracle import refslice as rs
from paths import GOLDEN

BASE = dict(me_method=rs.ME_HEX, n_refs=1, inter=0x33, intra=0x3, transform8x8=1, cabac=1, deblock=1)


def noisy_clip(w, h, n, amp, seed):
    """rs.clip with +-amp uniform noise on the luma samples: texture that moves with the clip's motion, which the small blocks follow."""
    y, u, v = rs.clip(w, h, n)
    r = np.random.default_rng(seed)
    y = np.clip(y.astype(np.int32) + r.integers(-amp, amp + 1, y.shape), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(y), u, v


def shift_clip(w, h, n, dx, seed):
    """Random content that moves dx luma samples to the left per frame (dx / 2 chroma samples)."""
    r = np.random.default_rng(seed)
    by = r.integers(0, 256, (h, w + dx * n), dtype=np.uint8)
    bu, bv = r.integers(0, 256, (2, h // 2, w // 2 + dx * n), dtype=np.uint8)
    y = np.stack([by[:, dx * t:dx * t + w] for t in range(n)])
    u = np.stack([bu[:, (dx // 2) * t:(dx // 2) * t + w // 2] for t in range(n)])
    v = np.stack([bv[:, (dx // 2) * t:(dx // 2) * t + w // 2] for t in range(n)])
    return tuple(np.ascontiguousarray(a) for a in (y, u, v))


def shift_noise_clip(w, h, n, dx, amp, seed):
    """shift_clip with +-amp fresh noise on every frame's luma: noise content that inter prediction can follow, block by block a little differently."""
    y, u, v = shift_clip(w, h, n, dx, seed)
    r = np.random.default_rng(seed + 1000)
    y = np.clip(y.astype(np.int32) + r.integers(-amp, amp + 1, y.shape), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(y), u, v


def cut_clip(w, h, n, cut, t0, amp, seed):
    """look_cases.clip (a hard cut at `cut`) with +-amp luma noise: what the post-encode scene cut gives a P attempt up for."""
    import look_cases as K
    y, u, v = K.clip(w, h, n, cut, t0, 1)
    r = np.random.default_rng(seed)
    y = np.clip(y.astype(np.int32) + r.integers(-amp, amp + 1, y.shape), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(y), u, v


def pcm_clip(w, h, n, amp, seed, col):
    """noisy_clip with macroblock column `col` replaced by fresh random samples in every frame: at a low QP without psy-rd those macroblocks are
    cheapest as I_PCM, in the middle of macroblocks that are coded inter."""
    y, u, v = noisy_clip(w, h, n, amp, seed)
    r = np.random.default_rng(seed + 500)
    y = y.copy()
    y[:, :, 16 * col:16 * col + 16] = r.integers(0, 256, (n, h, 16), dtype=np.uint8)
    return np.ascontiguousarray(y), u, v


def clip_of(c):
    (w, h), n, k = c["size"], c["frames"], c["clip"]
    return {"noisy": noisy_clip, "shift": shift_noise_clip, "cut": cut_clip, "pcm": pcm_clip}[k[0]](w, h, n, *k[1:])


# name: size, frames, clip, kw (x264hip / harness parameters), ext (harness extension; ChainEncoder takes the same keywords)
CHAINS = {
    # the RD choice of the sub-partitions alone (subme 6, 7) ...
    "s6_noisy": dict(size=(48, 32), frames=4, clip=("noisy", 12, 11), kw=dict(BASE, qp=18, subme=6), ext=dict()),
    "s7_noisy": dict(size=(48, 32), frames=4, clip=("noisy", 12, 12), kw=dict(BASE, qp=18, subme=7), ext=dict(psy_rd=1.0)),
    "s7_t1_aq": dict(size=(48, 32), frames=4, clip=("noisy", 16, 13), kw=dict(BASE, qp=18, subme=7), ext=dict(trellis=1, psy_rd=1.0, aq_mode=1, aq_strength=1.0)),
    "s7_t2_psy0": dict(size=(48, 32), frames=4, clip=("noisy", 12, 34), kw=dict(BASE, qp=17, subme=7), ext=dict(trellis=2, psy_rd=0.0)),
    "s6_mixed3": dict(size=(48, 32), frames=5, clip=("noisy", 12, 15), kw=dict(BASE, qp=18, subme=6, n_refs=3, mixed_refs=1), ext=dict(psy_rd=1.0)),
    "s7_umh_1ref": dict(size=(48, 32), frames=4, clip=("noisy", 12, 16), kw=dict(BASE, qp=18, subme=7, me_method=rs.ME_UMH), ext=dict(trellis=1, psy_rd=1.0)),
    "s7_nochroma_nodec": dict(size=(48, 32), frames=4, clip=("noisy", 12, 17), kw=dict(BASE, qp=18, subme=7, chroma_me=0, dct_decimate=0), ext=dict(psy_rd=1.0)),
    # ... with the refinement of the small blocks' vectors behind it (subme 8, 9)
    "s8_noisy": dict(size=(48, 32), frames=4, clip=("noisy", 12, 18), kw=dict(BASE, qp=18, subme=8), ext=dict(psy_rd=1.0)),
    "s8_t2_aq": dict(size=(48, 32), frames=4, clip=("noisy", 12, 19), kw=dict(BASE, qp=19, subme=8), ext=dict(trellis=2, psy_rd=1.0, aq_mode=1, aq_strength=1.0)),
    "s9_noisy": dict(size=(48, 32), frames=4, clip=("noisy", 12, 20), kw=dict(BASE, qp=18, subme=9), ext=dict(trellis=1, psy_rd=0.0)),
    "s9_mixed3_key3": dict(size=(48, 32), frames=5, clip=("noisy", 12, 21), kw=dict(BASE, qp=18, subme=9, n_refs=3, mixed_refs=1, keyint=3), ext=dict(psy_rd=1.0)),
    "s9_umh_nochroma_nodec": dict(size=(48, 32), frames=4, clip=("noisy", 12, 22), kw=dict(BASE, qp=19, subme=9, me_method=rs.ME_UMH, chroma_me=0, dct_decimate=0),
                                  ext=dict(trellis=1, psy_rd=1.0)),
    # psy-trellis: the refinement kind of k_psy_raster
    "s7_psyt_t1": dict(size=(48, 32), frames=4, clip=("noisy", 12, 23), kw=dict(BASE, qp=19, subme=7), ext=dict(trellis=1, psy_rd=1.0, psy_trellis=0.6)),
    "s6_psyt_t2": dict(size=(48, 32), frames=4, clip=("noisy", 12, 24), kw=dict(BASE, qp=19, subme=6), ext=dict(trellis=2, psy_rd=1.0, psy_trellis=1.0)),
    "s8_psyt_t2": dict(size=(48, 32), frames=4, clip=("noisy", 12, 25), kw=dict(BASE, qp=19, subme=8), ext=dict(trellis=2, psy_rd=0.4, psy_trellis=0.3)),
    # I_PCM (low QP, psy-rd off): the cache keeps the last trial's counts behind such a macroblock, and the macroblock after it starts its
    # partial trials from them (pcm: at least one I_PCM macroblock is followed by a P_8x8 macroblock with sub-partitions)
    "s7_pcm": dict(size=(80, 48), frames=5, clip=("pcm", 12, 4, 2), kw=dict(BASE, qp=8, subme=7), ext=dict(trellis=1, psy_rd=0.0), pcm=1),
    "s9_pcm": dict(size=(80, 48), frames=5, clip=("pcm", 12, 4, 2), kw=dict(BASE, qp=8, subme=9), ext=dict(trellis=1, psy_rd=0.0), pcm=1),
}
# one to six macroblocks of moving noise: 1x1, 2x1, 1x2, 3x2, 13 frames with an I frame every 6, so that so few macroblocks reach the count
# ((size, subme): shift per frame, fresh noise, QP, seed -- chosen with the reference until it held)
SMALL_SIZES = {((16, 16), 7): (4, 20, 20, 9), ((16, 16), 9): (2, 40, 24, 9), ((32, 16), 7): (4, 40, 20, 7), ((32, 16), 9): (4, 40, 20, 7),
               ((16, 32), 7): (2, 40, 28, 8), ((16, 32), 9): (4, 20, 20, 7), ((40, 24), 7): (2, 20, 20, 7), ((40, 24), 9): (2, 20, 20, 7)}
SMALL = {"small_%dx%d_s%d" % (s[0], s[1], sm): dict(size=s, frames=13, clip=("shift", dx, amp, seed), kw=dict(BASE, qp=qp, subme=sm, n_refs=2, keyint=6),
                                                    ext=dict(trellis=1, psy_rd=1.0))
         for (s, sm), (dx, amp, qp, seed) in SMALL_SIZES.items()}
CHAINS.update(SMALL)
# the whole encoder (CRF, no B frames, the default post-encode scene cut): x264_encoder_encode's queue in front of the loop.  given_up: the scene cut gives
# P attempts up (stat[:, 3]), and the I frame coded in their place inherits the attempt's leftovers
_ST = dict(crf=18.0, aq_mode=1, aq_strength=1.0, trellis=1, psy_rd=1.0, scenecut_threshold=40, pre_scenecut=0)
STREAMS = {
    "stream_cut_s7": dict(size=(80, 48), frames=8, clip=("cut", 4, 30, 12, 30), kw=dict(BASE, qp=26, subme=7, n_refs=2, keyint=250), ext=dict(_ST), given_up=1),
    "stream_cut_s8": dict(size=(80, 48), frames=8, clip=("cut", 4, 36, 12, 36), kw=dict(BASE, qp=26, subme=8, n_refs=2, keyint=250), ext=dict(_ST, crf=17.0), given_up=1),
    "stream_crf_s9": dict(size=(80, 48), frames=6, clip=("cut", 0, 32, 12, 32), kw=dict(BASE, qp=26, subme=9, n_refs=2, keyint=250), ext=dict(_ST, crf=19.0)),
}
ALL = list(CHAINS) + list(STREAMS)
MIN_BLOCKS = 8


def reference(name):
    """The reference's run of case `name`: its own loop with its writer (a chain) or its whole encoder (a stream)."""
    c = CHAINS.get(name) or STREAMS[name]
    p = rs.make_params(c["size"][0], c["size"][1], c["frames"], **c["kw"])
    e = rs.make_ext(write=1, **c["ext"])
    return (rs.run_reference2 if name in CHAINS else rs.run_reference_stream)(p, e, *clip_of(c))


def twin(lib, name):
    """The CPU twin (oracle/liboracle.so: x264o_encode_chain2) on chain case `name` (the twin has no frame queue: the stream cases pin the GPU alone)."""
    c = CHAINS[name]
    p = rs.make_params(c["size"][0], c["size"][1], c["frames"], **c["kw"])
    return rs.run2(lib, "x264o_encode_chain2", p, rs.make_ext(write=1, **c["ext"]), *clip_of(c))


def to_fixture(a):
    """What is compared and stored: everything but the harness's debugging aids and the arrays the reference leaves undefined."""
    from oracle.gen_golden_slice import masked2
    a = masked2(a)
    for k in ("qp_offset", "rc_info", "look_mv", "look_cost", "mv1", "ref1"):
        a.pop(k, None)
    return {k: np.ascontiguousarray(v) for k, v in a.items()}


def fixture_path(name):
    return os.path.join(GOLDEN, "sub8rd_%s.npz" % name)


def fixture(name):
    with np.load(fixture_path(name)) as z:
        return {k: z[k] for k in z.files}


def want(name):
    """What case `name` must give: from the live reference where oracle/_ref is built, from the fixture otherwise."""
    if ec.have_reference():
        return to_fixture(reference(name))
    return fixture(name)


def sub_blocks(x):
    """[4x4, 8x4, 4x8] blocks of P_8x8 macroblocks in the P slices of the reference's arrays x."""
    isp = x["frame_info"][:, 0] == rs.SLICE_P
    p8 = (x["mb_type"] == rs.P_8x8) & isp[:, None]
    sub = x["sub_partition"][p8]
    return [int((sub == t).sum()) for t in (0, 1, 2)]


def condition_problems(name, x):
    """What the reference's arrays `x` of case `name` fail to show: [] when the case proves what it is there for."""
    n = sum(sub_blocks(x))
    bad = [] if n >= MIN_BLOCKS else ["only %d blocks of P_8x8 macroblocks with a sub-partition below 8x8 in the P slices (at least %d)" % (n, MIN_BLOCKS)]
    if STREAMS.get(name, {}).get("given_up") and int(x["stat"][:, 3].sum()) < 1:
        bad.append("no given-up attempt")
    if CHAINS.get(name, {}).get("pcm") and pcm_then_sub(x) < 1:
        bad.append("no I_PCM macroblock followed by a P_8x8 macroblock with a sub-partition below 8x8")
    return bad


def pcm_then_sub(x):
    """I_PCM macroblocks whose successor in coding order (the next frame's first macroblock behind a frame's last) is a P_8x8 macroblock with a
    sub-partition below 8x8: its partial trial encodes start from what the I_PCM macroblock left in the cache, which is not the 16s of the frame's arrays."""
    t, sub = x["mb_type"].reshape(-1), x["sub_partition"].reshape(-1, 4)
    return int(((t[:-1] == rs.I_PCM) & (t[1:] == rs.P_8x8) & (sub[1:] != 3).any(1)).sum())


def write(name):
    x = to_fixture(reference(name))
    bad = condition_problems(name, x)
    assert not bad, "%s: %s" % (name, bad)
    np.savez_compressed(fixture_path(name), **x)
    return x


def main():
    tot = np.zeros(3, int)
    for name in sys.argv[1:] or ALL:
        x = write(name)
        tot += sub_blocks(x)
        print(name, "slices", x["frame_info"][:, 0].tolist(), "bytes", x["payload_len"].tolist(), "4x4 / 8x4 / 4x8 blocks", sub_blocks(x), "P_8x8",
              int((x["mb_type"] == rs.P_8x8).sum()), "file", os.path.getsize(fixture_path(name)))
    print("all: 4x4 / 8x4 / 4x8", tot.tolist())


if __name__ == "__main__":
    main()
