"""The cases of --nr in B slices and under the post-encode scene cut, shared by tests/test_gpu_nr_b.py and tests/test_nr_b_cpu.py, and --
under __main__ -- the generator of their fixtures tests/golden/nr_b_<name>.npz from the REFERENCE's own loop and whole encoder
(oracle/refslice.py: refslice_encode_chain2 / refslice_encode_stream with noise_reduction set; needs oracle/_ref/libx264ref.so).

    python tests/nr_b_cases.py [name ...]

A fixture holds what a test needs without the reference: payload bytes, mb_type, qp, frame_info / frame_info2 whole, every larger array as
one md5 per frame (digest()), and the md5 of every frame's payload in the same run with noise_reduction = 0 (payload0_md5).  Two conditions
are checked when a fixture is made and again by the tests from the stored data: the reference's payload of at least one B frame differs from
its payload without --nr (otherwise the case says nothing about B slices), and a stream case that asks for it (given_up) has at least one
given-up attempt (stat[:, 3], which refslice_encode_stream counts)."""
import hashlib
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import edge_cases as ec
import look_cases as K
from oracle import refslice as rs
from oracle.gen_golden_slice import case_inputs
from paths import GOLDEN

SIZE = (96, 80)
CAB = dict(me_method=rs.ME_HEX, inter=0x113, intra=0x3, transform8x8=1, cabac=1, deblock=1)
# name: (x264hip / harness parameters, harness extension): the B paths --nr goes through
CONFIGS = {
    "s2": (dict(CAB, qp=28, subme=2, n_refs=2), dict(direct_pred=rs.DIRECT_SPATIAL)),
    "s5": (dict(CAB, qp=27, subme=5, n_refs=2), dict(direct_pred=rs.DIRECT_SPATIAL)),
    "s4_cavlc": (dict(CAB, qp=28, subme=4, n_refs=2, cabac=0), dict(direct_pred=rs.DIRECT_SPATIAL)),
    "rd6_t1": (dict(CAB, qp=27, subme=6, n_refs=2), dict(trellis=1, direct_pred=rs.DIRECT_SPATIAL)),
    "rd7_t1": (dict(CAB, qp=29, subme=7, n_refs=2), dict(trellis=1, direct_pred=rs.DIRECT_SPATIAL)),
    "rd8_psy_aq": (dict(CAB, qp=28, subme=8, n_refs=2), dict(psy_rd=1.0, aq_mode=1, aq_strength=1.0, direct_pred=rs.DIRECT_SPATIAL)),
    "weightb_temporal": (dict(CAB, qp=26, subme=5, n_refs=2), dict(weightb=1, direct_pred=rs.DIRECT_TEMPORAL)),
    "spatial_mixed_ref3": (dict(CAB, qp=30, subme=5, n_refs=3, mixed_refs=1), dict(direct_pred=rs.DIRECT_SPATIAL)),
}
# every configuration at both strengths: the weak one with one B frame between the anchors, the strong one with two; 7 frames, so that a B
# frame is coded with nonzero offsets and a later P frame with offsets a B frame has added to (the I frame adds nothing, the first P frame
# is coded with zero offsets)
LOCK = {}
for _n, (_kw, _e) in CONFIGS.items():
    LOCK["%s_nr60_b1" % _n] = dict(size=SIZE, frames=7, clip=("moving",), kw=dict(_kw, noise_reduction=60), ext=dict(_e, bframes=1))
    LOCK["%s_nr400_b2" % _n] = dict(size=SIZE, frames=7, clip=("moving",), kw=dict(_kw, noise_reduction=400), ext=dict(_e, bframes=2))
# one to six macroblocks (edge_cases.SIZES' 1x1, 2x1 and 3x2), flat and noise
SMALL_SIZES = [(16, 16), (32, 16), (40, 24)]
SMALL = {"small_%dx%d_%s" % (s[0], s[1], kind): dict(size=s, frames=5, clip=("edge", kind), kw=dict(CAB, qp=28, subme=5, n_refs=2, noise_reduction=80),
                                                      ext=dict(bframes=1, weightb=1, direct_pred=rs.DIRECT_SPATIAL))
         for s in SMALL_SIZES for kind in ("flat128", "noise")}
CHAINS = dict(LOCK, **SMALL)
CHAIN_DIGESTS = ("mv", "ref", "mv1", "ref1", "cbp", "t8", "partition", "sub_partition", "luma", "luma_dc", "chroma_dc", "chroma_ac",
                 "rec_y", "rec_u", "rec_v", "fin_y", "fin_u", "fin_v")
CHAIN_RAW = ("payload", "payload_len", "mb_type", "qp", "frame_info", "frame_info2")

# the whole encoder (look_cases.clip: a hard cut at `cut`); the sizes and lengths of the existing post-encode scene cut cases
_ST = dict(w=112, h=96, frames=13, bframes=2, b_adapt=1, crf=24.0, subme=5, me=rs.ME_HEX, weightb=1, aq=1, n_refs=2, inter=0x113, scenecut_threshold=40,
           keyint=250, keyint_min=0, bframe_bias=0, qp=26, cut=7, t0=31, slow=1, cabac=1, noise_reduction=100)
STREAMS = {
    "stream_pre": dict(_ST, pre_scenecut=1),
    "stream_post": dict(_ST, pre_scenecut=0, given_up=1),
    "stream_post_cavlc": dict(_ST, pre_scenecut=0, cabac=0, given_up=1),
}
STREAM_RAW = ("payload", "payload_len", "frame_info", "frame_info2", "stat")
# batch 2, chain 1 fed two pictures fewer than chain 0 (no fixture: every chain against its own single-stream run)
STAGGER = [dict(_ST, pre_scenecut=0, w=96, h=80, frames=13, t0=3, cut=6), dict(_ST, pre_scenecut=0, w=96, h=80, frames=11, t0=40, cut=0)]
# BASELINE's MED flag set (mux_cases.MED / ARGS["MED"]) and the command line's defaults, each with --nr 100, on the command-line tests' small clip
CLI = {
    "cli_med": dict(args="--crf 23 --ref 3 --bframes 3 --b-adapt 1 --me hex --subme 7 --8x8dct --partitions p8x8,b8x8,i8x8,i4x4 --trellis 1 --weightb --mixed-refs "
                         "--direct spatial --nr 100", w=176, h=96, frames=14, t0=0),
    "cli_default": dict(args="--nr 100 --crf 23 --bframes 2", w=176, h=96, frames=12, t0=40),
}
ALL = list(CHAINS) + list(STREAMS) + list(CLI)


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).digest()


def payload(a, f):
    return bytes(a["payload"][f, :int(a["payload_len"][f])])


def clip_of(c):
    (w, h), n = c["size"], c["frames"]
    return case_inputs((w, h), n, "moving") if c["clip"][0] == "moving" else ec.content(c["clip"][1], w, h, n)


def chain_reference(c, noise_reduction=None):
    """The reference's own loop with its writer on the case's clip (frames in coding order); noise_reduction: another strength (0: off)."""
    kw = c["kw"] if noise_reduction is None else dict(c["kw"], noise_reduction=noise_reduction)
    return rs.run_reference2(rs.make_params(c["size"][0], c["size"][1], c["frames"], **kw), rs.make_ext(write=1, **c["ext"]), *clip_of(c))


def per_frame_md5(a, k):
    return np.array([list(md5(a[k][f])) for f in range(a[k].shape[0])], np.uint8)


def payload_md5(a):
    return np.array([list(md5(np.frombuffer(payload(a, f), np.uint8))) for f in range(a["payload_len"].shape[0])], np.uint8)


def digest(a, stream=False, cavlc=False):
    """Harness output `a` -- or the same arrays read back from the GPU -- in the form that is compared and stored: the small arrays whole, a
    chain's large ones as one md5 per frame.  cavlc: the harness records the luma levels of an 8x8-transform macroblock incompletely under
    CAVLC (tests/cavlc_host_util.py: restore_8x8_levels), so those macroblocks' luma levels stay out of the digest on both sides; the payload
    bytes carry them."""
    raw = STREAM_RAW if stream else CHAIN_RAW
    out = {k: np.ascontiguousarray(a[k]) for k in raw}
    if not stream:
        if cavlc:
            a = dict(a, luma=np.where((a["t8"] == 1)[..., None], 0, a["luma"]).astype(np.int16))
        out.update({k + "_md5": per_frame_md5(a, k) for k in CHAIN_DIGESTS})
    return out


def is_cavlc(name):
    return name in CHAINS and not CHAINS[name]["kw"]["cabac"]


def expected(name, a, a0):
    """What the fixture of case `name` keeps: digest(a), and the md5 of every frame's payload in `a0`, the same run without --nr."""
    return dict(digest(a, name not in CHAINS, is_cavlc(name)), payload0_md5=payload_md5(a0))


def stream_params(c, noise_reduction=None):
    nr = c["noise_reduction"] if noise_reduction is None else noise_reduction
    p = rs.make_params(c["w"], c["h"], c["frames"], qp=c["qp"], me_method=c["me"], subme=c["subme"], n_refs=c["n_refs"], inter=c["inter"], intra=0x3,
                       transform8x8=1, cabac=c["cabac"], deblock=1, keyint=c["keyint"], noise_reduction=nr)
    e = rs.make_ext(bframes=c["bframes"], b_adapt=c["b_adapt"], pre_scenecut=c["pre_scenecut"], scenecut_threshold=c["scenecut_threshold"],
                    keyint_min=c["keyint_min"], crf=c["crf"], bframe_bias=c["bframe_bias"], weightb=c["weightb"], aq_mode=c["aq"], aq_strength=1.0,
                    direct_pred=c.get("direct_pred", 1))
    return p, e


def stream_clip(c):
    return K.clip(c["w"], c["h"], c["frames"], c["cut"], c["t0"], c["slow"])


def stream_reference(c, noise_reduction=None):
    """The reference's whole encoder (refslice_encode_stream) on the case's clip."""
    return rs.run_reference_stream(*stream_params(c, noise_reduction), *stream_clip(c))


def cli_params(c, lib=None):
    """The validated x264hip_encoder_params of the case's argument list (x264hip_validate_parameters is host code: the library is only
    opened, no device is needed)."""
    from x264_vs2008_amd import encode as E, lib as L, mux
    o = E.build_parser().parse_args(c["args"].split() + ["-o", "x", "in.y4m"])
    return mux.encoder_params(lib or L.open_library(), width=c["w"], height=c["h"], fps_num=25, fps_den=1, **E.param_fields(o))


def cli_reference(c, p, noise_reduction=None):
    """The reference's whole encoder with the validated parameters p on rs.clip from t0 (mux_cases.reference_med with --nr)."""
    g = lambda k: getattr(p, k)
    w, h, n = c["w"], c["h"], c["frames"]
    rp = rs.make_params(w, h, n, qp=g("qp_constant"), me_method=g("me_method"), me_range=g("me_range"), subme=g("subpel_refine"), n_refs=g("frame_reference"),
                        inter=g("inter"), intra=g("intra"), transform8x8=g("transform_8x8"), cabac=g("cabac"), deblock=g("deblocking_filter"), keyint=g("keyint_max"),
                        mixed_refs=g("mixed_references"), chroma_me=g("chroma_me"), mv_range=g("mv_range"),
                        noise_reduction=g("noise_reduction") if noise_reduction is None else noise_reduction)
    e = rs.make_ext(bframes=g("bframe"), b_adapt=g("bframe_adaptive"), pre_scenecut=g("pre_scenecut"), scenecut_threshold=g("scenecut_threshold"),
                    keyint_min=g("keyint_min"), crf=g("rf_constant"), bframe_bias=g("bframe_bias"), weightb=g("weighted_bipred"), aq_mode=g("aq_mode"),
                    aq_strength=g("aq_strength"), trellis=g("trellis"), psy_rd=g("psy_rd"), direct_pred=g("direct_mv_pred"))
    return rs.run_reference_stream(rp, e, *rs.clip(w, h, n, c["t0"]))


def reference(name):
    """(the reference's run of case `name`, the same without --nr)."""
    if name in CHAINS:
        return chain_reference(CHAINS[name]), chain_reference(CHAINS[name], 0)
    if name in STREAMS:
        return stream_reference(STREAMS[name]), stream_reference(STREAMS[name], 0)
    p = cli_params(CLI[name])
    return cli_reference(CLI[name], p), cli_reference(CLI[name], p, 0)


def want(name):
    """What case `name` must give: from the live reference where oracle/_ref is built, from the fixture otherwise."""
    if ec.have_reference():
        a, a0 = reference(name)
        return expected(name, a, a0)
    return fixture(name)


def fixture_path(name):
    return os.path.join(GOLDEN, "nr_b_%s.npz" % name)


def fixture(name):
    with np.load(fixture_path(name)) as z:
        return {k: z[k] for k in z.files}


def given_up(name):
    return int(STREAMS.get(name, {}).get("given_up", 0))


def condition_problems(name, x):
    """What the stored data `x` (expected()) of case `name` fails to show: [] when the case proves what it is there for."""
    bad = []
    isb = x["frame_info"][:, 0] == rs.SLICE_B
    mine = np.array([list(md5(np.frombuffer(bytes(x["payload"][f, :int(x["payload_len"][f])]), np.uint8))) for f in range(len(isb))], np.uint8)
    bites = (mine != x["payload0_md5"]).any(1)
    if name in SMALL:                                   # (there for the sizes: flat content has nothing to denoise, noise is coded intra)
        return bad
    if name in LOCK and not (bites & isb).any():
        bad.append("--nr changes no B frame's payload")
    if not isb.any() or not bites.any():
        bad.append("no B frame, or --nr changes no payload")
    if given_up(name) and int(x["stat"][:, 3].sum()) < 1:
        bad.append("no given-up attempt")
    return bad


def write(name):
    a, a0 = reference(name)
    x = expected(name, a, a0)
    bad = condition_problems(name, x)
    assert not bad, "%s: %s" % (name, bad)
    np.savez_compressed(fixture_path(name), **x)
    return x


def main():
    for name in sys.argv[1:] or ALL:
        x = write(name)
        print(name, "slices", x["frame_info"][:, 0].tolist(), "bytes", x["payload_len"].tolist(), "given up", int(x["stat"][:, 3].sum()) if "stat" in x else "-",
              "file", os.path.getsize(fixture_path(name)))


if __name__ == "__main__":
    main()
