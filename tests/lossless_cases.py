"""TEST INFRASTRUCTURE -- the lossless (--qp 0) chains of the raster-order sweep: the case list, the fixture layout and the generator.

The fixtures (tests/golden/ll_*.npz) come from the REFERENCE's own loop (oracle/refslice.py: run_reference2 / run_reference_stream with
qp = 0, where oracle/ref_slice.c switches h->mb.b_lossless on), so they can only be made where oracle/_ref/libx264ref.so exists:

    python tests/lossless_cases.py [name ...]

A fixture holds every decision array, every level and mb_bits whole; the payloads and the planes -- incompressible at QP 0 -- as
md5 digests per frame (the reconstruction of a lossless frame is its source, which the tests check on their own).
"""
import hashlib
import os
import sys

import numpy as np

from paths import GOLDEN, ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ME_HEX, ME_UMH = 1, 2
BASE = dict(qp=0, cabac=1, deblock=1, intra=0x3)
# (name, size, frames, clip kind, parameters): I and P slices in every chain (keyint restarts some), the CABAC writer in the loop
LL_CASES = [
    ("s2_hex_1ref", (176, 112), 3, "static", dict(BASE, subme=2, me_method=ME_HEX, n_refs=1, inter=0x13, transform8x8=0)),
    ("s5_sub8x8", (208, 144), 4, "moving", dict(BASE, subme=5, me_method=ME_HEX, n_refs=2, inter=0x33, transform8x8=1, mixed_refs=1)),
    ("s5_umh_nomix", (176, 112), 4, "static", dict(BASE, subme=5, me_method=ME_UMH, n_refs=3, inter=0x13, transform8x8=1, mixed_refs=0, keyint=3)),
    ("s6_med", (208, 144), 4, "moving", dict(BASE, subme=6, me_method=ME_HEX, n_refs=3, inter=0x13, transform8x8=1, mixed_refs=1)),
    ("s7_umh", (176, 112), 5, "static", dict(BASE, subme=7, me_method=ME_UMH, n_refs=2, inter=0x13, transform8x8=1, mixed_refs=0, keyint=3)),
    ("s7_no8x8", (208, 144), 3, "moving", dict(BASE, subme=7, me_method=ME_HEX, n_refs=1, inter=0x11, intra=0x1, transform8x8=0, chroma_me=0)),
    ("s8_med", (176, 112), 3, "moving", dict(BASE, subme=8, me_method=ME_HEX, n_refs=3, inter=0x13, transform8x8=1, mixed_refs=1)),
    ("s9_umh", (208, 144), 4, "static", dict(BASE, subme=9, me_method=ME_UMH, n_refs=2, inter=0x13, transform8x8=1, mixed_refs=1)),
]
LL_BY_NAME = {c[0]: c for c in LL_CASES}

WHOLE = ["mb_type", "partition", "sub_partition", "ref", "i4mode", "i16mode", "chroma_mode", "qp", "t8", "mv", "cbp", "nnz", "luma", "luma_dc",
         "chroma_dc", "chroma_ac", "mvr", "frame_info", "stat", "payload_len", "mb_bits"]
PLANES = ["rec_y", "rec_u", "rec_v", "fin_y", "fin_u", "fin_v"]


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def to_fixture(a):
    """What a fixture keeps of run_reference2's arrays (mvr already masked)."""
    fx = {k: a[k] for k in WHOLE}
    F = a["mb_type"].shape[0]
    fx["payload_md5"] = np.array([hashlib.md5(bytes(a["payload"][f, :int(a["payload_len"][f])])).hexdigest() for f in range(F)])
    for k in PLANES:
        fx[k + "_md5"] = np.array([md5(a[k][f]) for f in range(F)])
    return fx


def reference_chain_of(size, kw, y, u, v):
    """A chain of the given planes through the reference's loop, live (needs oracle/_ref/libx264ref.so)."""
    from oracle import refslice as rs
    from oracle.gen_golden_slice import masked
    return masked(rs.run_reference2(rs.make_params(size[0], size[1], y.shape[0], **kw), rs.make_ext(), y, u, v))


def reference_chain(size, frames, kind, kw):
    from oracle.gen_golden_slice import case_inputs
    return reference_chain_of(size, kw, *case_inputs(size, frames, kind))


# ---- streams: the frame queue (SAD lookahead, scene cut before or after the encode, constant QP 0 for every frame type) -----------------
# look_cases.config's fields; every clip has a real cut.  The fixture of a stream holds, per chain, what tests/golden/stream_*.npz hold
# with the payloads as md5, plus the lookahead's vectors and costs (look_mv, rc_info) as the reference's queue had them.
LL_STREAM = dict(bframes=0, b_adapt=0, crf=None, qp=0, me=ME_HEX, weightb=0, aq=0, n_refs=2, inter=0x13, mixed_refs=1, scenecut_threshold=40, keyint=250,
                 keyint_min=0, bframe_bias=0, slow=1)
LL_STREAMS = {
    "postsc": [dict(LL_STREAM, w=112, h=96, frames=10, subme=6, pre_scenecut=0, cut=4, t0=30), dict(LL_STREAM, w=112, h=96, frames=10, subme=6, pre_scenecut=0, cut=7, t0=200)],
    # (chain 0's cut is one x264_slicetype_decide's scene-cut test finds with SAD costs: an I picture in mid-stream)
    "presc": [dict(LL_STREAM, w=112, h=96, frames=10, subme=7, pre_scenecut=1, cut=3, t0=90, slow=2), dict(LL_STREAM, w=112, h=96, frames=10, subme=7, pre_scenecut=1, cut=5, t0=310)],
}
STREAM_KEYS = ("frame_info", "frame_info2", "payload_len", "look_mv", "rc_info", "stat", "look_cost")


def stream_fixture(a, frames):
    fx = {k: a[k][:frames] for k in STREAM_KEYS}
    fx["payload_md5"] = np.array([hashlib.md5(bytes(a["payload"][f, :int(a["payload_len"][f])])).hexdigest() for f in range(frames)])
    return fx


# ---- the command line: `--qp 0` and nothing else (the reference's defaults: subme 6, one reference, the post-encode scene cut at 40) ----
CLI_ARGS = "--qp 0"
CLI_CLIP = dict(w=176, h=96, n=6, t0=11)


def cli_params(lib, extra=()):
    """The validated parameters of the command line (x264hip_validate_parameters through mux.encoder_params): host code only."""
    from x264_vs2008_amd import encode as E
    from x264_vs2008_amd import mux
    o = E.build_parser().parse_args(CLI_ARGS.split() + list(extra) + ["-o", "x", "in.y4m"])
    return mux.encoder_params(lib, width=CLI_CLIP["w"], height=CLI_CLIP["h"], fps_num=25, fps_den=1, **E.param_fields(o))


def cli_reference(p):
    """The reference's whole encoder on the command line's clip with the validated parameters p (constant QP: no CRF)."""
    from oracle import refslice as rs
    c = CLI_CLIP
    y, u, v = rs.clip(c["w"], c["h"], c["n"], c["t0"])
    rp = rs.make_params(c["w"], c["h"], c["n"], qp=p.qp_constant, me_method=p.me_method, me_range=p.me_range, subme=p.subpel_refine, n_refs=p.frame_reference,
                        inter=p.inter, intra=p.intra, transform8x8=p.transform_8x8, cabac=p.cabac, deblock=p.deblocking_filter, keyint=p.keyint_max,
                        mixed_refs=p.mixed_references, chroma_me=p.chroma_me, mv_range=p.mv_range)
    e = rs.make_ext(bframes=p.bframe, b_adapt=p.bframe_adaptive, pre_scenecut=p.pre_scenecut, scenecut_threshold=p.scenecut_threshold, keyint_min=p.keyint_min,
                    crf=-1.0, aq_mode=p.aq_mode, trellis=p.trellis, psy_rd=p.psy_rd)
    return rs.run_reference_stream(rp, e, y, u, v)


def main():
    only = sys.argv[1:]
    for name, size, frames, kind, kw in LL_CASES:
        if only and name not in only:
            continue
        a = reference_chain(size, frames, kind, kw)
        path = os.path.join(GOLDEN, "ll_%s.npz" % name)
        np.savez_compressed(path, **to_fixture(a))
        types = [np.bincount(a["mb_type"][f], minlength=7).tolist() for f in range(frames)]
        print("%s: %d bytes, payload %s, t8 %s, types per frame (I4 I8 I16 PCM P P8 skip) %s"
              % (path, os.path.getsize(path), a["payload_len"].tolist(), a["t8"].sum(axis=1).tolist(), types))
        for nm in ("y", "u", "v"):          # lossless: what the reference reconstructs is what it was given
            assert np.array_equal(a["rec_" + nm], a["fin_" + nm])
    import look_cases as K
    for name, cs in LL_STREAMS.items():
        if only and name not in only:
            continue
        fx = {}
        for i, c in enumerate(cs):
            a = K.reference_records(c)
            fx.update({"c%d_%s" % (i, k): v for k, v in stream_fixture(a, c["frames"]).items()})
            print("stream %s chain %d: slice types %s, QPs %s, attempts given up %d, payload %s" % (name, i, a["frame_info"][:c["frames"], 0].tolist(),
                  sorted(set(a["frame_info"][:c["frames"], 1].tolist())), int(a["stat"][:c["frames"], 3].sum()), a["payload_len"][:c["frames"]].tolist()))
        path = os.path.join(GOLDEN, "ll_stream_%s.npz" % name)
        np.savez_compressed(path, **fx)
        print("%s: %d bytes" % (path, os.path.getsize(path)))
    if not only or "cli" in only:
        from x264_vs2008_amd import lib as L
        p = cli_params(L.open_library())
        assert p.d_lossless and p.qp_constant == 0
        a, n = cli_reference(p), CLI_CLIP["n"]
        assert int(a["stat"][:n, 3].sum()) == 0         # no attempt given up on this clip: the headers need no frame_num bookkeeping beyond the muxer's
        path = os.path.join(GOLDEN, "ll_cli.npz")
        np.savez_compressed(path, **{k: a[k][:n] for k in ("frame_info", "frame_info2", "payload", "payload_len")})
        print("%s: %d bytes, slice types %s, payload %s" % (path, os.path.getsize(path), a["frame_info"][:n, 0].tolist(), a["payload_len"][:n].tolist()))


if __name__ == "__main__":
    main()
