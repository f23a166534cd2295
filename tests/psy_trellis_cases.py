"""TEST INFRASTRUCTURE -- psy-trellis (--psy-rd A:B with B > 0 under --trellis 1 / 2) in the raster-order sweep: the case list, the fixture
layout and the generator.

The fixtures (tests/golden/pt_*.npz) come from the REFERENCE's own loop (oracle/refslice.py: run_reference2 / run_reference_stream with
make_ext(psy_trellis=...), which oracle/ref_slice.c hands to h->mb.i_psy_trellis), so they can only be made where
oracle/_ref/libx264ref.so exists:

    python tests/psy_trellis_cases.py [name ...]

A fixture holds every decision array, every level and mb_bits whole; the payloads and the planes as md5 digests per frame.  The generator
asserts what each case is there for, and that the levels differ from the same chain with the strength at 0 (a kernel that ignores the
strength cannot pass).
"""
import hashlib
import os
import sys

import numpy as np

from paths import GOLDEN, ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SLICE_P, SLICE_B, SLICE_I = 0, 1, 2
I_16x16 = 2
CLI_T0 = 30          # the clip of the stream / command-line tests: synth frames CLI_T0 .. (chosen so that I, P and B slices all occur)
MED = dict(cabac=1, deblock=1, intra=3, me_method=1, inter=0x113, transform8x8=1, mixed_refs=1)
# (name, size, frames, clip kind, parameters, ext parameters): I and P slices in every chain, B slices in four
PT_CASES = [
    ("t1_s7", (96, 80), 4, "moving", dict(MED, qp=26, subme=7, n_refs=2), dict(trellis=1, psy_rd=1.0, psy_trellis=1.0)),
    ("t2_s7", (96, 80), 3, "moving", dict(MED, qp=24, subme=7, n_refs=2), dict(trellis=2, psy_rd=1.0, psy_trellis=1.0)),            # both arrays, the RD trials
    ("t2_s6_no8x8", (80, 80), 4, "moving", dict(MED, qp=30, subme=6, n_refs=1, transform8x8=0), dict(trellis=2, psy_rd=0.0, psy_trellis=1.0)),   # I_16x16 in P frames: the AC path with idx
    ("t1_s5", (96, 80), 4, "moving", dict(MED, qp=28, subme=5, n_refs=2), dict(trellis=1, psy_trellis=1.0)),                        # below the RD levels
    ("t2_s5", (96, 80), 4, "moving", dict(MED, qp=28, subme=5, n_refs=2), dict(trellis=2, psy_trellis=1.0)),                        # the arrays nobody writes: zeros
    ("t2_s8", (96, 80), 3, "moving", dict(MED, qp=26, subme=8, n_refs=2), dict(trellis=2, psy_rd=1.0, psy_trellis=1.0)),            # the refinement kernel
    ("t1_s7_b", (96, 80), 5, "moving", dict(MED, qp=26, subme=7, n_refs=2), dict(trellis=1, psy_rd=1.0, psy_trellis=1.0, bframes=2, weightb=1)),      # the B kernel
    ("t2_s7_bt", (96, 80), 5, "moving", dict(MED, qp=26, subme=7, n_refs=2), dict(trellis=2, psy_rd=1.0, psy_trellis=1.0, bframes=1, direct_pred=2)),  # the extended B kernel
    ("t1_s7_aq_weak", (96, 80), 4, "static", dict(MED, qp=26, subme=7, n_refs=2), dict(trellis=1, psy_rd=1.0, psy_trellis=0.15, aq_mode=1)),          # the < 0.25 chroma shift
    # beyond the nine: the trellis-2 twins of two trellis-1 cases (lock-step B launch with spatial direct prediction and weights; the weak strength with AQ) ...
    ("t2_s7_b", (96, 80), 5, "moving", dict(MED, qp=26, subme=7, n_refs=2), dict(trellis=2, psy_rd=1.0, psy_trellis=1.0, bframes=2, weightb=1)),
    ("t2_s7_aq_weak", (96, 80), 4, "static", dict(MED, qp=26, subme=7, n_refs=2), dict(trellis=2, psy_rd=1.0, psy_trellis=0.15, aq_mode=1)),
    # ... trellis 1 with the RD refinement: x264_rd_cost_i8x8 leaves h->mb.b_transform_8x8 set (R/encoder/rdo.c:249), so a refined I_8x8 macroblock refreshes
    # and reads the 8x8 array of its own source, unlike the I_8x8 macroblocks of t1_s7 ...
    ("t1_s8", (96, 80), 3, "moving", dict(MED, qp=26, subme=8, n_refs=2), dict(trellis=1, psy_rd=1.0, psy_trellis=1.0)),
    # ... and trellis 2 at subme 6 with B frames: the B slices are below the RD levels, the I and P slices are not, so a B macroblock is quantised against
    # the source transform of the LAST macroblock the frame coded before it analysed (x264_mb_cache_fenc_satd is the only writer)
    ("t2_s6_b", (96, 80), 5, "moving", dict(MED, qp=26, subme=6, n_refs=2), dict(trellis=2, psy_rd=1.0, psy_trellis=1.0, bframes=2, weightb=1)),
]
PT_BY_NAME = {c[0]: c for c in PT_CASES}
# With trellis 1 the reference refreshes, after the analysis, only the transform size h->mb.b_transform_8x8 names at that moment
# (R/encoder/analyse.c:2770-2771), and the flag turns 1 for an I_8x8 macroblock only in x264_macroblock_encode (macroblock.c:533): its blocks are quantised
# against the 8x8 array an EARLIER macroblock or frame left (zeros in a chain's first I frame).  Every trellis-1 case has I_8x8 macroblocks (asserted below).
I_8x8 = 1

WHOLE = ["mb_type", "partition", "sub_partition", "ref", "i4mode", "i16mode", "chroma_mode", "qp", "t8", "mv", "cbp", "nnz", "luma", "luma_dc",
         "chroma_dc", "chroma_ac", "mvr", "frame_info", "frame_info2", "stat", "payload_len", "mb_bits", "mv1", "ref1"]
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


def fixture_path(name):
    return os.path.join(GOLDEN, "pt_%s.npz" % name)


def load(name):
    with np.load(fixture_path(name)) as z:
        return {k: z[k] for k in z.files}


def reference_chain_of(size, kw, ekw, y, u, v):
    """A chain of the given planes through the reference's loop, live (needs oracle/_ref/libx264ref.so)."""
    from oracle import refslice as rs
    from oracle.gen_golden_slice import masked
    return masked(rs.run_reference2(rs.make_params(size[0], size[1], y.shape[0], **kw), rs.make_ext(**ekw), y, u, v))


def reference_chain(size, frames, kind, kw, ekw):
    from oracle.gen_golden_slice import case_inputs
    return reference_chain_of(size, kw, ekw, *case_inputs(size, frames, kind))


# ---- x264_validate_parameters' psy-trellis lines (R/encoder/encoder.c:502-522), restated for the tests that hold the encoders to them ----
def fix8(f):
    """FIX8 of a C float expression's value."""
    return int(float(np.float32(f)) * 256 + 0.5)


def validated(trellis, cabac, subme, psy_rd, psy_trellis, chroma_qp_offset=0):
    """(h->mb.i_psy_trellis, i_chroma_qp_offset) after x264_validate_parameters."""
    if not cabac:
        trellis = 0                                            # :493-494
    off = min(max(chroma_qp_offset, -12), 12)                  # :498
    if subme < 6:
        psy_rd = 0.0                                           # :499-500
    psy_rd = min(max(psy_rd, 0.0), 10.0)
    if not trellis:
        psy_trellis = 0.0                                      # :502-503
    psy_trellis = min(max(psy_trellis, 0.0), 10.0)             # :505
    if fix8(psy_rd):
        off -= 1 if np.float32(psy_rd) < 0.25 else 2           # :509-514
    i_psy_trellis = fix8(np.float32(psy_trellis) / np.float32(4))      # :515
    if i_psy_trellis:
        off -= 1 if np.float32(psy_trellis) < 0.25 else 2      # :517-518
    return i_psy_trellis, min(max(off, -12), 12)               # :521


# ---- one stream through the frame queue (StreamEncoder), and the same clip through the command line ----
# 112x96, 10 frames: CRF 23, adaptive B placement, weighted B prediction, adaptive quantisation, trellis 1 at the default subme, --psy-rd 1.0:0.15
CLI_ARGS = "--crf 23 --bframes 2 --b-adapt 1 --weightb --aq-mode 1 --trellis 1 --psy-rd 1.0:0.15"
CLI_CLIP = dict(w=112, h=96, n=10, t0=CLI_T0)
STREAM_KEYS = ("frame_info", "frame_info2", "payload", "payload_len")


def cli_params(lib, args=CLI_ARGS, extra=()):
    """The validated parameters of the command line (x264hip_validate_parameters through mux.encoder_params): host code only."""
    from x264_vs2008_amd import encode as E
    from x264_vs2008_amd import mux
    o = E.build_parser().parse_args(args.split() + list(extra) + ["-o", "x", "in.y4m"])
    return mux.encoder_params(lib, width=CLI_CLIP["w"], height=CLI_CLIP["h"], fps_num=25, fps_den=1, **E.param_fields(o))


def cli_reference(p, t0=None):
    """The reference's whole encoder on the command line's clip with the validated parameters p."""
    from oracle import refslice as rs
    c = CLI_CLIP
    y, u, v = rs.clip(c["w"], c["h"], c["n"], c["t0"] if t0 is None else t0)
    rp = rs.make_params(c["w"], c["h"], c["n"], qp=p.qp_constant, me_method=p.me_method, me_range=p.me_range, subme=p.subpel_refine, n_refs=p.frame_reference,
                        inter=p.inter, intra=p.intra, transform8x8=p.transform_8x8, cabac=p.cabac, deblock=p.deblocking_filter, keyint=p.keyint_max,
                        mixed_refs=p.mixed_references, chroma_me=p.chroma_me, mv_range=p.mv_range)
    e = rs.make_ext(bframes=p.bframe, b_adapt=p.bframe_adaptive, pre_scenecut=p.pre_scenecut, scenecut_threshold=p.scenecut_threshold, keyint_min=p.keyint_min,
                    crf=p.rf_constant, bframe_bias=p.bframe_bias, weightb=p.weighted_bipred, aq_mode=p.aq_mode, aq_strength=p.aq_strength, trellis=p.trellis,
                    psy_rd=p.psy_rd, psy_trellis=p.psy_trellis, direct_pred=p.direct_mv_pred)
    return rs.run_reference_stream(rp, e, y, u, v)


def main():
    only = sys.argv[1:]
    for name, size, frames, kind, kw, ekw in PT_CASES:
        if only and name not in only:
            continue
        a = reference_chain(size, frames, kind, kw, ekw)
        off = reference_chain(size, frames, kind, kw, dict(ekw, psy_trellis=0.0))
        path = fixture_path(name)
        np.savez_compressed(path, **to_fixture(a))
        stypes = a["frame_info"][:, 0].tolist()
        changed = [int((a["luma"][f] != off["luma"][f]).sum()) for f in range(frames)]
        types = [np.bincount(a["mb_type"][f], minlength=19).tolist() for f in range(frames)]
        print("%s: %d bytes, slice types %s, payload %s, t8 %s, luma levels changed by the strength %s, types per frame %s"
              % (path, os.path.getsize(path), stypes, a["payload_len"].tolist(), a["t8"].sum(axis=1).tolist(), changed, types))
        assert SLICE_I in stypes and SLICE_P in stypes and ((SLICE_B in stypes) == bool(ekw.get("bframes")))
        assert min(changed) > 0, "a frame whose levels the strength does not change"
        if kw["transform8x8"]:
            assert a["t8"].any()
        if ekw["trellis"] == 1 and kw["transform8x8"]:
            assert (a["mb_type"][0] == I_8x8).any(), "no I_8x8 macroblock in the I frame"
        if name == "t2_s6_no8x8":
            assert any((a["mb_type"][f] == I_16x16).any() for f in range(frames) if stypes[f] == SLICE_P), "no I_16x16 in a P frame"
        assert os.path.getsize(path) < (1 << 20)
    if not only or "stream" in only:
        from x264_vs2008_amd import lib as L
        p = cli_params(L.open_library())
        assert p.trellis == 1 and abs(p.psy_trellis - 0.15) < 1e-6 and p.bframe == 2
        a, n = cli_reference(p), CLI_CLIP["n"]
        stypes = a["frame_info"][:n, 0].tolist()
        assert SLICE_I in stypes and SLICE_P in stypes and SLICE_B in stypes, stypes
        off = cli_reference(cli_params(L.open_library(), CLI_ARGS.replace("1.0:0.15", "1.0:0")))
        assert any(bytes(a["payload"][f, :a["payload_len"][f]]) != bytes(off["payload"][f, :off["payload_len"][f]]) for f in range(n))
        path = fixture_path("stream")
        np.savez_compressed(path, **{k: a[k][:n] for k in STREAM_KEYS})
        print("%s: %d bytes, slice types %s, QPs %s, payload %s" % (path, os.path.getsize(path), stypes, a["frame_info"][:n, 1].tolist(), a["payload_len"][:n].tolist()))


if __name__ == "__main__":
    main()
