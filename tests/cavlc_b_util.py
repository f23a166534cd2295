"""Helpers of tests/test_gpu_cavlc_b.py and tests/test_gpu_cavlc_stream.py: the `--no-cabac` configurations with B frames, the reference's
own loop on them (oracle/ref_slice.c with cabac = 0: x264_macroblock_write_cavlc inside x264_slice_write's loop), which branches of the
B syntax the reference's decisions reach, and the stream encoder built without CABAC."""
import look_cases as K
from oracle import refslice as rs
from oracle.gen_golden_slice import case_inputs
from x264_vs2008_amd.frame import cqm_init
from x264_vs2008_amd.stream import StreamEncoder

B_DIRECT, B_L0_L0, B_L1_L1, B_BI_BI, B_8x8, B_SKIP = 7, 8, 12, 16, 17, 18      # R/common/macroblock.h:78-102
D_DIRECT_8x8, D_16x8, D_8x16, D_16x16 = 12, 14, 15, 16

# name: (size, frames, clip kind, x264hip / harness parameters, harness extension)
B_CASES = {
    # spatial direct, weighted bi-prediction, 8x8 transform, --ref 3 (7 frames hold two anchors before the last B frames: te() as one bit)
    "spatial_w_t8_ref3": ((96, 80), 7, "moving", dict(qp=24, me_method=rs.ME_HEX, subme=5, n_refs=3, inter=0x113, intra=0x3, transform8x8=1, mixed_refs=1, cabac=0, deblock=1),
                          dict(bframes=2, weightb=1, direct_pred=rs.DIRECT_SPATIAL)),
    # temporal direct, no weights, 4x4 transform only, one reference (no ref_idx at all), odd size
    "temporal_ref1": ((88, 72), 7, "moving", dict(qp=29, me_method=rs.ME_DIA, subme=2, n_refs=1, inter=0x111, intra=0x1, cabac=0, deblock=1),
                      dict(bframes=3, weightb=0, direct_pred=rs.DIRECT_TEMPORAL)),
    # adaptive quantisation: mb_qp_delta in every slice type; two references (te() as one bit)
    "aq_ref2": ((96, 80), 7, "moving", dict(qp=27, me_method=rs.ME_UMH, subme=5, n_refs=2, inter=0x133, intra=0x3, transform8x8=1, cabac=0, deblock=1),
                dict(bframes=2, weightb=1, direct_pred=rs.DIRECT_SPATIAL, aq_mode=1, aq_strength=1.3)),
    # high QP on a static clip: long skip runs, B_DIRECT without coefficients turned B_SKIP, a trailing run
    "high_qp_static": ((88, 72), 7, "static", dict(qp=41, me_method=rs.ME_HEX, subme=2, n_refs=2, inter=0x113, intra=0x3, transform8x8=1, cabac=0, deblock=1),
                       dict(bframes=3, weightb=1, direct_pred=rs.DIRECT_TEMPORAL)),
    # low QP: intra macroblocks in B slices, B_DIRECT with coefficients
    "low_qp": ((96, 80), 7, "moving", dict(qp=16, me_method=rs.ME_HEX, subme=5, n_refs=2, inter=0x113, intra=0x3, transform8x8=1, cabac=0, deblock=0),
               dict(bframes=3, weightb=0, direct_pred=rs.DIRECT_SPATIAL)),
    # ten frames, so that a P frame and the B frames behind it see three list-0 references: te() as ue(v)
    "ref3_long": ((96, 80), 10, "moving", dict(qp=30, me_method=rs.ME_HEX, subme=2, n_refs=3, inter=0x113, intra=0x3, transform8x8=1, mixed_refs=1, cabac=0, deblock=1),
                  dict(bframes=2, weightb=0, direct_pred=rs.DIRECT_SPATIAL)),
}

_ref_cache = {}


def reference(name):
    """The clip and the reference loop's arrays for a case (frames in coding order), computed once per session and left unchanged."""
    if name not in _ref_cache:
        size, frames, kind, kw, ekw = B_CASES[name]
        y, u, v = case_inputs(size, frames, kind)
        a = rs.run_reference2(rs.make_params(size[0], size[1], frames, **kw), rs.make_ext(write=1, **ekw), y, u, v)
        for arr in a.values():
            arr.setflags(write=False)
        _ref_cache[name] = ((y, u, v), a)
    return _ref_cache[name]


def coverage(a):
    """Which branches of the B-slice syntax the decisions in harness output `a` reach: {branch: count}."""
    isb = a["frame_info"][:, 0] == rs.SLICE_B
    t, part, sub, cbp, t8 = (a[k][isb] for k in ("mb_type", "partition", "sub_partition", "cbp", "t8"))
    two = (t > B_L0_L0) & (t < B_BI_BI) & (t != B_L1_L1)             # the list combinations whose halves differ
    direct_sub = (sub == D_DIRECT_8x8).sum(-1)
    return {
        "B_SKIP": int((t == B_SKIP).sum()),
        "B_DIRECT with coefficients": int(((t == B_DIRECT) & ((cbp & 0x3f) != 0)).sum()),
        "16x16 from L0": int(((t == B_L0_L0) & (part == D_16x16)).sum()),
        "16x16 from L1": int(((t == B_L1_L1) & (part == D_16x16)).sum()),
        "16x16 from BI": int(((t == B_BI_BI) & (part == D_16x16)).sum()),
        "16x8 with halves from different lists": int((two & (part == D_16x8)).sum()),
        "8x16 with halves from different lists": int((two & (part == D_8x16)).sum()),
        "B_8x8 with direct and non-direct sub-blocks": int(((t == B_8x8) & (direct_sub > 0) & (direct_sub < 4)).sum()),
        "intra macroblock in a B slice": int((t <= 2).sum()),
        "transform_size_8x8_flag = 1 in an inter B macroblock": int(((t >= B_DIRECT) & (t <= B_8x8) & (t8 == 1) & ((cbp & 15) != 0)).sum()),
    }


# ---- streams: --no-cabac through the frame queue (look_cases.clip / stream_util's records) -------------------------------------------------
STREAMS = {
    # the default (post-encode) scene cut on a clip with a scene change: the P picture at the cut is given up and coded again
    "crf_postsc": dict(w=96, h=80, frames=13, bframes=0, b_adapt=0, crf=23.0, subme=5, me=rs.ME_HEX, weightb=0, aq=1, n_refs=2, inter=0x113, pre_scenecut=0,
                       scenecut_threshold=40, keyint=250, keyint_min=0, bframe_bias=0, qp=26, cut=6, t0=31, slow=1),
    "crf_badapt1_direct_auto": dict(w=96, h=80, frames=14, bframes=3, b_adapt=1, crf=23.0, subme=5, me=rs.ME_HEX, weightb=1, aq=1, n_refs=2, inter=0x113, pre_scenecut=0,
                                    scenecut_threshold=40, keyint=250, keyint_min=0, bframe_bias=0, qp=26, cut=7, t0=5, slow=3, direct_pred=3),
}


def stream_reference(c):
    """look_cases.reference_records with cabac = 0."""
    p = rs.make_params(c["w"], c["h"], c["frames"], qp=c["qp"], me_method=c["me"], subme=c["subme"], n_refs=c["n_refs"], inter=c["inter"],
                       intra=0x3, transform8x8=1, cabac=0, deblock=1, keyint=c["keyint"])
    e = rs.make_ext(bframes=c["bframes"], b_adapt=c["b_adapt"], pre_scenecut=c["pre_scenecut"], scenecut_threshold=c["scenecut_threshold"],
                    keyint_min=c["keyint_min"], crf=c["crf"], bframe_bias=c["bframe_bias"], weightb=c["weightb"], aq_mode=c["aq"], aq_strength=1.0,
                    direct_pred=c.get("direct_pred", 1))
    y, u, v = K.clip(c["w"], c["h"], c["frames"], c["cut"], c["t0"], c["slow"])
    return rs.run_reference_stream(p, e, y, u, v)


def run_cavlc_stream(hip_lib, c, pipeline=False):
    """One chain through the StreamEncoder with cabac = 0: [(input frame, slice type, qp, payload)] in coding order, and the encoder's count
    of given-up attempts."""
    y, u, v = K.clip(c["w"], c["h"], c["frames"], c["cut"], c["t0"], c["slow"])
    frames = c["frames"]
    enc = StreamEncoder(hip_lib, c["w"], c["h"], cqm_init(hip_lib), batch=1, n_frames=frames if pipeline else None, crf=c["crf"], b_adapt=c["b_adapt"],
                        bframe_bias=c["bframe_bias"], keyint_min=c["keyint_min"], scenecut_threshold=c["scenecut_threshold"], pre_scenecut=c["pre_scenecut"],
                        qp=c["qp"], me_method=c["me"], me_range=16, subme=c["subme"], n_refs=c["n_refs"], inter=c["inter"], intra=0x3, transform8x8=1, cabac=0,
                        deblock=1, keyint=c["keyint"], aq_mode=c["aq"], aq_strength=1.0, bframes=c["bframes"], weightb=c["weightb"],
                        direct_pred=c.get("direct_pred", 1), qp_min=0)
    got, spatial = [], []

    def fill(pic, f):
        enc.src_ctx.upload(pic, y[f], u[f], v[f], b=0)

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
                    got.append((cd.frame, cd.slice_type, cd.qp, pl[cd.chain]))
                    spatial.append(int(cd.direct_spatial))
        given_up = enc.n_given_up
    finally:
        enc.close()
    return got, spatial, given_up
