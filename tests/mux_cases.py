"""BASELINE's configurations as the stream writer's and the command line's tests use them (and the smoke run, and
oracle/gen_golden_ref_offline.py): the flag sets of BASELINE.md 2 as encoder parameters, as x264_param_parse pairs (CLI) and as command
lines (ARGS), the md5 of the reference CLI's .264 (--threads 1), the synthetic clips in memory and as files, the product's
streams for the flag sets, and the reference-side runs (oracle/_ref) that give the payloads."""
import ctypes as C
import hashlib

from paths import REF_SO
from x264_vs2008_amd import mux, slice as sl, synth
from x264_vs2008_amd.frame import cqm_init

CLIP_MD5 = {"cif30": "a5ce9660cf16d66830d27bbfbf69545a", "hd24": "0c526ccaa572e26ba82832ba43d303d1", "uhd8": "f8f0fa654f79120b17dc2dfb11956e98"}
STREAM_MD5 = {"C1_UF_cif30": "02b208eecef842e084cbb9c83bc1a757", "C2_MED_hd24": "b0d54145534a5158d08c9f5fc06db5da",
              "C3_MED_umh_uhd8": "81eb4c4af687d83cc5d9ffb190f5b52c",
              "C4_SLOW_hd24": "77215ac697eac797265f81fc43fd007a", "C4_SLOW_pre_scenecut_hd24": "f0c9914d4e8f730b776206dd50aceb75"}

# UF  = --qp 26 --no-cabac --me dia --subme 0 --partitions none --no-deblock --aq-mode 0 --scenecut -1 --ref 1 --bframes 0 --b-adapt 0
#       (`--partitions none` clears param.analyse.inter only: analyse.intra keeps I4x4, I8x8 goes with 8x8dct off, encoder.c:483-487)
UF = dict(rc_method=mux.RC_CQP, qp_constant=26, cabac=0, me_method=0, subpel_refine=0, inter=0, deblocking_filter=0, aq_mode=0, scenecut_threshold=-1,
          frame_reference=1, bframe=0, bframe_adaptive=0)
# MED = --crf 23 --ref 3 --bframes 3 --b-adapt 1 --me hex --subme 7 --8x8dct --partitions p8x8,b8x8,i8x8,i4x4 --trellis 1 --weightb --mixed-refs --direct spatial
MED = dict(rc_method=mux.RC_CRF, rf_constant=23.0, frame_reference=3, bframe=3, bframe_adaptive=1, me_method=1, subpel_refine=7, transform_8x8=1, inter=0x113, intra=3,
           trellis=1, weighted_bipred=1, mixed_references=1, direct_mv_pred=1)
# SLOW = --crf 23 --ref 5 --bframes 3 --b-adapt 2 --me umh --subme 8 --8x8dct --partitions p8x8,b8x8,i8x8,i4x4 --trellis 1 --weightb --mixed-refs --direct auto
SLOW = dict(rc_method=mux.RC_CRF, rf_constant=23.0, frame_reference=5, bframe=3, bframe_adaptive=2, me_method=2, subpel_refine=8, transform_8x8=1, inter=0x113, intra=3,
            trellis=1, weighted_bipred=1, mixed_references=1, direct_mv_pred=3)


def clip_md5(w, h, n):
    m = hashlib.md5()
    for t in range(n):
        for pl in synth.frame(w, h, t):
            m.update(pl.tobytes())
    return m.hexdigest()


def reference_uf(w, h, n):
    from oracle import refslice as rs
    y, u, v = rs.clip(w, h, n)
    return rs.run_reference2(rs.make_params(w, h, n, qp=26, me_method=rs.ME_DIA, subme=0, n_refs=1, inter=0, intra=1, cabac=0, deblock=0, chroma_me=1, keyint=250,
                                            mv_range=128), rs.make_ext(write=1), y, u, v)


def reference_med(p, w, h, n, t0=0):
    """The reference's whole encoder (oracle/ref_slice.c refslice_encode_stream) with the validated parameters p -- the post-encode scene cut
    included (BASELINE's runs have it: no --pre-scenecut; it never fires on those clips)."""
    from oracle import refslice as rs
    y, u, v = rs.clip(w, h, n, t0)
    rp = rs.make_params(w, h, n, qp=p.qp_constant, me_method=p.me_method, me_range=p.me_range, subme=p.subpel_refine, n_refs=p.frame_reference, inter=p.inter,
                        intra=p.intra, transform8x8=p.transform_8x8, cabac=p.cabac, deblock=p.deblocking_filter, keyint=p.keyint_max, mixed_refs=p.mixed_references,
                        chroma_me=p.chroma_me, mv_range=p.mv_range)
    e = rs.make_ext(bframes=p.bframe, b_adapt=p.bframe_adaptive, pre_scenecut=p.pre_scenecut, scenecut_threshold=p.scenecut_threshold, keyint_min=p.keyint_min, crf=p.rf_constant,
                    bframe_bias=p.bframe_bias, weightb=p.weighted_bipred, aq_mode=p.aq_mode, aq_strength=p.aq_strength, trellis=p.trellis, psy_rd=p.psy_rd,
                    direct_pred=p.direct_mv_pred)
    return rs.run_reference_stream(rp, e, y, u, v)


def mux_reference_stream(lib, p, a, n):
    """The Annex B stream around the harness output `a` (coded order: input number, slice type, QP, POC, payload)."""
    m, out = mux.AnnexB(lib, p), []
    for f in range(n):
        st, qp, _, poc = (int(x) for x in a["frame_info"][f])
        ft = (mux.TYPE_IDR if poc == 0 else mux.TYPE_I) if st == 2 else mux.TYPE_P if st == 0 else mux.TYPE_B
        out.append(m.frame(frame=int(a["frame_info2"][f][0]), ftype=ft, qp=qp, payload=bytes(a["payload"][f, :a["payload_len"][f]]),
                           direct_spatial=int(a["frame_info2"][f][3]) if st == 1 else 1))       # (B slices: sh.b_direct_spatial_mv_pred as the harness recorded it)
    return b"".join(out)


def clip(w, h, n):
    fr = [synth.frame(w, h, t) for t in range(n)]
    m = hashlib.md5()
    for y, u, v in fr:
        m.update(y.tobytes()); m.update(u.tobytes()); m.update(v.tobytes())
    return fr, m.hexdigest()


def write_clip(path, w, h, n, t0=0, y4m=False):
    with open(path, "wb") as f:
        if y4m:
            f.write(b"YUV4MPEG2 W%d H%d F25:1 Ip A0:0 C420jpeg\n" % (w, h))
        for t in range(n):
            if y4m:
                f.write(b"FRAME\n")
            for pl in synth.frame(w, h, t0 + t):
                f.write(pl.tobytes())


def uf_stream(hip_lib, frames, w=352, h=288):
    """BASELINE's UF flag set (UF above) through the product: ChainEncoder (wavefront variant + the CAVLC pass) + the muxer."""
    p = mux.encoder_params(hip_lib, width=w, height=h, **UF)
    assert (p.level_idc, p.mv_range, p.intra, p.d_profile_idc) == (13, 128, 1, 66), "UF validated to (level, mv range, intra, profile) %s" % ((p.level_idc, p.mv_range, p.intra, p.d_profile_idc),)
    enc = sl.ChainEncoder(hip_lib, w, h, cqm_init(hip_lib), qp=p.qp_constant, me_method=p.me_method, me_range=p.me_range, subme=p.subpel_refine,
                          n_refs=p.frame_reference, inter=p.inter, intra=p.intra, transform8x8=p.transform_8x8, fast_pskip=p.fast_pskip,
                          dct_decimate=p.dct_decimate, chroma_me=p.chroma_me, cabac=0, deblock=p.deblocking_filter, keyint=p.keyint_max,
                          mv_range=p.mv_range, write=1)
    assert enc.cavlc, "the UF flag set did not select the CAVLC pass"
    m, out = mux.AnnexB(hip_lib, p), []
    try:
        for t, (y, u, v) in enumerate(frames):
            enc.upload(y, u, v)
            stype, qp, _ = enc.encode_frame()
            enc.status()
            pay = enc.payloads()[0]
            enc.finish_frame()
            out.append(m.frame(frame=t, ftype=mux.TYPE_IDR if stype == sl.SLICE_I else mux.TYPE_P, qp=qp, payload=pay))
    finally:
        enc.close()
    return out


def med_stream(hip_lib, p, w, h, n, pre_scenecut=0):
    """BASELINE's MED flag set through the product: StreamEncoder (lookahead, b-adapt 1, CRF, the sweep with the entropy coder) + the muxer.
    pre_scenecut = 0 is the CLI's default: the post-encode scene cut is evaluated after every P frame (it must not fire: the re-encode is not built)."""
    from x264_vs2008_amd.stream import StreamEncoder
    enc = StreamEncoder(hip_lib, w, h, cqm_init(hip_lib), batch=1, n_frames=n, crf=p.rf_constant, b_adapt=p.bframe_adaptive, bframe_bias=p.bframe_bias,
                        keyint_min=p.keyint_min, scenecut_threshold=p.scenecut_threshold, pre_scenecut=pre_scenecut, ip_factor=p.ip_factor, pb_factor=p.pb_factor,
                        qcompress=p.qcompress, qp_step=p.qp_step, qp=p.qp_constant, me_method=p.me_method, me_range=p.me_range, subme=p.subpel_refine,
                        n_refs=p.frame_reference, inter=p.inter, intra=p.intra, transform8x8=p.transform_8x8, cabac=1, deblock=p.deblocking_filter,
                        alpha_c0=p.deblocking_filter_alphac0, beta=p.deblocking_filter_beta, keyint=p.keyint_max, mixed_refs=p.mixed_references, chroma_me=p.chroma_me,
                        trellis=p.trellis, psy_rd=p.psy_rd, aq_mode=p.aq_mode, aq_strength=p.aq_strength, bframes=p.bframe, weightb=p.weighted_bipred,
                        direct_pred=p.direct_mv_pred, qp_min=p.qp_min, qp_max=p.qp_max, mv_range=p.mv_range, fast_pskip=p.fast_pskip, dct_decimate=p.dct_decimate)
    m, out, order = mux.AnnexB(hip_lib, p), [], []

    def fill(pic, f):
        y, u, v = synth.frame(w, h, f)
        enc.src_ctx.upload(pic, y, u, v, b=0)

    try:
        idle = 0
        while idle < 2 and len(out) < n:
            coded = enc.step(fill)
            idle = 0 if coded else idle + bool(enc.flushing)
            if coded:
                enc.sync()
                enc.status()
                cd = coded[0]
                out.append(m.frame(frame=cd.frame, ftype=cd.type, qp=cd.qp, payload=enc.payloads()[0], n_ref0=cd.n_ref0, n_ref1=cd.n_ref1, frame_num_reset=cd.frame_num_reset,
                                   direct_spatial=cd.direct_spatial))
                order.append((cd.frame, cd.type, cd.qp))
    finally:
        enc.close()
    return out, order


# the flag sets as (name, value) pairs for the reference's x264_param_parse, and as command lines for x264_vs2008_amd.encode
CLI = {
    "UF": [("qp", "26"), ("no-cabac", None), ("me", "dia"), ("subme", "0"), ("partitions", "none"), ("no-deblock", None), ("aq-mode", "0"), ("scenecut", "-1"),
           ("ref", "1"), ("bframes", "0"), ("b-adapt", "0")],
    "MED": [("crf", "23"), ("ref", "3"), ("bframes", "3"), ("b-adapt", "1"), ("me", "hex"), ("subme", "7"), ("8x8dct", None), ("partitions", "p8x8,b8x8,i8x8,i4x4"),
            ("trellis", "1"), ("weightb", None), ("mixed-refs", None), ("direct", "spatial")],
    "SLOW": [("crf", "23"), ("ref", "5"), ("bframes", "3"), ("b-adapt", "2"), ("me", "umh"), ("subme", "8"), ("8x8dct", None), ("partitions", "p8x8,b8x8,i8x8,i4x4"),
             ("trellis", "1"), ("weightb", None), ("mixed-refs", None), ("direct", "auto"), ("pre-scenecut", None)],
    "misc": [("qp", "31"), ("ref", "4"), ("bframes", "2"), ("b-bias", "10"), ("me", "esa"), ("merange", "24"), ("subme", "9"), ("psy-rd", "0.4:0.2"), ("trellis", "2"),
             ("deblock", "-1:2"), ("nr", "100"), ("cqm", "jvt"), ("chroma-qp-offset", "3"), ("keyint", "48"), ("min-keyint", "6"), ("scenecut", "30"), ("ipratio", "1.2"),
             ("pbratio", "1.5"), ("no-chroma-me", None), ("no-dct-decimate", None), ("deadzone-inter", "12"), ("deadzone-intra", "7")],
    "crf_misc": [("crf", "18.5"), ("qcomp", "0.75"), ("qpmin", "12"), ("qpmax", "44"), ("qpstep", "6"), ("aq-strength", "0.7"), ("bframes", "1"), ("no-cabac", None)],
}
ARGS = {
    "UF": "--qp 26 --no-cabac --me dia --subme 0 --partitions none --no-deblock --aq-mode 0 --scenecut -1 --ref 1 --bframes 0 --b-adapt 0",
    "MED": "--crf 23 --ref 3 --bframes 3 --b-adapt 1 --me hex --subme 7 --8x8dct --partitions p8x8,b8x8,i8x8,i4x4 --trellis 1 --weightb --mixed-refs --direct spatial",
    "SLOW": "--crf 23 --ref 5 --bframes 3 --b-adapt 2 --me umh --subme 8 --8x8dct --partitions p8x8,b8x8,i8x8,i4x4 --trellis 1 --weightb --mixed-refs --direct auto --pre-scenecut",
    "misc": "--qp 31 --ref 4 --bframes 2 --b-bias 10 --me esa --merange 24 --subme 9 --psy-rd 0.4:0.2 --trellis 2 --deblock=-1:2 --nr 100 --cqm jvt --chroma-qp-offset 3 "
            "--keyint 48 --min-keyint 6 --scenecut 30 --ipratio 1.2 --pbratio 1.5 --no-chroma-me --no-dct-decimate --deadzone-inter 12 --deadzone-intra 7 --partitions all",
    "crf_misc": "--crf 18.5 --qcomp 0.75 --qpmin 12 --qpmax 44 --qpstep 6 --aq-strength 0.7 --bframes 1 --no-cabac --no-fast-pskip --deblock 2 --psy-rd 0.8 --direct temporal",
}


def reference_string(args):
    from oracle import hostpic
    ref = hostpic.load_lazy(REF_SO)
    ref.x264_param2string.restype = C.c_void_p
    buf = C.create_string_buffer(16384)
    ref.x264_param_default(buf)
    toks = args.split()
    i = 0
    while i < len(toks):
        name = toks[i][2:]
        val = None
        if "=" in name:
            name, val = name.split("=", 1)
        elif i + 1 < len(toks) and not toks[i + 1].startswith("--"):
            val = toks[i + 1]
            i += 1
        i += 1
        assert ref.x264_param_parse(buf, name.encode(), None if val is None else val.encode()) == 0, (name, val)
    return C.string_at(ref.x264_param2string(buf, 0)).decode()
