"""Helpers of tests/test_gpu_cavlc.py and of oracle/gen_golden_cavlc.py, which writes its fixtures: the chains' configurations, the
reference's CAVLC writer on a configuration's clip, and the product's payloads for it."""
from oracle import refslice as rs
from x264_vs2008_amd import slice as sl
from x264_vs2008_amd.frame import cqm_init

CONFIGS = {
    "uf_cif": dict(w=352, h=288, n=6, kw=dict(qp=26, me_method=rs.ME_DIA, subme=0, n_refs=1, inter=0, intra=0, cabac=0, deblock=0, chroma_me=1)),
    "p_all_partitions": dict(w=208, h=144, n=6, kw=dict(qp=27, me_method=rs.ME_HEX, subme=5, n_refs=3, inter=0x33, intra=0x3, transform8x8=1, mixed_refs=1,
                                                       cabac=0, deblock=1)),
    "p_no_sub8x8_umh": dict(w=176, h=144, n=5, kw=dict(qp=31, me_method=rs.ME_UMH, subme=4, n_refs=2, inter=0x13, intra=0x3, transform8x8=1, cabac=0, deblock=1)),
    "intra_low_qp": dict(w=144, h=112, n=4, kw=dict(qp=12, me_method=rs.ME_HEX, subme=2, n_refs=1, inter=0x11, intra=0x3, transform8x8=1, cabac=0, deblock=1, keyint=2)),
    "high_qp_skips": dict(w=192, h=128, n=6, kw=dict(qp=40, me_method=rs.ME_HEX, subme=3, n_refs=2, inter=0x11, intra=0x1, cabac=0, deblock=1)),
    # adaptive quantisation: the raster variant without its writer leaves each macroblock's final QP (x264_macroblock_cache_save's rules and
    # cavlc_qp_delta's empty-I_16x16 one) in the state, the pass codes mb_qp_delta from it
    "aq_p_partitions": dict(w=208, h=144, n=6, ext=dict(aq_mode=1, aq_strength=1.0),
                            kw=dict(qp=28, me_method=rs.ME_HEX, subme=5, n_refs=2, inter=0x33, intra=0x3, transform8x8=1, mixed_refs=1, cabac=0, deblock=1)),
    "aq_strong_high_qp": dict(w=192, h=128, n=6, ext=dict(aq_mode=1, aq_strength=1.8),
                              kw=dict(qp=38, me_method=rs.ME_UMH, subme=3, n_refs=1, inter=0x11, intra=0x3, cabac=0, deblock=1, keyint=4)),
    "aq_intra_qp_clip": dict(w=144, h=112, n=4, ext=dict(aq_mode=1, aq_strength=2.5),
                             kw=dict(qp=47, me_method=rs.ME_HEX, subme=1, n_refs=1, inter=0x11, intra=0x3, transform8x8=1, cabac=0, deblock=1, keyint=2)),
}
# tests/edge_cases.py's chains at QP 1 (level codes in the extended escape, both profiles' arms) that tests/test_cavlc_host.py runs through the
# host-compiled writer: every content at the smallest size, the size with padding in both directions and the largest
QP1_CONFIGS = ("cavlc_qp1_high", "cavlc_qp1_base")
QP1_SIZES = ((16, 16), (24, 24), (40, 24))


def reference(c, t0=0):
    y, u, v = rs.clip(c["w"], c["h"], c["n"], t0)
    a = rs.run_reference2(rs.make_params(c["w"], c["h"], c["n"], **c["kw"]), rs.make_ext(write=1, **c.get("ext", {})), y, u, v)
    return (y, u, v), [bytes(a["payload"][f, :a["payload_len"][f]]) for f in range(c["n"])], a


def encode(hip_lib, c, clip):
    y, u, v = clip
    enc = sl.ChainEncoder(hip_lib, c["w"], c["h"], cqm_init(hip_lib), write=1, **c["kw"], **c.get("ext", {}))
    assert enc.cavlc and enc.raster == ("ext" in c), "the encoder chose cavlc=%s raster=%s for %s" % (enc.cavlc, enc.raster, c)
    out = []
    try:
        for f in range(c["n"]):
            enc.upload(y[f], u[f], v[f])
            enc.encode_frame()
            enc.status()
            out.append(enc.payloads()[0])
            enc.finish_frame()
    finally:
        enc.close()
    return out
