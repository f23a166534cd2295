"""TEST INFRASTRUCTURE -- pictures of one to six macroblocks with flat, saturated and full-range content: the case list shared by
oracle/gen_golden_edge.py (the reference's side, tests/golden/edge_chains.npz), tests/test_oracle_edge_chains.py (twin == reference),
tests/test_gpu_edge_chains.py, tests/test_gpu_edge_frames.py and tests/test_gpu_edge_table.py (kernel == twin / fixture).

The library accepts any picture from 16x16 upwards.  At these sizes mb_w x mb_h is 1x1, 2x1, 1x2, 3x1, 1x3, 2x2 (24x24: 8 padded columns and
rows, 18x18: 14) and 3x2: with one row no macroblock has a top neighbour, with one column none has a left or a top-right one, every search
candidate of a 16-pixel picture lies in the padding, and the padding of every plane is wider than the picture.  synth.frame cannot make
such pictures (its moving box needs more than 64 pixels), so content() is the generator.

A configuration names where its expected values come from:
  "twin"   x264o_encode_chain2 with the CABAC writer in the loop (pinned to the reference by tests/test_oracle_edge_chains.py),
  "plain"  x264o_encode_chain, no writer: the wavefront variant of the sweep, whose rows wait on each other,
  "ref"    the reference's own loop as recorded in tests/golden/edge_chains.npz (what the twin does not code: CAVLC payloads, lossless
           above subme 5).

Lossy QP 0..7 and escape-range levels are covered by the LOW_QP configurations: QP 1 (cavlc_qp1_high, cavlc_qp1_base, cavlc_b_qp1, s5_qp1,
rd9_t2_qp1, b_temporal_qp1, plain_s5_qp1), QP 2 under strong adaptive quantisation (cavlc_aq_qp2, rd7_aq_qp2, rd8_b_aq_qp2) and --cqm jvt
at QP 6 (jvt_qp6), plus the chain table's second QP assignment TABLE_LOW_QPS (1, 2, 3).  Their I slices (iframe_qp(1..3) = 0) and their
lowest adaptive-quantisation macroblocks are at QP 0 in a chain that is not lossless; levels reach 2967 under CAVLC (level codes >= 4096:
the High profile's growing prefix in cavlc_qp1_high, the Baseline clamp in cavlc_qp1_base), 3277 and more under CABAC, 3679 with the JVT
matrices; rd9_t2_qp1 chooses I_PCM at every size.  low_qp_problems() asserts all that, on the reference in the generator and on the twin in
tests/test_oracle_edge_chains.py; the fixture keeps each such chain's largest |level| (<name>_max_level), which writer_branch() turns into
the writer branch a failing chain was in."""
import ctypes as C
import functools
import hashlib
import os

import numpy as np

from oracle import refslice as rs
from paths import GOLDEN, REF_SO, ROOT
from x264_vs2008_amd import slice as sl

SIZES = [(16, 16), (32, 16), (16, 32), (48, 16), (16, 48), (24, 24), (18, 18), (40, 24)]
CONTENTS = ["flat0", "flat128", "flat255", "checker", "flip", "vstripe", "ramp", "noise", "satnoise"]
FIXTURE = os.path.join(GOLDEN, "edge_chains.npz")

# sweep_tables.h: the kernel kinds of a sweep
SW_KIND_PLAIN, SW_KIND_RD, SW_KIND_RF, SW_KIND_LL, SW_KIND_LL_RF, SW_KIND_B, SW_KIND_BT = range(7)


def seed_of(kind, w, h):
    """The seed of a random content kind: a fixed integer function of (kind index, width, height)."""
    return 7919 * CONTENTS.index(kind) + 131 * w + h + 20261


def content(kind, w, h, n):
    """n frames of content `kind`: (y [n][h][w], u, v [n][h/2][w/2]) uint8.  Chroma is luma's even / odd samples, v inverted."""
    r = np.random.default_rng(seed_of(kind, w, h))
    yy, xx = np.mgrid[0:h, 0:w]
    if kind.startswith("flat"):
        y = np.full((n, h, w), int(kind[4:]), np.uint8)
    elif kind == "checker":
        y = np.stack([(((xx + yy + t) & 1) * 255).astype(np.uint8) for t in range(n)])
    elif kind == "flip":
        y = np.stack([np.full((h, w), 255 * (t & 1), np.uint8) for t in range(n)])
    elif kind == "vstripe":
        y = np.stack([((((xx + 3 * t) // 4) & 1) * 255).astype(np.uint8) for t in range(n)])
    elif kind == "ramp":
        y = np.stack([((7 * xx + 5 * yy + 11 * t) & 255).astype(np.uint8) for t in range(n)])
    elif kind == "noise":
        y = r.integers(0, 256, (n, h, w), dtype=np.uint8)
    elif kind == "satnoise":
        y = (r.integers(0, 2, (n, h, w)) * 255).astype(np.uint8)
    else:
        raise ValueError(kind)
    y = np.ascontiguousarray(y)
    return y, np.ascontiguousarray(y[:, ::2, ::2]), np.ascontiguousarray(255 - y[:, 1::2, 1::2])


MED = dict(me_method=rs.ME_HEX, n_refs=3, inter=0x13, intra=0x3, transform8x8=1, mixed_refs=1, cabac=1, deblock=1)
MEDB = dict(MED, inter=0x113)
PARTS = dict(n_refs=2, inter=0x33, intra=0x3, transform8x8=1, mixed_refs=1, cabac=1, deblock=1)

# name: (source of the expected values, x264hip / harness parameters, harness extension, frames)
CONFIGS = {
    # ---- twin, CABAC writer in the loop: the raster variant -------------------------------------------------------------------------
    "s5_med": ("twin", dict(qp=26, subme=5, **MED), dict(), 5),
    "umh_sub8": ("twin", dict(qp=22, subme=5, me_method=rs.ME_UMH, **PARTS), dict(), 5),
    "esa": ("twin", dict(qp=26, subme=5, me_method=rs.ME_ESA, me_range=16, n_refs=2, inter=0x33, intra=0x1, mixed_refs=1, cabac=1, deblock=1), dict(), 5),
    "umh_r24_mv16": ("twin", dict(qp=24, subme=5, me_method=rs.ME_UMH, me_range=24, mv_range=16, alpha_c0=3, beta=-2, chroma_qp_offset=-4, **PARTS), dict(), 5),
    "nr_s4": ("twin", dict(qp=30, subme=4, me_method=rs.ME_DIA, n_refs=1, inter=0x11, intra=0x1, cabac=1, deblock=0, noise_reduction=80, chroma_me=0), dict(), 5),
    "jvt": ("twin", dict(qp=24, subme=5, me_method=rs.ME_HEX, cqm_preset=1, **PARTS), dict(), 5),
    "rd7_t1_aq": ("twin", dict(qp=26, subme=7, **MED), dict(trellis=1, psy_rd=1.0, aq_mode=1), 5),
    "rd7_t2_lowqp": ("twin", dict(qp=8, subme=7, **MED), dict(trellis=2, psy_rd=0.0), 5),           # psy-rd off: the I_PCM decision is live
    "qp51": ("twin", dict(qp=51, subme=7, **MED), dict(trellis=1, psy_rd=1.0), 5),
    "refs8_key3": ("twin", dict(qp=20, subme=7, me_method=rs.ME_HEX, n_refs=8, inter=0x13, intra=0x3, transform8x8=1, mixed_refs=1, cabac=1, deblock=1, keyint=3,
                                fast_pskip=0, dct_decimate=0), dict(trellis=2, psy_rd=0.4), 7),
    "rd8_t2": ("twin", dict(qp=30, subme=8, **MED), dict(trellis=2, psy_rd=0.0), 5),
    "rd9": ("twin", dict(qp=22, subme=9, **MED), dict(trellis=1, psy_rd=1.0), 5),
    "lossless": ("twin", dict(qp=0, subme=5, me_method=rs.ME_HEX, fast_pskip=0, **PARTS), dict(), 5),
    "b_s5": ("twin", dict(qp=30, subme=5, **MEDB), dict(bframes=2, weightb=1, direct_pred=1), 5),
    "b_temporal": ("twin", dict(qp=28, subme=6, **MEDB), dict(trellis=1, psy_rd=1.0, bframes=2, weightb=0, direct_pred=2), 5),
    "b_rd7": ("twin", dict(qp=26, subme=7, **MEDB), dict(trellis=1, psy_rd=1.0, aq_mode=1, bframes=2, weightb=1, direct_pred=1), 5),
    "rd8_b_aq": ("twin", dict(qp=33, subme=8, **MEDB), dict(trellis=2, psy_rd=1.0, aq_mode=1, aq_strength=1.8, bframes=3, weightb=1, direct_pred=2), 7),
    # ---- twin, no writer: the wavefront variant --------------------------------------------------------------------------------------
    "plain_uf": ("plain", dict(qp=30, subme=0), None, 5),
    "plain_s5": ("plain", dict(qp=27, me_method=rs.ME_HEX, subme=5, n_refs=3, inter=0x33, intra=0x3, transform8x8=1, mixed_refs=1, cabac=0, deblock=1), None, 5),
    "plain_s3_cabac": ("plain", dict(qp=34, subme=3, me_method=rs.ME_UMH, inter=0x13, intra=0x3, transform8x8=1, n_refs=2, cabac=1, deblock=1, dct_decimate=0), None, 5),
    "plain_ll": ("plain", dict(qp=0, subme=2, me_method=rs.ME_UMH, n_refs=1, inter=0x11, intra=0x1, deblock=1, fast_pskip=0), None, 5),
    # ---- the reference as recorded: CAVLC payloads (cabac = 0, write = 1), lossless with the RD levels --------------------------------
    "cavlc_parts": ("ref", dict(qp=27, me_method=rs.ME_HEX, subme=5, n_refs=3, inter=0x33, intra=0x3, transform8x8=1, mixed_refs=1, cabac=0, deblock=1), dict(), 5),
    "cavlc_aq": ("ref", dict(qp=28, me_method=rs.ME_HEX, subme=5, n_refs=2, inter=0x33, intra=0x3, transform8x8=1, mixed_refs=1, cabac=0, deblock=1), dict(aq_mode=1), 5),
    "cavlc_b": ("ref", dict(qp=28, me_method=rs.ME_HEX, subme=5, n_refs=2, inter=0x113, intra=0x3, transform8x8=1, cabac=0, deblock=1),
                dict(bframes=2, weightb=1, direct_pred=1), 5),
    "ll_rd6": ("ref", dict(qp=0, subme=6, me_method=rs.ME_HEX, n_refs=2, inter=0x13, intra=0x3, transform8x8=1, mixed_refs=1, cabac=1, deblock=1, fast_pskip=0), dict(), 5),
    "ll_rd8": ("ref", dict(qp=0, subme=8, me_method=rs.ME_HEX, n_refs=2, inter=0x13, intra=0x3, transform8x8=1, mixed_refs=1, cabac=1, deblock=1, fast_pskip=0), dict(), 5),
    "ll_rd9": ("ref", dict(qp=0, subme=9, me_method=rs.ME_UMH, n_refs=2, inter=0x13, intra=0x3, transform8x8=1, mixed_refs=1, cabac=1, deblock=1, fast_pskip=0), dict(), 5),
}


def at_qp(name, qp, **ext):
    """Configuration `name` at another constant QP (ext: what its harness extension takes on top)."""
    src, kw, ekw, frames = CONFIGS[name]
    return src, dict(kw, qp=qp), None if ekw is None else dict(ekw, **ext), frames


# ---- lossy QP 0..7: levels in the escape range of every entropy writer (CAVLC: level codes >= 4096, the High profile's growing prefix and
# the Baseline clamp; CABAC: deep in the Exp-Golomb tail of coeff_abs_level_minus1), macroblocks at QP 0 in a slice that is NOT lossless
# (I slices of QP 1..3 clip to 0, adaptive quantisation at QP 2 reaches it), I_PCM chosen often.  low_qp_problems() states what they reach.
CAVLC_QP1 = dict(qp=1, me_method=rs.ME_HEX, subme=5, n_refs=2, inter=0x33, intra=0x3, transform8x8=1, mixed_refs=1, cabac=0, deblock=1)
LOW_QP = {
    "cavlc_qp1_high": ("ref", CAVLC_QP1, dict(), 5),
    "cavlc_qp1_base": ("ref", dict(CAVLC_QP1, inter=0x31, intra=0x1, transform8x8=0), dict(), 5),
    "cavlc_b_qp1": at_qp("cavlc_b", 1),
    "cavlc_aq_qp2": at_qp("cavlc_aq", 2, aq_strength=1.8),
    "s5_qp1": at_qp("s5_med", 1),
    "rd7_aq_qp2": at_qp("rd7_t1_aq", 2, aq_strength=1.8),
    "rd9_t2_qp1": ("twin", dict(qp=1, subme=9, **MED), dict(trellis=2, psy_rd=0.0), 5),
    "b_temporal_qp1": at_qp("b_temporal", 1),
    "rd8_b_aq_qp2": at_qp("rd8_b_aq", 2),
    "plain_s5_qp1": at_qp("plain_s5", 1),
    "jvt_qp6": at_qp("jvt", 6),
}
CONFIGS.update(LOW_QP)
TWIN = [k for k, c in CONFIGS.items() if c[0] == "twin"]
PLAIN = [k for k, c in CONFIGS.items() if c[0] == "plain"]
REF = [k for k, c in CONFIGS.items() if c[0] == "ref"]
B_CONFIGS = [k for k in TWIN if CONFIGS[k][2].get("bframes")]

DECISIONS = ("mb_type", "mv", "ref", "qp", "cbp")
PLANES = ("fin_y", "fin_u", "fin_v")
WHOLE = DECISIONS[1:] + PLANES          # the fixture's whole-chain digests; payload and mb_type are per frame

# R/common/macroblock.h:78-102
I_4x4, I_8x8, I_16x16, I_PCM, P_L0, P_8x8, P_SKIP, B_DIRECT = range(8)
B_L0_L0, B_BI_BI, B_8x8, B_SKIP = 8, 16, 17, 18
B_LX_LX = tuple(range(B_L0_L0, B_BI_BI + 1))       # L0_L0 L0_L1 L0_BI L1_L0 L1_L1 L1_BI BI_L0 BI_L1 BI_BI
BIPRED = (10, 13, 14, 15, 16)                      # ... the ones with a bi-predicted half
TYPE_NAMES = {I_4x4: "I_4x4", I_8x8: "I_8x8", I_16x16: "I_16x16", I_PCM: "I_PCM", P_L0: "P_L0", P_8x8: "P_8x8", P_SKIP: "P_SKIP", B_DIRECT: "B_DIRECT",
              B_8x8: "B_8x8", B_SKIP: "B_SKIP", **{t: "B_Lx_Lx[%d]" % (t - B_L0_L0) for t in B_LX_LX}}


def order_of(name):
    """[(display index, slice type)] of a configuration's chain in coding order."""
    _, kw, ekw, frames = CONFIGS[name]
    key = kw.get("keyint", 0)
    if ekw and ekw.get("bframes"):
        return sl.coding_order(frames, key, ekw["bframes"])
    return [(t, sl.SLICE_I if (t % key == 0 if key else t == 0) else sl.SLICE_P) for t in range(frames)]


def expected_kind(name, stype):
    """The kernel kind frame_slice.hip's sweep_build selects for a slice of this configuration (as ChainEncoder drives it)."""
    src, kw, ekw, _ = CONFIGS[name]
    ekw = ekw or {}
    cavlc = src == "ref" and not kw["cabac"]
    if src == "plain" or (cavlc and not ekw.get("aq_mode") and not ekw.get("bframes")):
        return SW_KIND_PLAIN
    if stype == sl.SLICE_B:
        return SW_KIND_BT if ekw.get("direct_pred", 1) == 2 else SW_KIND_B
    if kw["qp"] == 0:
        return SW_KIND_LL_RF if kw["subme"] >= 8 else SW_KIND_LL
    return SW_KIND_RF if kw["subme"] >= 8 else SW_KIND_RD


def kinds_selected():
    return {expected_kind(n, t) for n in CONFIGS for _, t in order_of(n)}


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).digest()


def payload(a, f):
    return bytes(a["payload"][f, :int(a["payload_len"][f])])


@functools.lru_cache(maxsize=None)
def twin_lib():
    return C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))


@functools.lru_cache(maxsize=None)
def clip(kind, size, frames):
    out = content(kind, size[0], size[1], frames)
    for a in out:
        a.setflags(write=False)
    return out


# ---- x264hip_slice_sweep_chains (the chain table's own kernels): I / P chains with a QP per chain -----------------------------------------
TABLE_SIZES = [(16, 16), (32, 16), (16, 48), (40, 24)]
TABLE_QPS = (8, 26, 51)
# kernel : configuration.  Lossy: chain b codes content b at QP TABLE_QPS[b % 3]; lossless: every chain at QP 0
TABLE = {"ch_rd": "rd7_t1_aq", "ch_rf": "rd9", "ll_ch": "lossless", "ll_ch_rf": "ll_rd8"}


TABLE_LOW_QPS = (1, 2, 3)           # a second assignment for the lossy tables: chains at QP 1, 2 and 3 side by side (tablelow_<name>_*)
TABLE_LOSSY = [n for n in TABLE.values() if CONFIGS[n][1]["qp"] != 0]


def table_qps(name, low=False):
    return [0 if CONFIGS[name][1]["qp"] == 0 else (TABLE_LOW_QPS if low else TABLE_QPS)[b % 3] for b in range(len(CONTENTS))]


def params(name, size, qp=None):
    _, kw, _, frames = CONFIGS[name]
    return rs.make_params(size[0], size[1], frames, **(kw if qp is None else dict(kw, qp=qp)))


@functools.lru_cache(maxsize=None)
def twin_chain(name, size, kind, qp=None):
    """The twin's arrays for one chain (frames in coding order), computed once and left unchanged.  A "ref" configuration's CAVLC chain: the
    decisions alone (write = 0); its lossless chains above subme 5 are not the twin's to code (None).  qp: another constant QP."""
    src, kw, ekw, frames = CONFIGS[name]
    y, u, v = clip(kind, size, frames)
    if src == "plain":
        a = rs.run(twin_lib(), "x264o_encode_chain", params(name, size, qp), y, u, v)
    elif src == "ref" and kw["cabac"]:
        return None
    else:
        a = rs.run2(twin_lib(), "x264o_encode_chain2", params(name, size, qp), rs.make_ext(**dict(ekw, write=int(src == "twin"))), y, u, v)
    for arr in a.values():
        arr.setflags(write=False)
    return a


def reference_chain(name, size, kind, qp=None):
    """The same chain through the reference's own loop, live (needs oracle/_ref/libx264ref.so)."""
    src, kw, ekw, frames = CONFIGS[name]
    y, u, v = clip(kind, size, frames)
    if src == "plain":
        return rs.run_reference(params(name, size, qp), y, u, v)
    return rs.run_reference2(params(name, size, qp), rs.make_ext(write=1, **ekw), y, u, v)


def digests(a, name):
    """What the fixture keeps of one chain: md5 of every frame's payload (a chain without a writer has none), of every frame's mb_type, and
    of each array of WHOLE over the chain.  None of these arrays has undefined entries in the reference's output (mvr, which
    gen_golden_slice.masked2 masks, is not among them): the reference clears a macroblock's vectors and reference indices before it
    decides, and the twin equals it on every entry."""
    frames = CONFIGS[name][3]
    pay = np.array([list(md5(np.frombuffer(payload(a, f), np.uint8))) if "payload" in a else [0] * 16 for f in range(frames)], np.uint8)
    mbt = np.array([list(md5(a["mb_type"][f])) for f in range(frames)], np.uint8)
    whole = np.array([list(md5(a[k])) for k in WHOLE], np.uint8)
    return pay, mbt, whole


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def recorded(name, size, kind, table=False):
    """(payload md5 [frames][16], mb_type md5 [frames][16], {array: md5}) of the reference's chain as tests/golden/edge_chains.npz holds it.
    table: the chain at its chain-table QP (table_qps), recorded as table_<name>_* over TABLE_SIZES; table="low": at table_qps(name, low=True),
    tablelow_<name>_*."""
    g, i, j = fixture(), (TABLE_SIZES if table else SIZES).index(size), CONTENTS.index(kind)
    name = ("tablelow_" if table == "low" else "table_" if table else "") + name
    return g[name + "_payload"][i, j], g[name + "_mb_type"][i, j], {k: bytes(g[name + "_whole"][i, j, n]) for n, k in enumerate(WHOLE)}


LEVELS = ("luma", "luma_dc", "chroma_dc", "chroma_ac")


def max_level(a):
    """The largest |level| among the recorded coefficient levels of one chain."""
    return max(int(np.abs(a[k].astype(np.int32)).max()) for k in LEVELS)


def recorded_max_level(name, size, kind):
    """The largest |level| of the reference's chain (<name>_max_level of the fixture, the LOW_QP configurations), None where none is kept."""
    g = fixture()
    return int(g[name + "_max_level"][SIZES.index(size), CONTENTS.index(kind)]) if name + "_max_level" in g else None


def writer_branch(name, size, kind):
    """For a failure's message: where the chain's largest level puts it in the entropy writers."""
    m = recorded_max_level(name, size, kind)
    if m is None:
        return ""
    if not CONFIGS[name][1].get("cabac"):
        arm = "High profile's growing prefix" if CONFIGS[name][1].get("transform8x8") or CONFIGS[name][1].get("cqm_preset") else "Baseline clamp"
        return " [largest |level| %d: %s]" % (m, "CAVLC level code >= 4096, the " + arm if m >= CAVLC_ESCAPE_LEVEL else "below the CAVLC extended escape")
    return " [largest |level| %d: %d bits of Exp-Golomb suffix]" % (m, 2 * max(m - 14, 1).bit_length() - 1 if m > 14 else 0)


def have_reference():
    return os.path.exists(REF_SO)


def size_id(s):
    return "%dx%d" % s


# |level| from which cv_residual's level code is >= 4096 at every suffix length (the extended escape: 2064 at suffix length 0, 2529 at 6)
CAVLC_ESCAPE_LEVEL = 2600
JVT_LEVEL = 3000


def low_qp_problems(chains):
    """What the LOW_QP configurations must reach, over [(configuration, size, content kind, mb_type [frames][n_mb], qp [frames][n_mb],
    largest |level|)]: a list of what is missing.  The two cavlc_qp1 configurations have, at every size, a chain with a level whose CAVLC
    code is in the extended escape; every one but jvt_qp6 has a macroblock at QP 0 (none of them is lossless); rd9_t2_qp1 chooses I_PCM
    at every size; jvt_qp6 reaches |level| >= 3000."""
    esc, pcm, qp0, top = {}, set(), set(), {}
    for name, size, kind, t, qp, lvl in chains:
        if name not in LOW_QP:
            continue
        assert CONFIGS[name][1]["qp"] != 0
        top[name] = max(top.get(name, 0), lvl)
        if lvl >= CAVLC_ESCAPE_LEVEL:
            esc.setdefault(name, set()).add(size)
        if name == "rd9_t2_qp1" and (t == I_PCM).any():
            pcm.add(size)
        if (qp == 0).any():
            qp0.add(name)
    bad = ["%s: no |level| >= %d at %dx%d" % ((name, CAVLC_ESCAPE_LEVEL) + s) for name in ("cavlc_qp1_high", "cavlc_qp1_base") for s in SIZES if s not in esc.get(name, ())]
    bad += ["%s: no macroblock at QP 0" % name for name in LOW_QP if name != "jvt_qp6" and name not in qp0]
    bad += ["rd9_t2_qp1: no I_PCM macroblock at %dx%d" % s for s in SIZES if s not in pcm]
    if top.get("jvt_qp6", 0) < JVT_LEVEL:
        bad.append("jvt_qp6: largest |level| %d, below %d" % (top.get("jvt_qp6", 0), JVT_LEVEL))
    return bad


def coverage_problems(chains):
    """The coverage conditions of the case list, over [(configuration, size, content kind, mb_type [frames][n_mb])]: a list of what is
    missing (empty: all hold).  Every macroblock type occurs; I_PCM occurs at every size; every configuration reaches a non-skip inter
    macroblock and, in P or B slices, an intra one; every B configuration reaches B_SKIP, B_DIRECT and a bi-predicted type."""
    seen, pcm_sizes, per_cfg = set(), set(), {}
    for name, size, kind, t in chains:
        types = set(np.unique(t).tolist())
        seen |= types
        if I_PCM in types:
            pcm_sizes.add(size)
        inter_frames = np.array([st != sl.SLICE_I for _, st in order_of(name)])
        c = per_cfg.setdefault(name, dict(inter=False, intra=False, types=set()))
        c["types"] |= types
        c["inter"] |= bool(np.isin(t, (P_L0, P_8x8, B_DIRECT, B_8x8) + B_LX_LX).any())
        c["intra"] |= bool((t[inter_frames] <= I_PCM).any())
    bad = ["no macroblock of type %s" % TYPE_NAMES[t] for t in TYPE_NAMES if t not in seen]
    bad += ["no I_PCM macroblock at %dx%d" % s for s in SIZES if s not in pcm_sizes]
    for name, c in per_cfg.items():
        if not c["inter"]:
            bad.append("%s: no non-skip inter macroblock" % name)
        if not c["intra"]:
            bad.append("%s: no intra macroblock in a P or B slice" % name)
        if (CONFIGS[name][2] or {}).get("bframes"):
            bad += ["%s: no %s" % (name, w) for w, ts in (("B_SKIP", (B_SKIP,)), ("B_DIRECT", (B_DIRECT,)), ("bi-predicted type", BIPRED)) if not c["types"] & set(ts)]
    return bad
