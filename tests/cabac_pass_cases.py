"""The cases of the CABAC pass (x264hip_cabac_write_frame; csrc/cabac_pass_dev.h), shared by tests/test_cabac_pass_host.py and
tests/test_gpu_cabac_pass.py, and -- under __main__ -- the generator of their fixtures tests/golden/cabac_pass_<name>.npz: payload,
payload_len, mb_bits and frame_info of the REFERENCE's own loop with its CABAC writer (oracle/refslice.py: refslice_encode_chain2 with
write = 1; needs oracle/_ref/libx264ref.so).

    python tests/cabac_pass_cases.py [name ...]

I / P chains below the RD levels, cabac = 1, subme 1..5, on pictures of 6x5 and 3x2 macroblocks.  A case's clip is ("synth", t0) --
x264_vs2008_amd.synth's frames from t0 on --, ("edge", kind), edge_cases.content, or ("stripes", seed), stripes() below: macroblock columns of
noise beside perfectly flat ones, where adaptive quantisation gives neighbours different QPs and a flat macroblock under a flat one is an I_16x16
without a single coefficient.  LIVE_CLIPS names the other clip the live test runs the same case on.  coverage() counts the syntax branches the cases must reach together (test_cases_reach_every_branch)."""
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import edge_cases as ec
from oracle import refslice as rs
from paths import GOLDEN

P33 = dict(me_method=rs.ME_HEX, inter=0x33, intra=0x3, cabac=1, deblock=1)
P13 = dict(me_method=rs.ME_HEX, inter=0x13, intra=0x3, cabac=1, deblock=1)
CASES = {
    "s5_ref3_mixed": dict(size=(96, 80), n=4, clip=("synth", 0), kw=dict(P33, qp=24, subme=5, n_refs=3, mixed_refs=1, transform8x8=1)),
    "s4_ref3_nomix": dict(size=(96, 80), n=4, clip=("synth", 9), kw=dict(P13, qp=28, subme=4, n_refs=3, mixed_refs=0, transform8x8=1)),
    "s3_ref1_no8x8dct": dict(size=(96, 80), n=3, clip=("edge", "ramp"), kw=dict(P33, qp=26, subme=3, n_refs=1, transform8x8=0)),
    "s1_low_qp": dict(size=(40, 24), n=3, clip=("edge", "noise"), kw=dict(P13, qp=10, subme=1, n_refs=1, transform8x8=1)),
    "s2_high_qp": dict(size=(96, 80), n=4, clip=("synth", 3), kw=dict(P13, qp=42, subme=2, n_refs=1, transform8x8=1, me_method=rs.ME_DIA)),
    "s5_jvt": dict(size=(40, 24), n=3, clip=("edge", "vstripe"), kw=dict(P33, qp=24, subme=5, n_refs=2, mixed_refs=1, transform8x8=1, cqm_preset=1)),
    "aq_s5": dict(size=(96, 80), n=4, clip=("synth", 0), ext=dict(aq_mode=1, aq_strength=1.0),
                  kw=dict(P33, qp=28, subme=5, n_refs=2, mixed_refs=1, transform8x8=1)),
    "aq_strong_s3": dict(size=(96, 80), n=4, clip=("synth", 5), ext=dict(aq_mode=1, aq_strength=1.8),
                         kw=dict(P13, qp=36, subme=3, n_refs=1, transform8x8=1, keyint=2, me_method=rs.ME_UMH)),
    # x264_cabac_mb_qp_delta's side effect: an I_16x16 without coefficients right behind a macroblock of another QP takes that QP -- which the
    # next macroblock's QP rule and the loop filter then read
    # next macroblock's QP rule and the loop filter then read.  A loop without a writer decides differently from there on, so this case's
    # arrays come from the twin WITH its writer (twin_write: the state a sweep without a writer leaves since it applies the side effect itself)
    "aq_empty_i16": dict(size=(96, 80), n=4, clip=("stripes", 1), ext=dict(aq_mode=1, aq_strength=0.8), twin_write=1,
                         kw=dict(P13, qp=30, subme=5, n_refs=2, transform8x8=1, keyint=2)),
}
# lossy QP 1 (I slices at QP 0, not lossless): levels beyond 2900, deep in the Exp-Golomb tail of coeff_abs_level_minus1 -- edge_cases.MED at the
# smallest and the largest tiny picture on the three contents with the largest levels
QP1_SIZES, QP1_KINDS = ((40, 24), (16, 16)), ("checker", "noise", "satnoise")
QP1_KW = dict(ec.MED, qp=1, subme=5)
QP1_LEVEL = 2900
CASES.update({"qp1_%dx%d_%s" % (s + (k,)): dict(size=s, n=3, clip=("edge", k), kw=QP1_KW) for s in QP1_SIZES for k in QP1_KINDS})
LIVE_CLIPS = {("edge", "checker"): ("edge", "vstripe"), ("edge", "satnoise"): ("edge", "flip"), ("stripes", 1): ("stripes", 2), ("synth", 0): ("synth", 37), ("synth", 9): ("synth", 21), ("synth", 3): ("synth", 50), ("synth", 5): ("synth", 14),
              ("edge", "ramp"): ("edge", "checker"), ("edge", "noise"): ("edge", "satnoise"), ("edge", "vstripe"): ("edge", "ramp")}
FIXTURE_KEYS = ("payload", "payload_len", "mb_bits", "frame_info")


def stripes(seed, w, h, n):
    """n frames: 16-pixel columns of noise (a new one every frame) and of flat 128 in turn, the flat ones first; chroma alike."""
    r = np.random.default_rng(977 + seed)
    out = []
    for width, height, amp in ((w, h, 40), (w // 2, h // 2, 12), (w // 2, h // 2, 12)):
        col = 16 if width == w else 8
        flat = (np.arange(width) // col) % 2 == 0
        p = (128 + r.integers(-amp, amp + 1, (n, height, width))).astype(np.uint8)
        p[:, :, flat] = 128
        out.append(np.ascontiguousarray(p))
    return tuple(out)


def clip_of(c, live=False):
    kind, arg = LIVE_CLIPS[c["clip"]] if live else c["clip"]
    (w, h), n = c["size"], c["n"]
    return rs.clip(w, h, n, arg) if kind == "synth" else stripes(arg, w, h, n) if kind == "stripes" else ec.content(arg, w, h, n)


def params_of(c):
    return rs.make_params(c["size"][0], c["size"][1], c["n"], **c["kw"])


def twin_arrays(oracle_lib, c, live=False, write=None):
    """The state arrays of the case's chain from the CPU twin: without a writer, unless the case (twin_write) or the caller says otherwise."""
    write = c.get("twin_write", 0) if write is None else write
    return rs.run2(oracle_lib, "x264o_encode_chain2", params_of(c), rs.make_ext(write=write, **c.get("ext", {})), *clip_of(c, live))


def empty_i16(a):
    """[frame][mb]: I_16x16 macroblocks without a single coefficient."""
    return (a["mb_type"] == rs.I_16x16) & (a["cbp"] == 0)


def reference(c, live=False):
    """The reference's own loop with its CABAC writer: arrays, payload, payload_len, mb_bits."""
    return rs.run_reference2(params_of(c), rs.make_ext(write=1, **c.get("ext", {})), *clip_of(c, live))


def fixture(name):
    with np.load(os.path.join(GOLDEN, "cabac_pass_%s.npz" % name)) as z:
        return {k: z[k] for k in z.files}


def coverage(a, c):
    """{branch: count} over the arrays of one chain; mb_w x mb_h from the case."""
    mb_w, mb_h = (c["size"][0] + 15) // 16, (c["size"][1] + 15) // 16
    t, part, sub, cbp, ref, qp = a["mb_type"], a["partition"], a["sub_partition"], a["cbp"].astype(np.int32), a["ref"], a["qp"].astype(np.int32)
    is_p8 = t == rs.P_8x8
    inter = (t == rs.P_L0) | is_p8
    out = {"I_4x4": (t == rs.I_4x4).sum(), "I_8x8": (t == rs.I_8x8).sum(),
           "I_16x16 with AC": ((t == rs.I_16x16) & ((cbp & 15) != 0)).sum(), "I_16x16 without AC": ((t == rs.I_16x16) & ((cbp & 15) == 0)).sum(),
           "P 16x16": ((t == rs.P_L0) & (part == 16)).sum(), "P 16x8": ((t == rs.P_L0) & (part == 14)).sum(), "P 8x16": ((t == rs.P_L0) & (part == 15)).sum(),
           "P_SKIP": (t == rs.P_SKIP).sum(), "reference > 0": (inter[..., None] & (ref > 0)).sum(), "inter with 8x8 transform": (inter & (a["t8"] == 1)).sum(),
           "non-zero mb_qp_delta": 0, "AQ: empty macroblock after a QP change": 0, "AQ: empty I_16x16 whose own QP is not the previous one": 0}
    for s, nm in enumerate(("4x4", "8x4", "4x8", "8x8")):
        out["P_8x8 sub " + nm] = (is_p8[..., None] & (sub == s)).sum()
    for v in range(3):
        out["chroma cbp %d" % v] = ((t != rs.P_SKIP) & (((cbp >> 4) & 3) == v)).sum()
    n = mb_w * mb_h
    for e, (x0, y0) in (("left", (0, 1)), ("right", (mb_w - 1, 1)), ("top", (1, 0)), ("bottom", (1, mb_h - 1))):
        idx = [y * mb_w + x for y in range(mb_h) for x in range(mb_w) if (x == x0 if e in ("left", "right") else y == y0)]
        out["coded macroblock on the %s edge" % e] = (t[:, idx] != rs.P_SKIP).sum()
    # mb_qp_delta as a CABAC writer codes it, and the macroblocks it skips: I_16x16 or inter without coefficients right behind a QP change
    for f in range(t.shape[0]):
        last, last_dqp = int(a["frame_info"][f, 1]), 0
        for m in range(n):
            ty, cb = int(t[f, m]), int(cbp[f, m])
            empty = ty == rs.P_SKIP or (ty != rs.I_16x16 and not cb & 0x3f) or (ty == rs.I_16x16 and not cb)
            q = last if empty else int(qp[f, m])
            out["non-zero mb_qp_delta"] += int(q != last)
            if c.get("ext", {}).get("aq_mode") and empty and ty in (rs.I_16x16, rs.P_L0, rs.P_8x8) and last_dqp:
                out["AQ: empty macroblock after a QP change"] += 1
            # (a state from a sweep without a writer keeps such a macroblock's own QP: the reference's writer, and the pass, replace it)
            out["AQ: empty I_16x16 whose own QP is not the previous one"] += int(ty == rs.I_16x16 and not cb and int(qp[f, m]) != last)
            last_dqp, last = q - last, q
    return {k: int(v) for k, v in out.items()}


def main():
    for name in sys.argv[1:] or sorted(CASES):
        a = reference(CASES[name])
        np.savez_compressed(os.path.join(GOLDEN, "cabac_pass_%s.npz" % name), **{k: a[k] for k in FIXTURE_KEYS})
        print(name, "frames", CASES[name]["n"], "bytes", a["payload_len"].tolist())


if __name__ == "__main__":
    main()
