"""Helper of tests/test_cavlc_host.py and tests/test_gpu_cavlc.py: hand-built x264hip_mb_state arrays of one 3x2-macroblock slice with every
syntax element at the longest code the derivation beside CV_MB_BYTES_MAX (csrc/frame_cavlc.hip) lists -- what no quantiser produces and the
entry points' C ABI nevertheless accepts.  Four kinds of slice:

  "i16"  I slice, all I_16x16, cbp 0x2f;
  "i4"   I slice, all I_4x4 whose modes never equal their prediction, cbp 0x2f;
  "p8"   P slice, all P_8x8 of four 4x4 sub-partitions, 16 references, every block on reference 15, vectors alternating 32767 / -32768 from
         one 4x4 block to the next in both directions (the median predictor is then the other value: every difference is +-65535);
  "b8"   B slice, all B_8x8 of four bi-predicted 8x8 blocks, the same in both lists from one 8x8 block to the next,

each with all 384 levels of a macroblock at `levels`: "min" -32768, "alt" +-32767 in turn, "rand" uniform in -2000..2000 with a third
of them zero and some +-1 (seeded; the range real content at QP 1 reaches, where the writer is pinned to the reference).  The QP
alternates 0 / 26 so that every mb_qp_delta is -26."""
import numpy as np

from cavlc_host_util import MB_BYTES_MAX, STATE_ARRAYS
from x264_vs2008_amd.slice import PAYLOAD_LEAD

MB_W, MB_H = 3, 2
N = MB_W * MB_H
I_4x4, I_16x16, P_8x8, B_8x8 = 0, 2, 5, 17             # mb_vocab.h: T_*
D_L0_4x4, D_BI_8x8, D_8x8 = 0, 11, 13                  # ... D_*
SLICE_P, SLICE_B, SLICE_I = 0, 1, 2
KINDS = {"i16": SLICE_I, "i4": SLICE_I, "p8": SLICE_P, "b8": SLICE_B}
N_REF0 = 16
SLICE_QP = 26
LEVELS_PER_MB = 384                                    # 16 + 16 x 15 luma (or 16 x 16), 2 x 4 chroma DC, 8 x 15 chroma AC
HIGH_MB_BITS_MIN = LEVELS_PER_MB * 36                  # a level of -32768 ends at prefix 19 in High profile: 20 + 16 bits; = 8 x 1728


def levels_of(how, shape, seed):
    if how == "min":
        return np.full(shape, -32768, np.int16)
    if how == "alt":
        return (32767 * (1 - 2 * (np.arange(int(np.prod(shape))) & 1))).astype(np.int16).reshape(shape)
    r = np.random.default_rng(5150 + seed)
    v = r.integers(-2000, 2001, shape)
    pick = r.integers(0, 6, shape)
    return np.where(pick < 2, 0, np.where(pick == 2, np.sign(v), v)).astype(np.int16)


def state(kind, levels):
    """{name: array} over STATE_ARRAYS for one chain of MB_W x MB_H macroblocks."""
    st = dict(mb_type=np.zeros(N, np.int8), partition=np.full(N, D_8x8, np.int8), sub_partition=np.zeros((N, 4), np.int8),
              ref=np.full((N, 4), -1, np.int8), ref1=np.full((N, 4), -1, np.int8), mv=np.zeros((N, 16, 2), np.int16), mv1=np.zeros((N, 16, 2), np.int16),
              i4mode=np.full((N, 16), 2, np.int8), i16mode=(np.arange(N) % 4).astype(np.int8), chroma_mode=((np.arange(N) + 1) % 4).astype(np.int8),
              qp=(26 * (np.arange(N) & 1)).astype(np.int8), cbp=np.full(N, 0x2f, np.int16), t8=np.zeros(N, np.int8),
              luma=levels_of(levels, (N, 256), 1), luma_dc=levels_of(levels, (N, 16), 2), chroma_dc=levels_of(levels, (N, 8), 3),
              chroma_ac=levels_of(levels, (N, 128), 4))
    by, bx = np.mgrid[0:4, 0:4]
    for m in range(N):
        gx, gy = 4 * (m % MB_W) + bx, 4 * (m // MB_W) + by         # the 4x4 blocks' positions in the picture
        if kind == "i16":
            st["mb_type"][m] = I_16x16
            st["luma"][m, ::16] = 0                                # (an I_16x16 block's DC lives in luma_dc)
            st["chroma_ac"][m, ::16] = 0
        elif kind == "i4":
            st["mb_type"][m] = I_4x4
            # modes 0 / 1 in a checkerboard: the prediction (the smaller of left and top, DC without one) is the other mode or DC
            st["i4mode"][m, (bx & 1) + ((by & 1) << 1) + ((bx >> 1) << 2) + ((by >> 1) << 3)] = (gx + gy) & 1
        elif kind == "p8":
            st["mb_type"][m], st["sub_partition"][m], st["ref"][m] = P_8x8, D_L0_4x4, N_REF0 - 1
            st["mv"][m] = np.where((gx + gy) & 1, -32768, 32767).astype(np.int16).reshape(16, 1)
        elif kind == "b8":
            st["mb_type"][m], st["sub_partition"][m], st["ref"][m], st["ref1"][m] = B_8x8, D_BI_8x8, N_REF0 - 1, 0
            v = np.where(((gx >> 1) + (gy >> 1)) & 1, -32768, 32767).astype(np.int16).reshape(16, 1)
            st["mv"][m], st["mv1"][m] = v, -1 - v
        else:
            raise ValueError(kind)
    assert set(st) == set(STATE_ARRAYS)
    return st


def params(kind, profile_high):
    """write_state's keywords for a slice of this kind: sub-8x8 partitions analysed; High profile by the 8x8 transform's flag (every
    macroblock then carries transform_size_8x8_flag where the syntax has one)."""
    return dict(slice_type=KINDS[kind], slice_qp=SLICE_QP, n_ref0=N_REF0 if kind in ("p8", "b8") else 1, inter=0x33, transform8x8=int(profile_high), cqm_custom=0)


def mb_sizes(bits):
    """Bits per macroblock from the positions after every macroblock."""
    return np.diff(np.concatenate([[0], bits]))


def full_slot_cap(bits, k=2):
    """A payload_cap with which macroblock k + 1 begins between cap - 64 - 2624 and cap - 64 - 1024 bytes into its slot, 16 bytes below the
    latter: a margin of 2624 stops the writer there, one of 1024 lets it write a macroblock of which 1040 bytes fit."""
    begin = (int(bits[k]) + 7) // 8
    cap = begin + PAYLOAD_LEAD + 1024 + 16
    assert cap - PAYLOAD_LEAD - MB_BYTES_MAX < begin - 1 and begin < cap - PAYLOAD_LEAD - 1024 and cap >= 4096, (begin, cap)
    return cap
