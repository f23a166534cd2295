// mb_vocab.h -- the macroblock syntax vocabulary, stated once for the sweep, the CABAC writer and the CAVLC writer: the reference's
// numbering of macroblock types, partitions and sub-partitions, x264_scan8, the list-use tables of B macroblocks, the prediction-mode
// fixes, the predicted intra 4x4 mode and the motion vector predictors.  Plain C++; -DX264HIP_HOST_TEST compiles the same text for the
// host (cabac_dev.h and cavlc_dev.h are driven there by the CPU tests).
#pragma once
#include <stdint.h>
#ifdef X264HIP_HOST_TEST
#include <string.h>
#include <stdlib.h>
#define MB_FN static inline
#define __device__
#define __constant__ const
typedef uint8_t u8; typedef int16_t i16; typedef uint16_t u16; typedef uint32_t u32;
#else
#define MB_FN __device__ __forceinline__
#endif

enum { T_I_4x4 = 0, T_I_8x8 = 1, T_I_16x16 = 2, T_I_PCM = 3, T_P_L0 = 4, T_P_8x8 = 5, T_P_SKIP = 6,      // R/common/macroblock.h:78-102
       T_B_DIRECT = 7, T_B_L0_L0 = 8, T_B_L1_L1 = 12, T_B_BI_BI = 16, T_B_8x8 = 17, T_B_SKIP = 18 };
enum { D_L0_4x4 = 0, D_L0_8x4 = 1, D_L0_4x8 = 2, D_L0_8x8 = 3, D_L1_8x8 = 7, D_BI_8x8 = 11, D_DIRECT_8x8 = 12,
       D_8x8 = 13, D_16x8 = 14, D_8x16 = 15, D_16x16 = 16 };   // :55-76
#define IS_SKIP_T(t) ((t) == T_P_SKIP || (t) == T_B_SKIP)
#define IS_INTRA_T(t) ((t) >= 0 && (t) <= T_I_PCM)
// x264_mb_type_list_table (:94-106): does partition `part` of B type `t` (B_L0_L0 .. B_BI_BI) use list `l`?
// rows: L0L0 L0L1 L0BI L1L0 L1L1 L1BI BIL0 BIL1 BIBI; four bits each: l0p0 l0p1 l1p0 l1p1
#define B_USES(t_, l_, part_) ((int)((0xfd7ec6b93ull >> (4 * ((t_) - T_B_L0_L0) + 2 * (l_) + (part_))) & 1))
// x264_mb_partition_listX_table for the 8x8 sub-partitions (:140-156)
#define SUB_USES(s_, l_) ((s_) == D_DIRECT_8x8 ? 0 : (l_) ? ((s_) >= 4 && (s_) <= 11) : ((s_) <= 3 || ((s_) >= 8 && (s_) <= 11)))

// x264_scan8 (R/common/common.h:196-238) of the 16 luma blocks alone -- what the sweep indexes, by values the compiler cannot bound:
// the range tests of the whole table cost its refinement instantiation a spill -- and of all entries: 4 + 4 chroma, the three DC
MB_FN int mb_scan8_luma(int i)
{
    const int x = ((i >> 2) & 1) * 8 + (i & 1) * 4, y = (i >> 3) * 8 + ((i >> 1) & 1) * 4;      // the block's pixel position
    return 4 + 1 * 8 + (x >> 2) + 8 * (y >> 2);
}
MB_FN int mb_scan8(int i)
{
    if (i < 16) return mb_scan8_luma(i);
    if (i < 20) return 1 + 1 * 8 + ((i - 16) & 1) + 8 * ((i - 16) >> 1);
    if (i < 24) return 1 + 4 * 8 + ((i - 20) & 1) + 8 * ((i - 20) >> 1);
    return 4 + 5 * 8 + (i - 24);
}
MB_FN int mb_median(int a, int b, int c) { const int mx = a > b ? a : b, mn = a < b ? a : b; return c > mx ? mx : c < mn ? mn : c; }
MB_FN int mb_fix4(int m) { return m < 0 ? -1 : m < 9 ? m : 2; }          // x264_mb_pred_mode4x4_fix
MB_FN int mb_fix8c(int m) { return m < 4 ? m : 0; }                      // x264_mb_pred_mode8x8c_fix
MB_FN int mb_fix16(int m) { return m < 4 ? m : 2; }                      // x264_mb_pred_mode16x16_fix
// x264_mb_predict_intra4x4_mode (R/common/macroblock.h:423-434) from the left and the top block's modes (-1: no such block)
MB_FN int mb_pred_i4mode(int left, int top)
{
    const int ma = mb_fix4(left), mb = mb_fix4(top), v = ma < mb ? ma : mb;
    return v < 0 ? 2 : v;
}

// The motion vector predictors.  A motion cache (h->mb.cache.ref / mv of one list, x264_scan8 layout) is read through three
// callables ref(k), mvx(k), mvy(k), so that a record's arrays, LDS behind a wave-uniform read and a cache held in registers all
// take the same statement.
// the part all predictors end in: by how many of the neighbours A (left), B (top), C (top right, or top left) share the reference
MB_FN void mb_predict_mv_abc(int i_ref, int ra, int rb, int rc, int ax, int ay, int bx, int by, int cx, int cy, int &px, int &py)
{
    const int cnt = (ra == i_ref) + (rb == i_ref) + (rc == i_ref);
    if (cnt > 1) { px = mb_median(ax, bx, cx); py = mb_median(ay, by, cy); }
    else if (cnt == 1) { if (ra == i_ref) { px = ax; py = ay; } else if (rb == i_ref) { px = bx; py = by; } else { px = cx; py = cy; } }
    else if (rb == -2 && rc == -2 && ra != -2) { px = ax; py = ay; }
    else { px = mb_median(ax, bx, cx); py = mb_median(ay, by, cy); }
}
// x264_mb_predict_mv_16x16 (R/common/macroblock.c:90-128)
template <class R, class X, class Y> MB_FN void mb_predict_mv_16x16(R ref, X mvx, Y mvy, int i_ref, int &px, int &py)
{
    int ra = ref(11), rb = ref(4), rc = ref(8), kc = 8;
    if (rc == -2) { kc = 3; rc = ref(3); }
    mb_predict_mv_abc(i_ref, ra, rb, rc, mvx(11), mvy(11), mvx(4), mvy(4), mvx(kc), mvy(kc), px, py);
}
// x264_mb_predict_mv (:28-88) of the block at idx, `width` 4x4 blocks wide; part = h->mb.i_partition
template <class R, class X, class Y> MB_FN void mb_predict_mv(R ref, X mvx, Y mvy, int part, int idx, int width, int &px, int &py)
{
    const int i8 = mb_scan8(idx), i_ref = ref(i8);
    int ra = ref(i8 - 1), rb = ref(i8 - 8), kc = i8 - 8 + width, rc = ref(kc);
    if ((idx & 3) == 3 || (width == 2 && (idx & 3) == 2) || rc == -2) { kc = i8 - 8 - 1; rc = ref(kc); }
    const int ax = mvx(i8 - 1), ay = mvy(i8 - 1), bx = mvx(i8 - 8), by = mvy(i8 - 8), cx = mvx(kc), cy = mvy(kc);
    if (part == D_16x8) {
        if (idx == 0 && rb == i_ref) { px = bx; py = by; return; }
        if (idx != 0 && ra == i_ref) { px = ax; py = ay; return; }
    } else if (part == D_8x16) {
        if (idx == 0 && ra == i_ref) { px = ax; py = ay; return; }
        if (idx != 0 && rc == i_ref) { px = cx; py = cy; return; }
    }
    mb_predict_mv_abc(i_ref, ra, rb, rc, ax, ay, bx, by, cx, cy, px, py);
}
