// cabac_price.h -- the RD trials' bit count of a whole macroblock (x264_macroblock_size_cabac, the RDO_SKIP_BS build of
// R/encoder/cabac.c; R/encoder/rdo.c:139-171 calls it once per candidate) without lane 0 scanning coefficient arrays in LDS.  Before lane 0
// starts, the wave ballots the nonzero masks of every coefficient array the count can touch (seven 64-bit wave-uniform masks, one
// coefficient per lane).  A block's last coefficient is then its mask's highest bit, a zero between two coefficients is a clear bit, and
// a level is read only where a bit is set -- where cw_residual reads every position twice, one dependent LDS round trip each (the backward
// scan for the last coefficient, then the counting loop), however few coefficients the block holds.  Positions, contexts and the order
// of the bins are cw_residual's rd branch.
// The context states and the coder's tables stay where they were (the trial's copy of the states and the tables in LDS, lane 0 walking):
// DESIGN.md 3.1c has what holding them in lane-indexed registers and walking on all 64 lanes cost instead.
//
// Everything in front of the residual is cabac_dev.h's cw_mb_head.  Plain C++, compiled for the host too (-DX264HIP_HOST_TEST:
// tests/cabac_price_host.cpp, where a loop over 64 lanes stands for the ballot).
#pragma once
#include "cabac_dev.h"

typedef unsigned long long cp_u64;
#ifdef X264HIP_HOST_TEST
#define CP_UNI(x_) ((int)(x_))
#else
#define CP_UNI(x_) __builtin_amdgcn_readfirstlane((int)(x_))     /* the walking lane's value in a scalar register */
#endif

// ---- the masks: bit k of a mask is "coefficient k of these 64 is not zero"
struct CpMasks { cp_u64 y0, y1, y2, y3, c0, c1, d; };     // 256 luma levels (of the transform the macroblock uses), 128 chroma AC, lv_dc | lv_cdc << 16
template <class MS> CD_FN int cp_luma8(const MS &m) { return m.t8 && m.type != T_I_16x16; }    // which luma array cw_macroblock walks
// lane `lane`'s bit of ballot q: 0..3 luma, 4 / 5 chroma AC, 6 the three DC arrays
template <class MS> CD_FN bool cp_mask_lane(const MS &m, int q, int lane)
{
    if (q < 4) return (cp_luma8(m) ? (&m.lv8[0][0])[64 * q + lane] : (&m.lv4[0][0])[64 * q + lane]) != 0;
    if (q < 6) return (&m.lv_cac[0][0])[64 * (q - 4) + lane] != 0;
    return lane < 16 ? m.lv_dc[lane] != 0 : lane < 24 ? (&m.lv_cdc[0][0])[lane - 16] != 0 : false;
}
// ballot(q): the wave's bits of cp_mask_lane(m, q, lane)
template <class BAL> CD_FN CpMasks cp_masks(BAL ballot)
{
    CpMasks k;
    k.y0 = ballot(0); k.y1 = ballot(1); k.y2 = ballot(2); k.y3 = ballot(3); k.c0 = ballot(4); k.c1 = ballot(5); k.d = ballot(6);
    return k;
}
// a block's mask, bit 0 = the first coefficient the block codes (category: 0 luma DC, 1 luma AC, 2 luma 4x4, 3 chroma DC, 4 chroma AC,
// 5 luma 8x8; idx: the block's index in non_zero_count, as cw_residual takes it)
CD_FN cp_u64 cp_block_mask(const CpMasks &k, int cat, int idx)
{
    if (cat == 0) return k.d & 0xffffu;
    if (cat == 3) return (k.d >> (16 + 4 * (idx - 25))) & 15u;
    if (cat == 4) return ((idx < 20 ? k.c0 : k.c1) >> (16 * (idx & 3) + 1)) & 0x7fffu;
    const int q = idx >> 2;                     // an 8x8 block is named by its first 4x4 block
    const cp_u64 y = q == 0 ? k.y0 : q == 1 ? k.y1 : q == 2 ? k.y2 : k.y3;
    if (cat == 5) return y;
    return cat == 1 ? (y >> (16 * (idx & 3) + 1)) & 0x7fffu : (y >> (16 * (idx & 3))) & 0xffffu;
}

// block_residual_write_cabac in the RD order (R/encoder/cabac.c:679-763; cw_residual's rd branch) from the block's mask
template <class ST, class MS, class LV> CD_FN void cp_residual(DCabac &cb, ST st, const MS &m, int cat, int idx, LV l, int count, cp_u64 mask)
{
    const int c_sig = CD_SIG_OFF(cat), c_last = CD_LAST_OFF(cat), c_lvl = CD_LEVEL_OFF(cat), b8 = cat == 5;
    if (!b8) {
        const int ctx = 85 + cw_cbf_ctx(m, cat, idx);
        if (!CP_UNI(m.nnz[idx])) { cdd(cb, st, 1, ctx, 0); return; }
        cdd(cb, st, 1, ctx, 1);
    }
    if (!mask) return;                          // (a count that says "coded" over an empty block: nothing follows, as in cw_residual)
    const int last = 63 - __builtin_clzll(mask);
    int node = 0;
    for (int i = last; i >= 0; i--) {
        const int cs = c_sig + (b8 ? CP_UNI(CD_SIG8(i < 63 ? i : 62)) : i), cl = c_last + (b8 ? CP_UNI(CD_LAST8(i < 63 ? i : 62)) : i);
        if (i == last) {
            if (last != count - 1) { cdd(cb, st, 1, cs, 1); cdd(cb, st, 1, cl, 1); }
        } else if ((mask >> i) & 1) { cdd(cb, st, 1, cs, 1); cdd(cb, st, 1, cl, 0); }
        else { cdd(cb, st, 1, cs, 0); continue; }
        const int v = CP_UNI(l[i]);
        const int am1 = cd_abs(v) - 1, prefix = am1 < 14 ? am1 : 14;
        int ctx = CD_LVL1_CTX(node) + c_lvl;
        if (prefix) {
            cdd(cb, st, 1, ctx, 1);
            ctx = CD_LVLGT1_CTX(node) + c_lvl;
            cb.f8 += cd_unary(st, ctx, prefix);
            if (prefix >= 14) cd_ue(cb, 1, 0, am1 - 14);
            node = CD_NODE_NEXT1(node);
        } else {
            cdd(cb, st, 1, ctx, 0);
            node = CD_NODE_NEXT0(node);
            cb.f8 += 256;
        }
    }
}

// x264_macroblock_size_cabac: cw_macroblock(cb, st, 1, m, fe, 0) with the residual from the masks.  The count is cb.f8.
template <class ST, class MS> CD_FN void cp_macroblock(DCabac &cb, ST st, MS &m, const CpMasks &k)
{
    const int type = m.type;
    if (!cw_mb_head(cb, st, 1, m, (const u8 *)nullptr, 0)) return;
    if (type == T_I_16x16) {
        cp_residual(cb, st, m, 0, 24, &m.lv_dc[0], 16, cp_block_mask(k, 0, 24));
        if (m.cbp_luma) for (int i = 0; i < 16; i++) cp_residual(cb, st, m, 1, i, &m.lv4[i][1], 15, cp_block_mask(k, 1, i));
    } else if (m.t8) {
        for (int i = 0; i < 4; i++) if (m.cbp_luma & (1 << i)) cp_residual(cb, st, m, 5, 4 * i, &m.lv8[i][0], 64, cp_block_mask(k, 5, 4 * i));
    } else
        for (int i = 0; i < 16; i++) if (m.cbp_luma & (1 << (i >> 2))) cp_residual(cb, st, m, 2, i, &m.lv4[i][0], 16, cp_block_mask(k, 2, i));
    if (m.cbp_chroma & 3) {
        cp_residual(cb, st, m, 3, 25, &m.lv_cdc[0][0], 4, cp_block_mask(k, 3, 25));
        cp_residual(cb, st, m, 3, 26, &m.lv_cdc[1][0], 4, cp_block_mask(k, 3, 26));
    }
    if (m.cbp_chroma & 2) for (int i = 16; i < 24; i++) cp_residual(cb, st, m, 4, i, &m.lv_cac[i - 16][1], 15, cp_block_mask(k, 4, i));
}
