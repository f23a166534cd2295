// cavlc_dev.h -- the CAVLC slice writer of frame_cavlc.hip's kernels (x264_macroblock_write_cavlc with block_residual_write_cavlc and
// the skip runs of x264_slice_write, R/encoder/cavlc.c:60-620, R/encoder/encoder.c:1200-1280): serial code of one lane over the plain
// arrays of an x264hip_mb_state.  Like cabac_dev.h the file is plain C++ over mb_vocab.h, and the same text compiles for the host
// (-DX264HIP_HOST_TEST): tests/cavlc_host.cpp runs it there on the reference's arrays against the reference's bytes, no GPU needed.
#pragma once
#include <string.h>
#include "x264hip.h"
#include "x264hip_lookahead.h"
#include "mb_vocab.h"
#include "cavlc_tables.h"

#define CV_MAX_W 512
// mb_type of a B macroblock with two partitions (H.264 table 7-14; 16x8, the 8x16 form is one more), by the lists of its halves in
// mb_vocab.h's order (B_USES); one 16x16 partition: 1 L0, 2 L1, 3 BI
static __device__ const u8 d_cv_b_type_16x8[9] = {4, 8, 12, 10, 6, 14, 16, 18, 20};

struct CvArgs {
    const signed char *mb_type, *partition, *sub_partition, *ref, *ref1, *i4mode, *i16mode, *chroma_mode, *t8;
    const i16 *mv, *mv1, *cbp, *luma, *luma_dc, *chroma_dc, *chroma_ac;
    const u8 *nnz;
    const signed char *qp; int slice_qp;
    u8 *payload; int payload_cap; int *payload_len, *mb_bits; int *abort_flag;
    int mb_w, mb_h, slice_type, n_ref0, psub8x8, t8_mode, profile_high;
    int chain, margin;                   // the batch element this slice belongs to; the bytes kept free behind the macroblock about to be written
};
// the arguments from the ABI's description of one slice of mb_w x mb_h macroblocks per chain (host code)
static inline void cv_args(CvArgs &a, const x264hip_mb_state *st, const x264hip_cavlc_params *p, int mb_w, int mb_h, int *abort_flag, int margin)
{
    memset(&a, 0, sizeof(a));
    a.mb_type = (const signed char *)st->mb_type; a.partition = (const signed char *)st->partition; a.sub_partition = (const signed char *)st->sub_partition;
    a.ref = (const signed char *)st->ref; a.ref1 = (const signed char *)st->ref1; a.i4mode = (const signed char *)st->i4mode; a.i16mode = (const signed char *)st->i16mode;
    a.chroma_mode = (const signed char *)st->chroma_mode; a.t8 = (const signed char *)st->t8;
    a.qp = (const signed char *)st->qp; a.slice_qp = p->slice_qp;
    a.mv = st->mv; a.mv1 = st->mv1; a.cbp = st->cbp; a.luma = st->luma; a.luma_dc = st->luma_dc; a.chroma_dc = st->chroma_dc; a.chroma_ac = st->chroma_ac; a.nnz = st->nnz;
    a.payload = p->payload; a.payload_cap = p->payload_cap; a.payload_len = p->payload_len; a.mb_bits = p->mb_bits;
    a.abort_flag = abort_flag;
    a.mb_w = mb_w; a.mb_h = mb_h; a.slice_type = p->slice_type; a.n_ref0 = p->n_ref0; a.psub8x8 = (p->analyse_inter & 0x20) != 0;
    a.t8_mode = p->transform8x8 != 0; a.profile_high = p->transform8x8 != 0 || p->cqm_custom != 0;
    a.margin = margin;
}
// The writer's work arrays.  On the device the kernel places the record in LDS (one lane works: they live there, not in scratch) and
// hands it on as an LDS pointer; on the host it is an ordinary object.
struct CvWork {
    int level[16], run[16];                      // cv_residual: the block's non-zero levels and the zero runs before them
    int cmvx[2][40], cmvy[2][40];                // the motion cache of x264_macroblock_cache_load per list: x264_scan8 layout, 5 rows x 8
    i16 blk[16];                                 // one 4x4 block's levels in coding order
    signed char cref[2][40];
    u8 cn[48];                                   // this macroblock's coefficient totals and its neighbours' (0x80: none), x264_scan8 layout
    u8 top_nnz[CV_MAX_W][8], left_nnz[8];        // the row above and the left macroblock: totals of 4 luma + 2 Cb + 2 Cr blocks per side
};
#ifdef X264HIP_HOST_TEST
typedef CvWork *CvWorkP;
#define CV_RES_FN static
#define CV_ABORT(flag_) (++*(flag_))
#else
typedef __attribute__((address_space(3))) CvWork *CvWorkP;
#define CV_RES_FN __device__
#define CV_ABORT(flag_) atomicAdd(flag_, 1)
#endif

struct CvBs { u8 *p; unsigned long long acc; int n; };                 // bits not yet stored, MSB first
MB_FN void cv_put(CvBs &b, int n, u32 v)
{
    b.acc = (b.acc << n) | (v & ((n >= 32) ? 0xffffffffu : ((1u << n) - 1u)));
    b.n += n;
    while (b.n >= 8) { *b.p++ = (u8)(b.acc >> (b.n - 8)); b.n -= 8; }
}
MB_FN void cv_ue(CvBs &b, u32 v)
{   // bs_write_ue_big: Exp-Golomb
    v += 1;
    const int len = v ? 32 - __builtin_clz(v) : 0;
    if (len > 1) cv_put(b, len - 1, 0);
    cv_put(b, len, v);
}
MB_FN void cv_se(CvBs &b, int v) { cv_ue(b, v <= 0 ? (u32)(-2 * v) : (u32)(2 * v - 1)); }
MB_FN void cv_te(CvBs &b, int x, int v) { if (x == 1) cv_put(b, 1, v ^ 1); else cv_ue(b, (u32)v); }
MB_FN void cv_vlc(CvBs &b, unsigned short e) { cv_put(b, e & 0xff, (u32)(e >> 8)); }

// one residual block: block_residual_write_cavlc.  l: the block's coefficients in scan order (count of them), nC already predicted.
CV_RES_FN int cv_residual(CvBs &b, CvWorkP w, const i16 *l, int count, int nc_class, bool chroma_dc, int profile_high)
{
    int last = count - 1;
    while (last >= 0 && l[last] == 0) last--;
    if (last < 0) { cv_vlc(b, c_cv_coeff0[nc_class]); return 0; }
    auto level = w->level, run = w->run;
    int total = 0, i_last = last;
    do {
        int r = 0;
        level[total] = l[i_last];
        while (--i_last >= 0 && l[i_last] == 0) r++;
        run[total++] = r;
    } while (i_last >= 0);
    int total_zero = last + 1 - total;
    int trailing = 0;
    while (trailing < 3 && trailing < total && (level[trailing] == 1 || level[trailing] == -1)) trailing++;
    u32 sign = 0;
    for (int i = 0; i < trailing; i++) sign = (sign << 1) | (level[i] < 0);
    cv_vlc(b, c_cv_coeff[nc_class * 64 + total * 4 + trailing - 4]);
    int suffix = total > 10 && trailing < 3;
    if (trailing > 0) cv_put(b, trailing, sign);
    for (int i = trailing; i < total; i++) {
        int val = level[i];
        if (i == trailing && trailing < 3) val -= (val >> 31) | 1;        // the first level after fewer than three trailing ones cannot be +-1
        // x264_level_token[suffix][val] (R/common/vlc.c:874-915) / block_residual_write_cavlc_escape beyond the table
        const int orig = level[i];
        const int mask = val >> 31, abs_level = (val ^ mask) - mask;
        int code = abs_level * 2 - mask - 2;
        const bool in_table = (unsigned)(orig + 64) < 128u && (unsigned)(val + 64) < 128u;
        if (in_table) {
            if ((code >> suffix) < 14) cv_put(b, (code >> suffix) + 1 + suffix, (1u << suffix) + (code & ((1 << suffix) - 1)));
            else if (suffix == 0 && code < 30) cv_put(b, 19, (1u << 4) + (code - 14));
            else if (suffix > 0 && (code >> suffix) == 14) cv_put(b, 15 + suffix, (1u << suffix) + (code & ((1 << suffix) - 1)));
            else { code -= 15 << suffix; if (suffix == 0) code -= 15; cv_put(b, 28, (1u << 12) + code); }
        } else {
            int prefix = 15;
            if ((code >> suffix) < 15) cv_put(b, (code >> suffix) + 1 + suffix, (1u << suffix) + (code & ((1 << suffix) - 1)));
            else {
                code -= 15 << suffix;
                if (suffix == 0) code -= 15;
                if (code >= 1 << 12) {
                    if (profile_high) while (code > 1 << (prefix - 3)) { code -= 1 << (prefix - 3); prefix++; }
                    else code = (1 << 12) - 2 + (code & 1);
                }
                cv_put(b, prefix + 1, 1);
                cv_put(b, prefix - 3, code & ((1 << (prefix - 3)) - 1));
            }
        }
        // i_next: by the ORIGINAL level (x264_level_token[..][val_original].i_next; the escape computes it from the adjusted one)
        const int a2 = in_table ? (orig < 0 ? -orig : orig) : abs_level;
        if (suffix == 0) suffix++;
        if (a2 > (3 << (suffix - 1)) && suffix < 6) suffix++;
    }
    if (total < count) cv_vlc(b, chroma_dc ? c_cv_total_zeros_dc[(total - 1) * 4 + total_zero] : c_cv_total_zeros[(total - 1) * 16 + total_zero]);
    for (int i = 0; i < total - 1 && total_zero > 0; i++) {
        const int zl = total_zero - 1 < 6 ? total_zero - 1 : 6;
        cv_vlc(b, c_cv_run_before[zl * 16 + run[i]]);
        total_zero -= run[i];
    }
    return total;
}

// one slice: chain bz's, by the one lane that calls (inlined into both kernels: the arguments stay where the kernel has them)
MB_FN void cv_write_slice(const CvArgs &a, const int bz, CvWorkP w)
{
    const int n = a.mb_w * a.mb_h;
    const size_t cb = (size_t)n * bz;
    u8 *out = a.payload + (size_t)bz * a.payload_cap + 64;
    CvBs b = {out, 0ull, 0};
    const u8 *limit = out + a.payload_cap - 64 - a.margin;
    int skip_run = 0, last_qp = a.slice_qp;                                  // h->mb.i_last_qp (x264_slice_write starts it at the slice's QP)
    const bool is_b = a.slice_type == 1, is_p = a.slice_type == 0 || is_b;     // is_p: "has skip runs and list 0" in what follows
    for (int mb = 0; mb < n; mb++) {
        const int mbx = mb % a.mb_w, mby = mb / a.mb_w;
        const size_t M = cb + mb;
        const int type = a.mb_type[M];
        auto tn = w->top_nnz[mbx], ln = w->left_nnz, cn = w->cn;
        // what the slice type cannot hold (I_PCM is not built) ends the slice like a slot too small
        const bool known = type >= 0 && (type < T_I_PCM || (is_b ? type >= T_B_DIRECT && type <= T_B_SKIP : is_p && type >= T_P_L0 && type <= T_P_SKIP));
        if (b.p > limit || !known) { CV_ABORT(a.abort_flag); a.payload_len[bz] = 0; return; }
        if (IS_SKIP_T(type)) {
            skip_run++;
            last_qp = a.qp[M];                                                 // x264_macroblock_cache_save: every macroblock leaves its QP (a skipped one: the previous)
            for (int k = 0; k < 8; k++) { tn[k] = 0; ln[k] = 0; }
            if (a.mb_bits) a.mb_bits[M] = (int)((b.p - out) * 8 + b.n);
            continue;
        }
        if (is_p) { cv_ue(b, (u32)skip_run); skip_run = 0; }
        const int off = is_b ? 23 : is_p ? 5 : 0;
        const int cbp = a.cbp[M], cbp_luma = cbp & 15, cbp_chroma = (cbp >> 4) & 3, t8 = a.t8[M];
        const bool has_left = mbx > 0, has_top = mby > 0;
        // ---- type, prediction, vectors ----
        if (type == T_I_4x4 || type == T_I_8x8) {
            cv_ue(b, (u32)off);
            if (a.t8_mode) cv_put(b, 1, (u32)(type == T_I_8x8));
            const signed char *mine = a.i4mode + M * 16;
            // the mode of 4x4 block (bx, by) of macroblock Mn; one that is not I_4x4 / I_8x8 counts as DC
            auto mode_at = [&](size_t Mn, int bx, int by) -> int {
                const int tn_ = a.mb_type[Mn];
                if (tn_ != T_I_4x4 && tn_ != T_I_8x8) return 2;
                return a.i4mode[Mn * 16 + (bx & 1) + ((by & 1) << 1) + ((bx >> 1) << 2) + ((by >> 1) << 3)];
            };
            for (int i = 0; i < 16; i += (type == T_I_8x8 ? 4 : 1)) {
                const int s8 = mb_scan8(i), x = (s8 & 7) - 4, y = (s8 >> 3) - 1;
                const int left = x > 0 ? mode_at(M, x - 1, y) : has_left ? mode_at(M - 1, 3, y) : -1;
                const int top = y > 0 ? mode_at(M, x, y - 1) : has_top ? mode_at(M - a.mb_w, x, 3) : -1;
                const int pred = mb_pred_i4mode(left, top), mode = mb_fix4(mine[i]);
                if (pred == mode) cv_put(b, 1, 1);
                else cv_put(b, 4, (u32)(mode - (mode > pred)));
            }
            cv_ue(b, (u32)mb_fix8c(a.chroma_mode[M]));
        } else if (type == T_I_16x16) {
            cv_ue(b, (u32)(off + 1 + mb_fix16(a.i16mode[M]) + cbp_chroma * 4 + (cbp_luma == 0 ? 0 : 12)));
            cv_ue(b, (u32)mb_fix8c(a.chroma_mode[M]));
        } else {
            // the motion cache for each list the slice has, then x264_mb_predict_mv per partition.  The state holds what
            // x264_macroblock_cache_save left: reference -1 and vector 0 where a block does not use the list, the direct vectors and
            // references in B_SKIP / B_DIRECT macroblocks and direct sub-blocks.
            for (int l = 0; l <= (int)is_b; l++) {
                auto cref = w->cref[l];
                auto cmvx = w->cmvx[l], cmvy = w->cmvy[l];
                const signed char *sref = l ? a.ref1 : a.ref;
                const i16 *smv = l ? a.mv1 : a.mv;
                for (int k = 0; k < 40; k++) { cref[k] = -2; cmvx[k] = cmvy[k] = 0; }
                auto load_nb = [&](size_t Mn, int pos, int bx, int by) {      // neighbour macroblock's 4x4 block (bx, by) -> cache position
                    const int tn_ = a.mb_type[Mn];
                    if (tn_ < T_P_L0) { cref[pos] = -1; return; }             // intra: reference -1, vector 0
                    cref[pos] = sref[Mn * 4 + (bx >> 1) + (by >> 1) * 2];
                    cmvx[pos] = smv[(Mn * 16 + by * 4 + bx) * 2]; cmvy[pos] = smv[(Mn * 16 + by * 4 + bx) * 2 + 1];
                };
                if (has_top) for (int x = 0; x < 4; x++) load_nb(M - a.mb_w, 4 + x, x, 3);
                if (has_top && has_left) load_nb(M - a.mb_w - 1, 3, 3, 3);
                if (has_top && mbx < a.mb_w - 1) load_nb(M - a.mb_w + 1, 8, 0, 3);
                if (has_left) for (int y = 0; y < 4; y++) load_nb(M - 1, 11 + 8 * y, 3, y);
                for (int y = 0; y < 4; y++)
                    for (int x = 0; x < 4; x++) {
                        const int pos = 12 + x + 8 * y;
                        cref[pos] = sref[M * 4 + (x >> 1) + (y >> 1) * 2];
                        cmvx[pos] = smv[(M * 16 + y * 4 + x) * 2]; cmvy[pos] = smv[(M * 16 + y * 4 + x) * 2 + 1];
                    }
                // what the decoder has not reached when it predicts: the positions right of blocks 5, 7 and 13 (R/common/macroblock.c:1050-1052)
                cref[mb_scan8(5) + 1] = cref[mb_scan8(7) + 1] = cref[mb_scan8(13) + 1] = -2;
            }
            const auto cref = w->cref[0];
            const int part = a.partition[M];
            auto mvd_l = [&](int l, int idx, int width) {                      // cavlc_mb_mvd
                int px, py;
                mb_predict_mv([&](int k) -> int { return w->cref[l][k]; }, [&](int k) -> int { return w->cmvx[l][k]; },
                              [&](int k) -> int { return w->cmvy[l][k]; }, part, idx, width, px, py);
                const int i8 = mb_scan8(idx);
                cv_se(b, w->cmvx[l][i8] - px); cv_se(b, w->cmvy[l][i8] - py);
            };
            auto mvd = [&](int idx, int width) { mvd_l(0, idx, width); };
            if (type == T_P_L0) {
                if (part == D_16x16) {
                    cv_ue(b, 0);
                    if (a.n_ref0 > 1) cv_te(b, a.n_ref0 - 1, cref[mb_scan8(0)]);
                    mvd(0, 4);
                } else if (part == D_16x8) {
                    cv_ue(b, 1);
                    if (a.n_ref0 > 1) { cv_te(b, a.n_ref0 - 1, cref[mb_scan8(0)]); cv_te(b, a.n_ref0 - 1, cref[mb_scan8(8)]); }
                    mvd(0, 4); mvd(8, 4);
                } else {
                    cv_ue(b, 2);
                    if (a.n_ref0 > 1) { cv_te(b, a.n_ref0 - 1, cref[mb_scan8(0)]); cv_te(b, a.n_ref0 - 1, cref[mb_scan8(4)]); }
                    mvd(0, 2); mvd(4, 2);
                }
            } else if (type == T_B_DIRECT)
                cv_ue(b, 0);
            else if (type == T_B_8x8) {                                        // R/encoder/cavlc.c:462-483; x264 codes no B partition below 8x8
                cv_ue(b, 22);
                const signed char *sub = a.sub_partition + M * 4;
                for (int i = 0; i < 4; i++) {
                    const int sp = sub[i];
                    if (sp != D_DIRECT_8x8 && sp != D_L0_8x8 && sp != D_L1_8x8 && sp != D_BI_8x8) { CV_ABORT(a.abort_flag); a.payload_len[bz] = 0; return; }
                    cv_ue(b, sp == D_DIRECT_8x8 ? 0u : sp == D_L0_8x8 ? 1u : sp == D_L1_8x8 ? 2u : 3u);      // sub_mb_type, H.264 table 7-18
                }
                // ref_idx of list 0 (te() against the list's size: nothing when it holds one picture); list 1 holds one picture here
                if (a.n_ref0 > 1)
                    for (int i = 0; i < 4; i++) if (SUB_USES(sub[i], 0)) cv_te(b, a.n_ref0 - 1, cref[mb_scan8(4 * i)]);
                for (int l = 0; l < 2; l++)
                    for (int i = 0; i < 4; i++) if (SUB_USES(sub[i], l)) mvd_l(l, 4 * i, 2);
            } else if (type > T_B_DIRECT && type < T_B_8x8) {                  // :484-556: the B types with explicit lists
                if (part != D_16x16 && part != D_16x8 && part != D_8x16) { CV_ABORT(a.abort_flag); a.payload_len[bz] = 0; return; }
                const int t = type - T_B_L0_L0;
                cv_ue(b, part == D_16x16 ? (u32)(1 + t / 4) : (u32)(d_cv_b_type_16x8[t] + (part == D_8x16)));
                const int np = part == D_16x16 ? 1 : 2, step = part == D_16x8 ? 8 : 4, width = part == D_8x16 ? 2 : 4;
                if (a.n_ref0 > 1)
                    for (int i = 0; i < np; i++) if (B_USES(type, 0, i)) cv_te(b, a.n_ref0 - 1, cref[mb_scan8(step * i)]);
                for (int l = 0; l < 2; l++)
                    for (int i = 0; i < np; i++) if (B_USES(type, l, i)) mvd_l(l, step * i, width);
            } else {
                const bool all0 = (cref[mb_scan8(0)] | cref[mb_scan8(4)] | cref[mb_scan8(8)] | cref[mb_scan8(12)]) == 0;
                cv_ue(b, all0 ? 4u : 3u);
                const signed char *sub = a.sub_partition + M * 4;
                if (a.psub8x8) { for (int i = 0; i < 4; i++) { const int sp = sub[i]; cv_ue(b, sp == D_L0_8x8 ? 0u : sp == D_L0_8x4 ? 1u : sp == D_L0_4x8 ? 2u : 3u); } }
                else cv_put(b, 4, 0xf);
                if (!all0 && a.n_ref0 > 1) for (int i = 0; i < 4; i++) cv_te(b, a.n_ref0 - 1, cref[mb_scan8(4 * i)]);
                for (int i = 0; i < 4; i++) {
                    const int sp = sub[i];
                    if (sp == D_L0_8x8) mvd(4 * i, 2);
                    else if (sp == D_L0_8x4) { mvd(4 * i, 2); mvd(4 * i + 2, 2); }
                    else if (sp == D_L0_4x8) { mvd(4 * i, 1); mvd(4 * i + 1, 1); }
                    else { mvd(4 * i, 1); mvd(4 * i + 1, 1); mvd(4 * i + 2, 1); mvd(4 * i + 3, 1); }
                }
            }
        }
        // ---- coded block pattern, transform size ----
        if (type == T_I_4x4 || type == T_I_8x8) cv_ue(b, c_cv_cbp_intra[(cbp_chroma << 4) | cbp_luma]);
        else if (type != T_I_16x16) cv_ue(b, c_cv_cbp_inter[(cbp_chroma << 4) | cbp_luma]);
        if (a.t8_mode && cbp_luma) {                                           // x264_mb_transform_8x8_allowed
            bool allowed = type == T_P_L0 || (type >= T_B_DIRECT && type <= T_B_8x8);       // (B_DIRECT and B_8x8: sps->b_direct8x8_inference is 1)
            if (type == T_P_8x8) { const signed char *sub = a.sub_partition + M * 4; allowed = sub[0] == D_L0_8x8 && sub[1] == D_L0_8x8 && sub[2] == D_L0_8x8 && sub[3] == D_L0_8x8; }
            if (allowed) cv_put(b, 1, (u32)t8);
        }
        // ---- residual ----
        // the nnz cache of this macroblock: neighbours' totals, own totals as they are written
        for (int k = 0; k < 48; k++) cn[k] = 0;
        for (int k = 0; k < 4; k++) { cn[4 + k] = has_top ? tn[k] : 0x80; cn[11 + 8 * k] = has_left ? ln[k] : 0x80; }
        for (int k = 0; k < 2; k++) {
            cn[1 + k] = has_top ? tn[4 + k] : 0x80; cn[8 + 8 * k] = has_left ? ln[4 + k] : 0x80;                 // Cb: scan8[16] = 1 + 8 * 1
            cn[1 + 8 * 3 + k] = has_top ? tn[6 + k] : 0x80; cn[8 * 4 + 8 * k] = has_left ? ln[6 + k] : 0x80;     // Cr: scan8[20] = 1 + 8 * 4
        }
        auto nc_of = [&](int idx) -> int {
            const int s8 = mb_scan8(idx);
            int r = cn[s8 - 1] + cn[s8 - 8];
            if (r < 0x80) r = (r + 1) >> 1;
            r &= 0x7f;
            return r < 2 ? 0 : r < 4 ? 1 : r < 8 ? 2 : 3;
        };
        const bool coded = type == T_I_16x16 || cbp_luma || cbp_chroma;
        if (coded) {                                                           // cavlc_qp_delta: the state's QP already has the rules applied (an empty I_16x16 took the previous one)
            int dqp = a.qp[M] - last_qp;
            if (dqp < -26) dqp += 52; else if (dqp > 25) dqp -= 52;
            cv_se(b, dqp);
        }
        last_qp = a.qp[M];
        const i16 *ly = a.luma + M * 256;
        if (type == T_I_16x16) {
            cv_residual(b, w, a.luma_dc + M * 16, 16, nc_of(0), false, a.profile_high);
            if (cbp_luma)
                for (int i = 0; i < 16; i++) cn[mb_scan8(i)] = (u8)cv_residual(b, w, ly + 16 * i + 1, 15, nc_of(i), false, a.profile_high);
        } else if (cbp_luma | cbp_chroma) {
            for (int i8 = 0; i8 < 4; i8++) {
                if (!(cbp_luma >> i8 & 1)) continue;
                for (int i4 = 0; i4 < 4; i4++) {
                    const int i = 4 * i8 + i4;
                    auto blk = w->blk;
                    if (t8) for (int j = 0; j < 16; j++) blk[j] = ly[64 * i8 + i4 + 4 * j];        // zigzag_interleave_8x8_cavlc
                    else for (int j = 0; j < 16; j++) blk[j] = ly[16 * i + j];
                    cn[mb_scan8(i)] = (u8)cv_residual(b, w, (const i16 *)blk, 16, nc_of(i), false, a.profile_high);
                }
            }
        }
        if (cbp_chroma) {
            cv_residual(b, w, a.chroma_dc + M * 8, 4, 4, true, a.profile_high);
            cv_residual(b, w, a.chroma_dc + M * 8 + 4, 4, 4, true, a.profile_high);
            if (cbp_chroma & 2)
                for (int i = 16; i < 24; i++) cn[mb_scan8(i)] = (u8)cv_residual(b, w, a.chroma_ac + M * 128 + 16 * (i - 16) + 1, 15, nc_of(i), false, a.profile_high);
        }
        // what the neighbours to come read: this macroblock's bottom row and right column
        for (int k = 0; k < 4; k++) { tn[k] = cn[12 + 8 * 3 + k]; ln[k] = cn[12 + 3 + 8 * k]; }
        for (int k = 0; k < 2; k++) {
            tn[4 + k] = cn[1 + 8 * 2 + k]; ln[4 + k] = cn[2 + 8 * 1 + 8 * k];
            tn[6 + k] = cn[1 + 8 * 5 + k]; ln[6 + k] = cn[2 + 8 * 4 + 8 * k];
        }
        if (a.mb_bits) a.mb_bits[M] = (int)((b.p - out) * 8 + b.n);
    }
    if (is_p && skip_run > 0) cv_ue(b, (u32)skip_run);
    cv_put(b, 1, 1);                                                           // bs_rbsp_trailing
    if (b.n) cv_put(b, 8 - b.n, 0);
    a.payload_len[bz] = (int)(b.p - out);
}
