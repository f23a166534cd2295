// cavlc_dev.h -- the CAVLC slice writer of frame_cavlc.hip's kernels (x264_macroblock_write_cavlc with block_residual_write_cavlc and
// the skip runs of x264_slice_write, R/encoder/cavlc.c:60-620, R/encoder/encoder.c:1200-1280): serial code of one lane over the plain
// arrays of an x264hip_mb_state.  Like cabac_dev.h the file is plain C++ over mb_vocab.h, and the same text compiles for the host
// (-DX264HIP_HOST_TEST): tests/cavlc_host.cpp runs it there on the reference's arrays against the reference's bytes, no GPU needed.
// Behind the serial writer (cv_write_slice, the yardstick) the file holds the macroblock-parallel form: one macroblock's bits as a function
// of the state arrays (cv_mb), in a COUNTING mode that returns the bit length and stores nothing and a PLACING mode that writes the bits at a
// given offset -- the syntax text is the same, the sink is its template argument (tests/cavlc_mp_host.cpp drives both on the host).  The
// counting mode is the twin of the writer R/encoder/rdo.c:28-60 prices CAVLC bits with; the RD trials that would call it are not built, and
// CAVLC under the RD levels is still refused.
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

// Where the bits go is the syntax text's template argument B: three sinks take cv_put.
//   CvBs   the serial writer's: bytes stored one after the other from the slot's first
//   CvCnt  counting: the bit length and nothing else -- no byte is stored
//   CvPl   placing: the bits at a given bit offset of the slot, beside neighbours that write the bytes around them at the same time
struct CvBs { u8 *p; unsigned long long acc; int n; };                 // bits not yet stored, MSB first
MB_FN void cv_put(CvBs &b, int n, u32 v)
{
    b.acc = (b.acc << n) | (v & ((n >= 32) ? 0xffffffffu : ((1u << n) - 1u)));
    b.n += n;
    while (b.n >= 8) { *b.p++ = (u8)(b.acc >> (b.n - 8)); b.n -= 8; }
}
struct CvCnt { int bits; };
MB_FN void cv_put(CvCnt &b, int n, u32) { b.bits += n; }
// CvPl collects 32-bit words at 4-byte-aligned addresses (wp; n: bits of the current word that are decided, those in front of the start
// offset among them, as zeros).  A word that holds nothing but this sink's bits is stored; the first and the last word may also hold a
// neighbour's bits and are merged with OR -- an atomic one on the device -- into bytes the pass has zeroed (cv_mp: phase 2).  The OR
// carries zeros for every bit that is not this sink's, so the bytes of such a word that are not the slice's keep their values -- but on the
// device they are READ AND WRITTEN BACK by the 4-byte atomic (the host form ORs byte by byte and touches only bytes it has a bit for, so a
// host sanitizer run does not see this).  Which bytes: the last word ends at most 3 bytes behind the slice, inside the slot -- the space check
// leaves margin - (a macroblock's worst case + the slice's end) = 2624 - 2604 = 20 bytes free behind the last element; the first word begins
// at the slice's first byte when the slot's start (payload + chain * payload_cap + 64) is a multiple of 4, as it is for every payload_cap
// that is one, and otherwise up to 3 bytes in front of it, in the slot's own X264HIP_PAYLOAD_LEAD bytes.  No word reaches another slot.
struct CvPl { u8 *wp; unsigned long long acc; int n; bool shared; };
MB_FN void cv_pl_word(u8 *wp, u32 bits, bool shared)
{
#ifdef X264HIP_HOST_TEST
    (void)shared;
    for (int i = 0; i < 4; i++) { const u8 v = (u8)(bits >> (24 - 8 * i)); if (v) wp[i] |= v; }       // (touches no byte it has no bit for)
#else
    const u32 v = __builtin_bswap32(bits);
    if (!shared) *(u32 *)wp = v;
    else if (v) atomicOr((u32 *)wp, v);
#endif
}
MB_FN void cv_pl_begin(CvPl &b, u8 *out, int start_bits)
{
    u8 *p = out + (start_bits >> 3);
    const int lead = (int)((size_t)p & 3);
    b.wp = p - lead; b.acc = 0ull; b.n = lead * 8 + (start_bits & 7); b.shared = b.n > 0;
}
MB_FN void cv_put(CvPl &b, int n, u32 v)
{
    b.acc = (b.acc << n) | (v & ((n >= 32) ? 0xffffffffu : ((1u << n) - 1u)));
    b.n += n;
    while (b.n >= 32) { cv_pl_word(b.wp, (u32)(b.acc >> (b.n - 32)), b.shared); b.wp += 4; b.n -= 32; b.shared = false; }
}
MB_FN void cv_pl_end(CvPl &b) { if (b.n > 0) cv_pl_word(b.wp, (u32)(b.acc << (32 - b.n)), true); }

template <class B> MB_FN void cv_ue(B &b, u32 v)
{   // bs_write_ue_big: Exp-Golomb
    v += 1;
    const int len = v ? 32 - __builtin_clz(v) : 0;
    if (len > 1) cv_put(b, len - 1, 0);
    cv_put(b, len, v);
}
template <class B> MB_FN void cv_se(B &b, int v) { cv_ue(b, v <= 0 ? (u32)(-2 * v) : (u32)(2 * v - 1)); }
template <class B> MB_FN void cv_te(B &b, int x, int v) { if (x == 1) cv_put(b, 1, v ^ 1); else cv_ue(b, (u32)v); }
template <class B> MB_FN void cv_vlc(B &b, unsigned short e) { cv_put(b, e & 0xff, (u32)(e >> 8)); }

// one residual block: block_residual_write_cavlc.  l: the block's coefficients in scan order (count of them), nC already predicted.
// w: the work arrays level[16] and run[16] (CvWork's, or a lane's CvWorkMp)
template <class B, class W> CV_RES_FN int cv_residual(B &b, W w, const i16 *l, int count, int nc_class, bool chroma_dc, int profile_high)
{
    int last = count - 1;
    while (last >= 0 && l[last] == 0) last--;
    if (last < 0) { cv_vlc(b, c_cv_coeff0[nc_class]); return 0; }
    auto level = w->level;
    auto run = w->run;
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

// one slice: chain bz's, by the one lane that calls (inlined into both kernels: the arguments stay where the kernel has them).
// THE MACROBLOCK'S SYNTAX BELOW HAS A TWIN: cv_mb (further down) states the same type / prediction / vector, cbp, transform flag, qp delta and
// residual text for the macroblock-parallel pass, with this loop's running values as lookups.  A change of syntax here is made there as well;
// tests/test_cavlc_mp_host.py compares the two byte for byte and fails when they part.  (This writer stays a text of its own for now because
// it is what the new pass is measured against; folding it into a loop over cv_mb<CvBs> is the follow-up once the new pass is the default.)
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

// ---- The macroblock-parallel form: count, scan, place ---------------------------------------------------------------------------------
// CAVLC has no adaptive state: a macroblock's bits are a function of the state arrays, and only their POSITION in the slice is serial -- a
// prefix sum of the lengths.  cv_mb below is cv_write_slice's per-macroblock text with every running value restated as something
// macroblock n can look up in any order:
//   nC's neighbour totals   cv_write_slice keeps the totals of the row above and of the left macroblock as it goes.  Here a short first
//                           phase fills a side array of 24 bytes per macroblock (cv_total: 16 luma, 4 Cb, 4 Cr; 0 outside the cbp and in
//                           skipped macroblocks, 16 in I_PCM) and cv_mb reads the neighbours' entries from it.  The alternative -- each
//                           macroblock recounting its two neighbours' 16 border blocks from their levels -- reads 512 bytes per macroblock
//                           twice over (count and place) where the side array reads 16, and was not built.
//   vectors, modes, refs    from the neighbours' entries of the state arrays, as cv_write_slice derives them already
//   mb_qp_delta's base      qp[n - 1], slice_qp for n = 0: cv_write_slice's last_qp takes a.qp[M] after EVERY macroblock, skipped ones
//                           included, and carries nothing the array does not hold
//   mb_skip_run             the skipped macroblocks directly before n: a segmented scan over the lengths (a skipped macroblock has none),
//                           made in the scan phase together with the prefix sum; the run's code is added to the next coded macroblock's
//                           length there (cv_skip_run_bits) and written in front of it in the place phase (cv_skip_run).  The run that ends
//                           the slice and the rbsp trailing bits are element n_mb of the scan (cv_slice_end).
// Two modes over the one text: cv_mb<CvCnt> returns the length and stores nothing, cv_mb<CvPl> writes the bits at the scanned offset.  The
// counting mode is the "counting twin" R/encoder/rdo.c prices CAVLC bits with; CAVLC under the RD levels itself is still refused.
// Scratch per slice (cv_mp_scratch): int off[n_mb + 1] -- lengths after the count, inclusive end offsets in bits after the scan --,
// int run[n_mb + 1], u8 tot[n_mb][24].

// a lane's work arrays: CvWork's without the row buffer, in the narrowest types that hold the values (levels and vectors are int16 in the
// state, a run is at most 15).  133 dwords: an odd stride, so the 64 lanes' records of one wavefront start in different LDS banks.
struct CvWorkMp {
    i16 level[16]; u8 run[16];
    i16 cmvx[2][40], cmvy[2][40];
    i16 blk[16];
    signed char cref[2][40];
    u8 cn[48];
    u8 pad[4];
};
#ifdef X264HIP_HOST_TEST
typedef CvWorkMp *CvWorkMpP;
#define CV_HD static inline
#else
#define CV_HD static inline __host__ __device__
typedef __attribute__((address_space(3))) CvWorkMp *CvWorkMpP;
#endif

struct CvMpScratch { int *off, *run; u8 *tot; };
CV_HD size_t cv_mp_scratch_bytes(int n_mb) { return ((size_t)8 * (n_mb + 1) + (size_t)24 * n_mb + 63) & ~(size_t)63; }
CV_HD CvMpScratch cv_mp_scratch(void *base, int slice, int n_mb)
{
    u8 *p = (u8 *)base + cv_mp_scratch_bytes(n_mb) * (size_t)slice;
    CvMpScratch s = {(int *)p, (int *)p + (n_mb + 1), p + (size_t)8 * (n_mb + 1)};
    return s;
}
MB_FN int cv_blk_index(int x, int y) { return (x & 1) + ((y & 1) << 1) + ((x >> 1) << 2) + ((y >> 1) << 3); }      // the 4x4 block at (x, y)

// entry k of macroblock M's totals: what block_residual_write_cavlc leaves in non_zero_count for block k (0..15 luma, 16..19 Cb, 20..23 Cr)
MB_FN int cv_total(const CvArgs &a, size_t M, int k)
{
    const int type = a.mb_type[M];
    if (type == T_I_PCM) return 16;
    if (type < 0 || IS_SKIP_T(type)) return 0;
    const int cbp = a.cbp[M];
    const i16 *l;
    int first = 0, step = 1;
    if (k < 16) {
        if (type == T_I_16x16) { if (!(cbp & 15)) return 0; l = a.luma + M * 256 + 16 * k; first = 1; }
        else {
            if (!(cbp >> (k >> 2) & 1)) return 0;
            if (a.t8[M]) { l = a.luma + M * 256 + 64 * (k >> 2) + (k & 3); step = 4; }       // zigzag_interleave_8x8_cavlc
            else l = a.luma + M * 256 + 16 * k;
        }
    } else {
        if (!(cbp >> 4 & 2)) return 0;
        l = a.chroma_ac + M * 128 + 16 * (k - 16); first = 1;
    }
    int t = 0;
    for (int j = first; j < 16; j++) t += l[j * step] != 0;
    return t;
}

template <class B> MB_FN void cv_skip_run(B &b, int run) { cv_ue(b, (u32)run); }
MB_FN int cv_skip_run_bits(int run) { CvCnt c = {0}; cv_skip_run(c, run); return c.bits; }
// element n_mb of a slice: the skip run that ends it, bs_rbsp_trailing.  start: the element's bit offset
template <class B> MB_FN void cv_slice_end(B &b, bool is_p, int run, int start)
{
    int pos = start + 1;
    if (is_p && run > 0) { cv_skip_run(b, run); pos += cv_skip_run_bits(run); }
    cv_put(b, 1, 1);
    if (pos & 7) cv_put(b, 8 - (pos & 7), 0);
}
// cv_write_slice's space check, restated on the offsets.  It stops before the first macroblock that starts more than `margin` bytes short
// of the slot's end; starts only grow, so that is a comparison of the last macroblock's.  (A slice that passes the check and is still longer
// than its slot -- only with a margin below a macroblock's worst case, which no entry point sets -- counts as too small as well: nothing is
// placed outside the slot.)
MB_FN bool cv_slot_too_small(const CvArgs &a, int start_last_bits, int total_bytes)
{
    return (start_last_bits >> 3) > a.payload_cap - 64 - a.margin || total_bytes > a.payload_cap - 64;
}

// Macroblock mb of chain bz's slice into sink b, the skip run in front of it excluded; tot: the slice's totals.  Returns 0, or -1 for what ends
// the pass (a type the slice cannot hold, I_PCM, a B partition x264 does not code); a skipped macroblock has no bits.
template <class B, class W> MB_FN int cv_mb(const CvArgs &a, const int bz, const int mb, const u8 *tot, B &b, W w)
{
    const size_t M = (size_t)a.mb_w * a.mb_h * bz + mb;
    const bool is_b = a.slice_type == 1, is_p = a.slice_type == 0 || is_b;
    const int mbx = mb % a.mb_w, mby = mb / a.mb_w;
    const int type = a.mb_type[M];
    const bool known = type >= 0 && (type < T_I_PCM || (is_b ? type >= T_B_DIRECT && type <= T_B_SKIP : is_p && type >= T_P_L0 && type <= T_P_SKIP));
    if (!known) return -1;
    if (IS_SKIP_T(type)) return 0;
    auto cn = w->cn;
    const int off = is_b ? 23 : is_p ? 5 : 0;
    const int cbp = a.cbp[M], cbp_luma = cbp & 15, cbp_chroma = (cbp >> 4) & 3, t8 = a.t8[M];
    const bool has_left = mbx > 0, has_top = mby > 0;
    // ---- type, prediction, vectors ----
    if (type == T_I_4x4 || type == T_I_8x8) {
        cv_ue(b, (u32)off);
        if (a.t8_mode) cv_put(b, 1, (u32)(type == T_I_8x8));
        const signed char *mine = a.i4mode + M * 16;
        auto mode_at = [&](size_t Mn, int bx, int by) -> int {
            const int tn_ = a.mb_type[Mn];
            if (tn_ != T_I_4x4 && tn_ != T_I_8x8) return 2;
            return a.i4mode[Mn * 16 + cv_blk_index(bx, by)];
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
        // the motion cache for each list the slice has (cv_write_slice's, from the same arrays), then x264_mb_predict_mv per partition
        for (int l = 0; l <= (int)is_b; l++) {
            auto cref = w->cref[l];
            auto cmvx = w->cmvx[l], cmvy = w->cmvy[l];
            const signed char *sref = l ? a.ref1 : a.ref;
            const i16 *smv = l ? a.mv1 : a.mv;
            for (int k = 0; k < 40; k++) { cref[k] = -2; cmvx[k] = cmvy[k] = 0; }
            auto load_nb = [&](size_t Mn, int pos, int bx, int by) {
                const int tn_ = a.mb_type[Mn];
                if (tn_ < T_P_L0) { cref[pos] = -1; return; }
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
        else if (type == T_B_8x8) {
            cv_ue(b, 22);
            const signed char *sub = a.sub_partition + M * 4;
            for (int i = 0; i < 4; i++) {
                const int sp = sub[i];
                if (sp != D_DIRECT_8x8 && sp != D_L0_8x8 && sp != D_L1_8x8 && sp != D_BI_8x8) return -1;
                cv_ue(b, sp == D_DIRECT_8x8 ? 0u : sp == D_L0_8x8 ? 1u : sp == D_L1_8x8 ? 2u : 3u);
            }
            if (a.n_ref0 > 1)
                for (int i = 0; i < 4; i++) if (SUB_USES(sub[i], 0)) cv_te(b, a.n_ref0 - 1, cref[mb_scan8(4 * i)]);
            for (int l = 0; l < 2; l++)
                for (int i = 0; i < 4; i++) if (SUB_USES(sub[i], l)) mvd_l(l, 4 * i, 2);
        } else if (type > T_B_DIRECT && type < T_B_8x8) {
            if (part != D_16x16 && part != D_16x8 && part != D_8x16) return -1;
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
    if (a.t8_mode && cbp_luma) {
        bool allowed = type == T_P_L0 || (type >= T_B_DIRECT && type <= T_B_8x8);
        if (type == T_P_8x8) { const signed char *sub = a.sub_partition + M * 4; allowed = sub[0] == D_L0_8x8 && sub[1] == D_L0_8x8 && sub[2] == D_L0_8x8 && sub[3] == D_L0_8x8; }
        if (allowed) cv_put(b, 1, (u32)t8);
    }
    // ---- residual ----
    // the nnz cache: the neighbours' totals from the side array, this macroblock's own as they are written
    const u8 *tt = tot + ((size_t)mb - (has_top ? a.mb_w : 0)) * 24, *tl = tot + ((size_t)mb - (has_left ? 1 : 0)) * 24;
    for (int k = 0; k < 48; k++) cn[k] = 0;
    for (int k = 0; k < 4; k++) { cn[4 + k] = has_top ? tt[cv_blk_index(k, 3)] : 0x80; cn[11 + 8 * k] = has_left ? tl[cv_blk_index(3, k)] : 0x80; }
    for (int k = 0; k < 2; k++) {
        cn[1 + k] = has_top ? tt[16 + 2 + k] : 0x80; cn[8 + 8 * k] = has_left ? tl[16 + 1 + 2 * k] : 0x80;                 // Cb: scan8[16] = 1 + 8 * 1
        cn[1 + 8 * 3 + k] = has_top ? tt[20 + 2 + k] : 0x80; cn[8 * 4 + 8 * k] = has_left ? tl[20 + 1 + 2 * k] : 0x80;     // Cr: scan8[20] = 1 + 8 * 4
    }
    auto nc_of = [&](int idx) -> int {
        const int s8 = mb_scan8(idx);
        int r = cn[s8 - 1] + cn[s8 - 8];
        if (r < 0x80) r = (r + 1) >> 1;
        r &= 0x7f;
        return r < 2 ? 0 : r < 4 ? 1 : r < 8 ? 2 : 3;
    };
    if (type == T_I_16x16 || cbp_luma || cbp_chroma) {                         // cavlc_qp_delta, against the QP the macroblock before this one left
        int dqp = a.qp[M] - (mb ? a.qp[M - 1] : a.slice_qp);
        if (dqp < -26) dqp += 52; else if (dqp > 25) dqp -= 52;
        cv_se(b, dqp);
    }
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
                if (t8) for (int j = 0; j < 16; j++) blk[j] = ly[64 * i8 + i4 + 4 * j];
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
    return 0;
}
