// cabac_pass_dev.h -- the CABAC slice writer as a pass over the plain arrays of an x264hip_mb_state (frame_cabac.hip's kernel): what the
// in-loop writer of slice_sweep_body.h does per macroblock -- cd_encode_terminal, cw_mb_skip, cw_macroblock on a syntax record, cd_encode_flush
// at the slice's end -- with the record (mbsyn.h's MbSyn) rebuilt from the state instead of taken from the sweep's caches.  Like cavlc_dev.h
// the file is plain C++ over mb_vocab.h, mbsyn.h and cabac_dev.h, and the same text compiles for the host (-DX264HIP_HOST_TEST):
// tests/cabac_pass_host.cpp runs it there on the CPU twin's or the reference's arrays against the reference's bytes, no GPU needed.
//
// What the record needs beyond the state is derived as x264_macroblock_cache_load does (R/common/macroblock.c:896-1160):
//   * the motion cache (references and vectors of the macroblock and of its left, top, top-left and top-right neighbours, -2 where there is
//     none, -1 / 0 for an intra neighbour) and from it mvd = mv - x264_mb_predict_mv of every partition and sub-partition; the left
//     macroblock's and the row above's mvd are kept for the context sums of x264_cabac_mb_mvd_cpn;
//   * the neighbours' syntax: type (I_8x8 counts as I_4x4: x264_mb_type_fix), cbp with its DC flags, chroma prediction mode, transform
//     size, the coded-block-flag neighbours nz_l / nz_t / nz_lc / nz_tc (0x80: none), the intra 4x4 mode cache;
//   * h->mb.i_last_qp / i_last_dqp and "the previous macroblock has coefficients" from the state's per-macroblock QP.  The state holds what
//     x264_macroblock_cache_save left (a macroblock without coefficients carries the QP before it); x264_cabac_mb_qp_delta's own side effect
//     -- an I_16x16 macroblock without any coefficient takes the previous QP -- is applied here as well, so a state that does not carry it
//     (a sweep that ran no writer) codes the same bits.
// The record is built in two steps written for many lanes (CP_FOR: every lane takes the entries lane, lane + CP_LANES, ...): cp_fetch loads
// a macroblock's share of the state into registers, cp_commit turns it into the record; the coder in between is one lane's.
#pragma once
#include <string.h>
#include "x264hip.h"
#include "x264hip_lookahead.h"
#include "mb_vocab.h"
#include "cabac_dev.h"

#define CP_MAX_W 512
#define CP_MB_BYTES_MAX 8192           // SW_MB_BYTES_MAX (slice_kernel.h), the in-loop writer's bound on one macroblock: frame_cabac.hip asserts the two equal

struct CpArgs {
    const signed char *mb_type, *partition, *sub_partition, *ref, *i4mode, *i16mode, *chroma_mode, *t8, *qp;
    const i16 *mv, *cbp, *luma, *luma_dc, *chroma_dc, *chroma_ac;
    const u8 *nnz;
    u8 *payload; int payload_cap; int *payload_len, *mb_bits; int *abort_flag, *abort_total;
    int mb_w, mb_h, slice_type, n_ref0, pps_t8, slice_qp, cabac_init_idc, i_frame, i_frame_stride;
};
// the arguments from the ABI's description of one slice of mb_w x mb_h macroblocks per chain (host code)
static inline void cp_args(CpArgs &a, const x264hip_mb_state *st, const x264hip_cabac_params *p, int mb_w, int mb_h, int *abort_flag, int *abort_total)
{
    memset(&a, 0, sizeof(a));
    a.mb_type = (const signed char *)st->mb_type; a.partition = (const signed char *)st->partition; a.sub_partition = (const signed char *)st->sub_partition;
    a.ref = (const signed char *)st->ref; a.i4mode = (const signed char *)st->i4mode; a.i16mode = (const signed char *)st->i16mode;
    a.chroma_mode = (const signed char *)st->chroma_mode; a.t8 = (const signed char *)st->t8; a.qp = (const signed char *)st->qp;
    a.mv = st->mv; a.cbp = st->cbp; a.luma = st->luma; a.luma_dc = st->luma_dc; a.chroma_dc = st->chroma_dc; a.chroma_ac = st->chroma_ac; a.nnz = st->nnz;
    a.payload = p->payload; a.payload_cap = p->payload_cap; a.payload_len = p->payload_len; a.mb_bits = p->mb_bits;
    a.abort_flag = abort_flag; a.abort_total = abort_total;
    // (p->analyse_inter is not read: CABAC codes a P_8x8 macroblock's sub-partition types whether or not PSUB8x8 is analysed; the field keeps the
    // record beside x264hip_cavlc_params)
    a.mb_w = mb_w; a.mb_h = mb_h; a.slice_type = p->slice_type; a.n_ref0 = p->n_ref0; a.pps_t8 = p->transform8x8 != 0;
    a.slice_qp = p->slice_qp; a.cabac_init_idc = p->cabac_init_idc; a.i_frame = p->i_frame; a.i_frame_stride = p->i_frame_stride;
}
// The pass's work arrays: LDS on the device, an ordinary object on the host.
struct CpWork {
    MbSyn rec;                                   // the record the coder walks
    u8 ctx[464];                                 // the 460 context states
    i16 top_mvd[CP_MAX_W][4][2], left_mvd[4][2]; // mvd of the row above's bottom blocks and of the left macroblock's right column
    int stop;                                    // the coder's verdict after a macroblock: the next one might not fit
};
#ifdef X264HIP_HOST_TEST
typedef CpWork *CpWorkP;
typedef MbSyn *CpRecP;
typedef u8 *CpCtxP;
#define CP_LANES 1
#define CP_LANE() 0
#define CP_SYNC() do { } while (0)
#define CP_ABORT(a_) do { *(a_).abort_flag = 1; ++*(a_).abort_total; } while (0)
#define CP_UNROLL
#else
typedef __attribute__((address_space(3))) CpWork *CpWorkP;
typedef __attribute__((address_space(3))) MbSyn *CpRecP;
typedef __attribute__((address_space(3))) u8 *CpCtxP;
#define CP_LANES 64
#define CP_LANE() ((int)threadIdx.x)
#define CP_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local"); __builtin_amdgcn_wave_barrier(); \
                       __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local"); } while (0)
#define CP_ABORT(a_) do { __hip_atomic_store((a_).abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); atomicAdd((a_).abort_total, 1); } while (0)
#define CP_UNROLL _Pragma("unroll")
#endif
// every lane takes the entries lane, lane + CP_LANES, ... of n; j counts a lane's own entries (its slot in a CpFetch array)
#define CP_PER(n_) (((n_) + CP_LANES - 1) / CP_LANES)
#define CP_FOR(j_, k_, n_) CP_UNROLL for (int j_ = 0; j_ < CP_PER(n_); j_++) for (int k_ = lane + j_ * CP_LANES; k_ < (n_); k_ = (n_))

// h->mb.i_last_qp / i_last_dqp / "the previous macroblock has coefficients", carried from macroblock to macroblock (wave-uniform)
struct CpQp { int last_qp, last_dqp, prev_coded; };

// One lane's share of what a macroblock's record is built from, as loaded from the state: registers.  cp_fetch only issues the loads --
// none of its addresses depends on a loaded value -- so they are in flight while lane 0 codes the macroblock before; cp_commit turns
// them into the record once the coder is done with it.
struct CpFetch {
    int type, cbp, t8, qp, part, m16, cpm, sub[4];                       // the macroblock's own scalars (every lane loads them: one address)
    int type_l, type_t, cbp_l, cbp_t, cpm_l, cpm_t, t8_l, t8_t;          // the left and top neighbour's
    int mode[CP_PER(48)], r[CP_PER(48)], vx[CP_PER(48)], vy[CP_PER(48)], nbt[CP_PER(48)];       // cache entry k: intra mode, reference, vector, its macroblock's type
    int nnz[CP_PER(27)], nz_l[CP_PER(4)], nz_t[CP_PER(4)], nz_lc[CP_PER(4)], nz_tc[CP_PER(4)];
    i16 luma[CP_PER(256)], cac[CP_PER(128)], dc[CP_PER(16)], cdc[CP_PER(8)];
};

// index of the 4x4 block at (x, y) in coding order
MB_FN int cp_blk(int x, int y) { return (x & 1) + ((y & 1) << 1) + ((x >> 1) << 2) + ((y >> 1) << 3); }

MB_FN void cp_fetch(const CpArgs &a, const size_t cb, const int mb, CpFetch &f, const int lane)
{
    const int mbx = mb % a.mb_w, mby = mb / a.mb_w;
    const size_t M = cb + mb, L = M - 1, T = M - a.mb_w;
    const bool has_left = mbx > 0, has_top = mby > 0;
    f.type = a.mb_type[M]; f.cbp = a.cbp[M]; f.t8 = a.t8[M]; f.qp = a.qp[M]; f.part = a.partition[M]; f.m16 = a.i16mode[M]; f.cpm = a.chroma_mode[M];
    for (int i = 0; i < 4; i++) f.sub[i] = a.sub_partition[M * 4 + i];
    f.type_l = has_left ? a.mb_type[L] : -1; f.cbp_l = has_left ? a.cbp[L] : -1; f.cpm_l = has_left ? a.chroma_mode[L] : 0; f.t8_l = has_left ? a.t8[L] : 0;
    f.type_t = has_top ? a.mb_type[T] : -1; f.cbp_t = has_top ? a.cbp[T] : -1; f.cpm_t = has_top ? a.chroma_mode[T] : 0; f.t8_t = has_top ? a.t8[T] : 0;
    // the caches, x264_scan8 layout: entry k is the 4x4 block at (x, y), -1 the left / top neighbour's
    CP_FOR(j, k, 48) {
        const int x = (k & 7) - 4, y = (k >> 3) - 1;
        const bool own = x >= 0 && y >= 0 && y < 4, top = y == -1 && x >= 0, left = x == -1 && y >= 0 && y < 4;
        size_t Mn = M; int bx = x, by = y; bool have = own;
        if (top && has_top) { Mn = T; by = 3; have = true; }
        else if (left && has_left) { Mn = L; bx = 3; have = true; }
        else if (k == 3 && has_top && has_left) { Mn = T - 1; bx = 3; by = 3; have = true; }
        else if (k == 8 && has_top && mbx < a.mb_w - 1) { Mn = T + 1; bx = 0; by = 3; have = true; }
        f.mode[j] = -1; f.r[j] = -2; f.vx[j] = f.vy[j] = 0; f.nbt[j] = -1;
        if (have) {
            // intra4x4_pred_mode (the state holds I_PRED_4x4_DC for every macroblock that is not I_4x4 / I_8x8; the corner entries are never read)
            f.mode[j] = a.i4mode[Mn * 16 + cp_blk(bx, by)];
            f.nbt[j] = a.mb_type[Mn];
            if (a.slice_type == 0) { f.r[j] = a.ref[Mn * 4 + (bx >> 1) + (by >> 1) * 2]; f.vx[j] = a.mv[(Mn * 16 + by * 4 + bx) * 2]; f.vy[j] = a.mv[(Mn * 16 + by * 4 + bx) * 2 + 1]; }
        }
    }
    CP_FOR(j, k, 27) f.nnz[j] = a.nnz[M * 27 + k];
    CP_FOR(j, k, 4) {
        f.nz_l[j] = has_left ? a.nnz[L * 27 + (k == 0 ? 5 : k == 1 ? 7 : k == 2 ? 13 : 15)] : 0x80;
        f.nz_t[j] = has_top ? a.nnz[T * 27 + (k == 0 ? 10 : k == 1 ? 11 : k == 2 ? 14 : 15)] : 0x80;
        f.nz_lc[j] = has_left ? a.nnz[L * 27 + 16 + 4 * (k >> 1) + 1 + 2 * (k & 1)] : 0x80;
        f.nz_tc[j] = has_top ? a.nnz[T * 27 + 16 + 4 * (k >> 1) + 2 + (k & 1)] : 0x80;
    }
    CP_FOR(j, k, 256) f.luma[j] = a.luma[M * 256 + k];
    CP_FOR(j, k, 128) f.cac[j] = a.chroma_ac[M * 128 + k];
    CP_FOR(j, k, 16) f.dc[j] = a.luma_dc[M * 16 + k];
    CP_FOR(j, k, 8) f.cdc[j] = a.chroma_dc[M * 8 + k];
}

// The record of macroblock `mb` from what cp_fetch loaded, by all lanes; q: the QP state before this macroblock on entry, after it on
// return (every lane computes the same).
MB_FN void cp_commit(const CpArgs &a, const int mb, const CpFetch &f, CpRecP m, CpWorkP w, CpQp &q, const int lane)
{
    const int mbx = mb % a.mb_w, mby = mb / a.mb_w;
    const bool has_left = mbx > 0, has_top = mby > 0, is_p = a.slice_type == 0;
    const int type = f.type, cbp = f.cbp;
    const bool i48 = type == T_I_4x4 || type == T_I_8x8, inter = type == T_P_L0 || type == T_P_8x8;
    // ---- scalars: one lane ----
    if (lane == 0) {
        m->slice_type = a.slice_type; m->type = type; m->partition = f.part;
        m->i16mode = f.m16; m->chroma_mode = f.cpm; m->cbp_luma = cbp & 15; m->cbp_chroma = (cbp >> 4) & 3; m->t8 = f.t8; m->qp = f.qp;
        m->n_ref = a.n_ref0; m->n_ref1 = 0; m->pps_t8 = a.pps_t8;
        bool all8 = true;
        for (int i = 0; i < 4; i++) { m->sub[i] = (signed char)f.sub[i]; all8 = all8 && f.sub[i] == D_L0_8x8; }
        m->t8_allowed = a.pps_t8 && (type == T_P_L0 || (type == T_P_8x8 && all8));
        m->type_left = f.type_l == T_I_8x8 ? T_I_4x4 : f.type_l; m->type_top = f.type_t == T_I_8x8 ? T_I_4x4 : f.type_t;       // x264_mb_type_fix
        m->cbp_left = f.cbp_l; m->cbp_top = f.cbp_t;
        m->cpm_left = IS_INTRA_T(f.type_l) && f.type_l != T_I_PCM ? mb_fix8c(f.cpm_l) : 0;
        m->cpm_top = IS_INTRA_T(f.type_t) && f.type_t != T_I_PCM ? mb_fix8c(f.cpm_t) : 0;
        m->nb_t8 = (f.t8_l != 0) + (f.t8_t != 0);
        m->last_qp = q.last_qp; m->last_dqp = q.last_dqp; m->prev_coded = q.prev_coded;
        m->nnz[27] = 0;
    }
    // x264_macroblock_cache_save's QP rules and x264_cabac_mb_qp_delta's side effect (R/common/macroblock.c:1244-1272, R/encoder/cabac.c:270-276)
    {
        int qp = f.qp;
        if (IS_SKIP_T(type) || (type != T_I_16x16 && !(cbp & 0x3f)) || (type == T_I_16x16 && !cbp)) qp = q.last_qp;
        q.last_dqp = qp - q.last_qp; q.last_qp = qp;
        q.prev_coded = !IS_SKIP_T(type) && (type == T_I_16x16 || (cbp & 0x3f));
    }
    CP_FOR(j, k, 48) {
        const int x = (k & 7) - 4, y = (k >> 3) - 1;
        const bool own = x >= 0 && y >= 0 && y < 4, top = y == -1 && x >= 0, left = x == -1 && y >= 0 && y < 4;
        m->i4c[k] = (signed char)((own ? i48 : (top || left)) ? f.mode[j] : -1);
        // references and vectors: the macroblock's own, then the neighbour macroblock each entry belongs to: -2 where there is none, -1 and
        // no vector for an intra one (the entries right of blocks 5, 7 and 13, which the decoder has not reached when it predicts, lie
        // outside and stay -2, R/common/macroblock.c:1050-1052)
        int r = -2, vx = 0, vy = 0, dx = 0, dy = 0;
        if (is_p && inter && f.nbt[j] >= 0) {
            if (f.nbt[j] < T_P_L0) r = -1;
            else { r = f.r[j]; vx = f.vx[j]; vy = f.vy[j]; }
        }
        if (top && has_top) { dx = w->top_mvd[mbx][x][0]; dy = w->top_mvd[mbx][x][1]; }
        else if (left && has_left) { dx = w->left_mvd[y][0]; dy = w->left_mvd[y][1]; }
        m->cref[k] = (signed char)r; m->cmv[k][0] = (i16)vx; m->cmv[k][1] = (i16)vy;
        m->cmvd[k][0] = (i16)dx; m->cmvd[k][1] = (i16)dy;
    }
    // ---- non_zero_count: the macroblock's, and the neighbours' next to it ----
    CP_FOR(j, k, 27) m->nnz[k] = (u8)f.nnz[j];
    CP_FOR(j, k, 4) { m->nz_l[k] = (u8)f.nz_l[j]; m->nz_t[k] = (u8)f.nz_t[j]; m->nz_lc[k >> 1][k & 1] = (u8)f.nz_lc[j]; m->nz_tc[k >> 1][k & 1] = (u8)f.nz_tc[j]; }
    // ---- h->dct: the state's luma array is lv4[16][16] or, in an 8x8-transform macroblock, lv8[4][64] ----
    if (!IS_SKIP_T(type) && (cbp || type == T_I_16x16)) {
        if (f.t8) CP_FOR(j, k, 256) m->lv8[k >> 6][k & 63] = f.luma[j];
        else CP_FOR(j, k, 256) m->lv4[k >> 4][k & 15] = f.luma[j];
        CP_FOR(j, k, 128) m->lv_cac[k >> 4][k & 15] = f.cac[j];
        CP_FOR(j, k, 16) m->lv_dc[k] = f.dc[j];
        CP_FOR(j, k, 8) m->lv_cdc[k >> 2][k & 3] = f.cdc[j];
    }
    CP_SYNC();
    // ---- mvd of every 4x4 block: its vector minus x264_mb_predict_mv of the partition or sub-partition it belongs to ----
    CP_FOR(j, i, 16) {
        int dx = 0, dy = 0;
        if (is_p && inter) {
            const int i8 = i >> 2, sp = m->sub[i8], part = f.part;            // (the record's copy: an index a lane computes)
            int idx = 0, width = 4;
            if (type == T_P_L0) {
                if (part == D_16x8) idx = i & 8;
                else if (part == D_8x16) { idx = i & 4; width = 2; }
            } else if (sp == D_L0_8x8) { idx = 4 * i8; width = 2; }
            else if (sp == D_L0_8x4) { idx = 4 * i8 + (i & 2); width = 2; }
            else if (sp == D_L0_4x8) { idx = 4 * i8 + (i & 1); width = 1; }
            else { idx = i; width = 1; }
            int px, py;
            mb_predict_mv([&](int k) -> int { return m->cref[k]; }, [&](int k) -> int { return m->cmv[k][0]; },
                          [&](int k) -> int { return m->cmv[k][1]; }, part, idx, width, px, py);
            dx = m->cmv[mb_scan8(i)][0] - px; dy = m->cmv[mb_scan8(i)][1] - py;
        }
        m->cmvd[mb_scan8(i)][0] = (i16)dx; m->cmvd[mb_scan8(i)][1] = (i16)dy;
    }
    CP_SYNC();
    // what the macroblocks to come read: this one's right column and bottom row
    CP_FOR(j, k, 4) {
        w->left_mvd[k][0] = m->cmvd[12 + 3 + 8 * k][0]; w->left_mvd[k][1] = m->cmvd[12 + 3 + 8 * k][1];
        w->top_mvd[mbx][k][0] = m->cmvd[12 + 24 + k][0]; w->top_mvd[mbx][k][1] = m->cmvd[12 + 24 + k][1];
    }
    CP_SYNC();
}

// one macroblock through the arithmetic coder: the in-loop writer's calls (slice_sweep_body.h), by the one lane that calls
MB_FN void cp_code(const CpArgs &a, DCabac &cab, CpCtxP ctx, CpRecP m, const int mb, const int i_frame)
{
    if (mb > 0) cd_encode_terminal(cab);
    if (IS_SKIP_T(m->type)) { cw_mb_skip(cab, ctx, m->type_left, m->type_top, 1, a.slice_type); return; }
    if (a.slice_type == 0) cw_mb_skip(cab, ctx, m->type_left, m->type_top, 0, a.slice_type);
    cw_macroblock(cab, ctx, 0, *m, (const u8 *)nullptr, i_frame);        // (no source samples: an I_PCM macroblock ends the slice before it gets here)
}

// one slice: chain bz's, by every lane of the wavefront that calls (the host: one "lane")
MB_FN void cp_write_slice(const CpArgs &a, const int bz, CpWorkP w)
{
    const int lane = CP_LANE();
    const int n = a.mb_w * a.mb_h;
    const size_t cb = (size_t)n * bz;
    const bool is_p = a.slice_type == 0;
    u8 *out = a.payload + (size_t)bz * a.payload_cap + X264HIP_PAYLOAD_LEAD;
    CpCtxP ctx = w->ctx;
    CpRecP m = &w->rec;
    DCabac cab;
    cd_encode_init(cab, out);
    for (int k = lane; k < 460; k += CP_LANES) ctx[k] = (u8)cd_context_init_one(k, a.slice_type, a.slice_qp, a.cabac_init_idc);
    CpQp q = {a.slice_qp, 0, 0};
    CpFetch f;
    cp_fetch(a, cb, 0, f, lane);
    for (int mb = 0; mb < n; mb++) {
        cp_commit(a, mb, f, m, w, q, lane);
        if (mb + 1 < n) cp_fetch(a, cb, mb + 1, f, lane);      // in flight while lane 0 codes
        if (lane == 0) {
            // what the slice type cannot hold (I_PCM: no source samples here) ends the slice like a slot too small
            const int type = m->type;
            const bool known = type >= 0 && (type < T_I_PCM || (is_p && type >= T_P_L0 && type <= T_P_SKIP));
            int stop = 1;
            if (known) {
                cp_code(a, cab, ctx, m, mb, a.i_frame + bz * a.i_frame_stride);
                const int pos = cd_pos(cab, out);
                if (a.mb_bits) a.mb_bits[cb + mb] = pos;
                stop = (pos >> 3) + CP_MB_BYTES_MAX + 64 > a.payload_cap;      // the next macroblock (and the flush) may not fit
            }
            w->stop = stop;
        }
        CP_SYNC();
        if (w->stop) {
            if (lane == 0) { CP_ABORT(a); a.payload_len[bz] = 0; }
            return;
        }
    }
    if (lane == 0) { cd_encode_flush(cab, a.i_frame + bz * a.i_frame_stride); a.payload_len[bz] = (int)(cab.p - out); }
}
