#pragma once
// frame_slice.hip -- FRAME LEVEL, part 7: the reference's per-macroblock hot loop itself.
//
// What x264_slice_write does for every macroblock of a slice (R/encoder/encoder.c:1141-1291):
//   x264_macroblock_cache_load   R/common/macroblock.c:872-1187   neighbour state, predictors
//   x264_macroblock_analyse      R/encoder/analyse.c:2156-2774    I and P slices, no RD (subme <= 5)
//   x264_macroblock_encode       R/encoder/macroblock.c:475-790
//   x264_macroblock_cache_save   R/common/macroblock.c:1208-1372
// in ONE launch per frame for a whole batch of independent GOP chains.
//
// Schedule.  A macroblock needs its left, top-left, top and top-right neighbours finished
// (reconstructed pixels for intra prediction, vectors / references / types for the predictors), so
// a frame is a 2:1 wavefront.  One wavefront (= one workgroup) owns one macroblock ROW of one
// chain and walks it left to right; row r may start macroblock x once row r-1 has published x+2
// finished macroblocks (release store / acquire load on a per-row progress word in HBM).  The left
// neighbour is the wave's own previous iteration: its state stays in LDS / registers.  Workgroup
// ids are laid out so that all rows of a chain land on the same XCD (id % 8 == chain % 8): the
// cross-row traffic stays inside one L2.  Every wait is bounded: a wave that spins too long raises
// the abort flag and every wave leaves, so the grid always drains.  FORWARD PROGRESS ASSUMPTION: the grid is oversubscribed
// (more row waves than wave slots), so a waiting wave relies on the waves of the rows above being resident or dispatched before it:
// workgroups are dispatched in increasing blockIdx order on this hardware (ids are laid out row-major for exactly that reason).
// HIP does not promise the order; if it ever changed, waves would exhaust their spin budget and the launch would be reported as
// aborted (never silently wrong): the abort count is sticky per context (x264hip_slice_sweep_status).
//
// Inside a macroblock all 64 lanes work on the same block and every decision is wave-uniform scalar state: 4 luma pixels
// per lane for prediction and SAD, one lane per 8x4 block for SATD, one lane per coefficient for the 4x4 transform, a lane
// per column / row for the 8x8 one; the motion search scores one candidate per lane group and ranks a trip's candidates
// with one packed key (me_exact.h); intra 4x4 / 8x8 modes are read out of a per-block table through a compile-time LUT
// (intra_pred.h); the motion cache and the partition candidates live in lane-indexed registers.
// Built: I_16x16 / I_8x8 / I_4x4 + chroma modes, P_SKIP (fast and early), P 16x16 / 16x8 / 8x16 / 8x8 over several
// references with or without mixed references (DIA / HEX / UMH, subme 0..5, chroma ME), 4x4 / 8x8 transform choice, CQP.
// The lane id is laundered once per macroblock and at phase boundaries (LAUNDER): otherwise every lane-derived address of the
// 60k-instruction body is hoisted out of the macroblock loop and spilled.
#include <cstddef>
#include <cstring>
#include "me_exact.h"
#include "intra_pred.h"
#include "frame_internal.h"
#include "mb_vocab.h"
#include "trellis_wave.h"
#include "cabac_price.h"

using namespace x264hip;

#define SW_MAX_REFS 8
#define SW_SPIN_LIMIT (1 << 21)
// Most bytes one macroblock's CABAC syntax can take, proven rather than observed: 384 coefficients x (significance + last flag + 14 prefix
// bins, each at most -log2(0.01875) < 6 bits when it is the least probable symbol of the most skewed state, + 31 bypass bins of the
// Exp-Golomb suffix of a 16-bit level + the sign) = 384 x 128 bits = 6144 bytes, + under 400 bytes of header, modes, vector differences
// of 16 blocks x 2 lists; I_PCM is 384.  The sweep stops (abort flag) before a macroblock that might not fit.
// Lossless (LL): the levels are differences of 8-bit samples, |level| <= 255, and below the RD levels no I_PCM candidate caps the
// macroblock, so the bound is the coefficients' own: coeff_abs_level_minus1 <= 254 = 14 prefix bins + the Exp-Golomb (k = 0) suffix of
// 240 (7 ones, a zero, 7 bits: 15 bypass bins), so 384 x (16 context-coded bins under 6 bits + 15 + the sign) = 384 x 112 bits =
// 5376 bytes, + the same under 400 bytes of everything else (27 coded_block_flags, modes, one list of vector differences): under 5800,
// inside the constant.  (6 bits per context-coded bin: the costliest is the LPS of state 62, log2(range / rangeLPS) <= log2(383 / 7)
// = 5.78.)  What changes with LL is the AVERAGE a caller should provide for below the RD levels: 6144 bytes per macroblock (slice.py:
// LL_MB_BYTES, its default) instead of the lossy 800, since a frame of noise really costs about 800 bytes per macroblock (17 bits
// per level) and nothing bounds a hostile one below the per-macroblock figure.  With the RD levels I_PCM (384 bytes) is a candidate
// of every macroblock and wins against anything priced higher, so 800 stays.
#define SW_MB_BYTES_MAX 8192
#define FD 32                      // FDEC_STRIDE
#define FDY (2 * FD)               // fdec_buf layout, R/common/macroblock.c:721-737
#define FDU (19 * FD)
#define FDV (19 * FD + 16)

enum { NB_LEFT = 1, NB_TOP = 2, NB_TOPRIGHT = 4, NB_TOPLEFT = 8 };

struct SwRefs {
    const u8 *y[SW_MAX_REFS][4];
    const u8 *u[SW_MAX_REFS], *v[SW_MAX_REFS];
    // everything indexed by a run-time reference number lives here, in the argument the kernel never writes: SwArgs is adjusted per
    // chain at the top of the kernel, and a modified argument struct with a dynamically indexed member is kept in scratch memory whole
    int ref_bits[SW_MAX_REFS], poc_delta[SW_MAX_REFS], l0_inv_ref_poc[SW_MAX_REFS];   // REF_COST = lambda * ref_bits (bs_size_te, R/encoder/analyse.c:195-197)
    // B slices: the list-1 picture (x264 core 66 without b-pyramid has one) and h->mb.bipred_weight[list-0 reference][0]
    const u8 *y1[4], *u1, *v1;
    int biw[SW_MAX_REFS];
    int dsf[SW_MAX_REFS], map_col[SW_MAX_REFS];     // temporal direct: h->mb.dist_scale_factor[i][0], h->mb.map_col_to_list0[i]
};
struct SwArgs {
    int mb_w, mb_h, sy, sc, batch, batch_pad;
    int chain;                  // the chain-table launch (template argument CH): the batch element this table entry codes
    size_t bs_y, bs_c;
    int slice_type, qp, qpc, lambda, chroma_skip_thresh, n_refs;
    int l0_n_ref0;
    int me_method, me_range, subme, chroma_me, fast_pskip, dct_decimate, cabac, mv_range;
    int flags_inter, mixed_refs; // X264_ANALYSE_PSUB16x16 (0x10) / PSUB8x8 (0x20) of param.analyse.inter; param.analyse.b_mixed_references
    int flags_intra;            // X264_ANALYSE_I4x4 | I8x8 bits that apply to this slice type (param.analyse.intra / .inter)
    int transform8x8;
    const u16 *q4mf, *q4bias, *q8mf, *q8bias;
    const int *dq4, *dq8;
    const i16 *cost_mv;
    int cost_center;
    const i16 *lowres0, *lowres1;   // fenc->lowres_mvs of list 0 / 1 towards reference 0: [batch][n_mb][2], or NULL (x264hip_slice_params.lowres_mv)
    const u8 *fy, *fu, *fv;
    u8 *dy, *du, *dv;
    const signed char *l0_type, *l0_ref;
    const i16 *l0_mv;
    signed char *mb_type, *partition, *sub_partition, *ref, *i4mode, *i16mode, *chroma_mode, *qp_out, *t8;
    i16 *mv, *mvr, *cbp;
    u8 *nnz;
    i16 *luma, *luma_dc, *chroma_dc, *chroma_ac;
    int *cost_intra, *cost_inter, *cost_alt;
    int *progress, *abort_flag;
    int *abort_total;           // per context, never reset: waves that gave up waiting, over all launches (x264hip_slice_sweep_status)
    int spin_limit;             // polls before a waiting wave gives up (SW_SPIN_LIMIT; X264HIP_SPIN_LIMIT overrides it for the abort-path test)
    long long *prof;            // optional [batch][mb_h][8] accumulated wall-clock ticks per phase (developer aid)
    int nr;                     // param.analyse.i_noise_reduction != 0
    int lossless;               // h->mb.b_lossless
    u32 *nr_sum, *nr_count;     // [batch][2][64], [batch][2]
    const u16 *nr_offset;       // [batch][2][64]
};

// the macroblock's QP and what follows from it (x264_mb_analyse_init, R/encoder/analyse.c:227-230): one set per slice at constant
// QP, per macroblock with adaptive quantisation
struct SwQp { int qp, qpc, lambda, lambda2, skip_thresh; };

struct SwLds {
    __attribute__((aligned(16))) u8 fe[384];   // source: Y 16x16 | U 8x8 | V 8x8
    u8 fd[27 * FD];             // prediction / reconstruction with its borders, fdec_buf layout
    i16 coef[16][16];           // dequantised luma coefficients
    i16 ccoef[8][16];           // dequantised chroma AC
    int score[16], cscore[8];
    i16 cdc[8], cdcout[8], dc16[16];
    int keep8, cmode[2], nzdc16;
    i16 lv_y[256], lv_dc[16], lv_cdc[8], lv_cac[128];
    u8 nnz[32];
    i16 mvc[9][2];              // x264_mb_predict_mv_ref16x16's list: direct, lookahead, four neighbours, three temporal
    i16 left_mvr[SW_MAX_REFS][2];
    // intra 4x4 / 8x8 analysis: prediction-mode cache in x264_scan8 layout, edge arrays, and what the reference keeps
    // when i_skip_intra is set (the partly encoded macroblock of the analysis is the final one, macroblock.c:527-577)
    signed char i4c[48];
    u8 e4[16], edge8[40];
    __attribute__((aligned(4))) u8 pt4[48];   // the current 4x4 / 8x8 block's prediction table (intra_pred.h: RAW | F1 | F2 | DC..)
    __attribute__((aligned(4))) u8 pt8[80];
    u32 p4lut[48], p8lut[192];  // c_plut4 / c_plut8
    u16 nr_off4[16], nr_off8[64];   // h->nr_offset[0] / [1] of this chain (--nr)
    __attribute__((aligned(16))) u8 patch[MX_PATCH_BYTES];   // the motion search's staged sub-pel neighbourhood (me_exact.h)
    u8 i4_fdec[256], i8_fdec[256], i4_nnz[16], i8_nnz[16];
    i16 lv_y8[256];             // levels of the 8x8 transform (h->dct.luma8x8), separate from the 4x4 ones like the reference's
    i16 t8[256];                // 8x8 transform: intermediate between the two 1-D passes
    signed char left_i4[4];     // the left macroblock's modes of blocks 5, 7, 13, 15
    signed char pred4[16], pred8[4];
    // P partitions: the motion cache (h->mb.cache.ref / mv, x264_scan8 layout), a->l0.mvc, candidate records, final vectors
    i16 l0mvc[SW_MAX_REFS][5][2];
    i16 mv4[16][2];
    signed char ref8[4];
    i16 left_mv4[4][2];         // the left macroblock's vectors of blocks 3, 7, 11, 15 and references of its 8x8 blocks 1, 3
    signed char left_r8[2];
    u16 q8mf[2][64], q8bias[2][64];
    int q8dq[2][64];
    // this frame's quantiser rows (cat 0 intra Y, 1 inter Y at qp; 2 intra C, 3 inter C at the chroma qp) and the centre of p_cost_mv
    u16 qmf[4][16], qbias[4][16];
    int qdq[4][16];
    i16 costl[2 * MX_COST_LDS + 2];
};

// ---- round 2: what the raster-order variant of the sweep (RD levels, trellis, adaptive quantisation, the entropy coder) adds ----
struct SwRd {                       // kernel argument
    int on;                         // this launch is the raster variant
    int mbrd, trellis, psy_rd;      // a->i_mbrd, param.analyse.i_trellis, h->mb.i_psy_rd
    int write, cabac_init_idc, i_frame, i_frame_stride;
    int aq, qp_min, qp_max, chroma_qp_offset;
    float f_qpm;
    int psy_trellis;                // h->mb.i_psy_trellis (k_psy_raster; in what was padding: every other member keeps its offset)
    const float *aq_offset;         // [batch][n_mb]
    const i16 *cost_mv_all;         // [52][2 * cost_center + 1]: p_cost_mv of every QP
    const int *unq4, *unq8;         // h->unquant4_mf [4][52][16], h->unquant8_mf [2][52][64]
    u8 *payload; int payload_cap;
    u32 psy_carry_lo;               // x264hip_slice_rd.psy_carry, low half (k_psy_raster; this and psy_carry_hi sit in what was padding, as psy_trellis does)
    int *payload_len, *mb_bits;
    i16 *mvd;                       // h->mb.mvd[0]: [batch][n_mb][16][2]
    // B slices: list 1 of the per-macroblock state, h->mb.skipbp, and the co-located picture's arrays (direct prediction)
    i16 *mv1, *mvr1, *mvd1;
    signed char *ref1;
    union {
        u8 *skipbp;                 // a B slice: h->mb.skipbp
        u8 *mb_carry;               // an I / P slice (no list 1, no skip flags: the member is free there, and SwRd keeps its size and every kernel its
                                    // argument layout): x264hip_slice_rd.mb_carry, [batch][160], the macroblock's own non_zero_count / mvd cache entries
    };
    const signed char *col_type, *col_ref;
    const i16 *col_mv;
    int direct_temporal;            // !sh.b_direct_spatial_mv_pred
    u32 psy_carry_hi;
    int *direct_score;              // --direct auto: [batch][2] h->stat.frame.i_direct_score ({temporal, spatial}); NULL: off
    i16 *stale;                     // [batch][8]: the cache entry of block 12 that survives macroblocks and frames (x264hip_slice_rd.stale)
};
static_assert(offsetof(SwRd, psy_carry_lo) == offsetof(SwRd, payload_cap) + 4 && offsetof(SwRd, payload_len) == offsetof(SwRd, psy_carry_lo) + 4 &&
              offsetof(SwRd, psy_carry_hi) == offsetof(SwRd, direct_temporal) + 4 && offsetof(SwRd, direct_score) == offsetof(SwRd, psy_carry_hi) + 4,
              "the two halves of the psy-trellis carry's address fill padding: the kernel argument of every other kernel keeps its layout");
// what a B slice adds to the wavefront's LDS: list 1 of the motion caches, the direct prediction, the analysis records
struct SwLdsB {
    signed char cref1[48], cskip[48];
    i16 cmv1[48][2], cmvd1[48][2];
    signed char dref[2][4], sub[4];     // h->mb.cache.direct_ref; h->mb.i_sub_partition
    i16 dmv[2][16][2];                  // h->mb.cache.direct_mv (the 16 blocks in raster order)
    i16 mv4_1[16][2];
    signed char ref8_1[4];
    i16 left_mv4_1[4][2], left_mvd1[4][2], left_mvr1[2];
    signed char left_r8_1[2];
    u8 left_skipbp;
    i16 stale[6];                       // SwRd::stale while the slice is coded: {ref, mv x, mv y} of cache entry 30, list 0 | list 1
    int me[2][9][6];                    // x264_me_t records of a->l0 / a->l1: [list][me16x16, me8x8 x 4, me16x8 x 2, me8x16 x 2][mv x, y, cost, cost_mv, mvp x, y]
    int cost8direct[4];
};
struct SwLdsRdB;
// x264_me_refine_bidir's 32 candidate offsets per pass in evaluation order (CHECK_BIDIR8 / CHECK_BIDIR2, R/encoder/me.c:893-909):
// (m0x, m0y, m1x, m1y) offsets + 1 in four 2-bit fields
static __device__ const u8 c_bidir_dirs[32] = {149, 21, 101, 69, 89, 81, 86, 84, 165, 5, 105, 65, 90, 80, 150, 20, 153, 17, 102, 68, 133, 37, 97, 73, 88, 82, 22, 148, 145, 25, 100, 70};
struct SwLdsRd {
    u8 cabac[460], cabac_tmp[460];  // h->cabac.state and the RD trial's copy (COPY_CABAC, R/encoder/rdo.c:62)
    // what the entropy coder reads beyond SwLds (MbSynDev below points into both)
    signed char cref[48], sub[4];
    i16 cmv[48][2], cmvd[48][2];
    u8 nz_l[4], nz_t[4], nz_lc[2][2], nz_tc[2][2];
    i16 i4_dct[256], i8_dct[256];   // h->mb.pic.i4x4_dct_buf / i8x8_dct_buf (i_skip_intra == 2)
    int fenc_satd[16], fenc_sa8d[4];   // h->mb.pic.fenc_satd / fenc_sa8d (psy-RD)
    int unq4[4][16], unq8[2][64];   // unquant rows of the current QPs
    i16 left_mvd[4][2];             // the left macroblock's mvd of blocks 3, 7, 11, 15
    u8 left_nz[8];                  // its non_zero_count of blocks 5 7 13 15 | U 1 3 | V 1 3
    u8 zz2[4], zz4[16], zz8[64];    // scan position -> raster index; the trellis weights in scan order (x264_dct4/8_weight2_zigzag[0])
    int w4z[16], w8z[64];
    u8 zero16[16];                  // sixteen zeros (SATD / SA8D of the source against nothing)
    int tmp_i[4];                   // lane 0 -> wave: bit count / QP after the writer
    TdWave tw;
};
struct SwLdsNone { int unused; };
struct SwLdsRdB { SwLdsRd r; SwLdsB b; };
// what the RD refinement (subme 8+, template argument RF) adds: the analysis' per-mode costs (a->i_satd_i16x16_dir[mode],
// i_satd_i8x8chroma_dir[list position], i_satd_i8x8_dir[mode][block]) and the pixels x264_intra_rd_refine keeps of its best trial
struct SwLdsRf { int i16dir[8], cdir[4], i8dir[12][4]; u8 pels[16]; };
struct SwLdsRdF { SwLdsRd r; SwLdsRf f; };
// the record cabac_dev.h's writer walks (same member names as MbSyn): scalars in registers, arrays where the kernel keeps them in LDS
struct MbSynDev {
    int slice_type, type, partition, i16mode, chroma_mode, cbp_luma, cbp_chroma, t8, qp, n_ref, pps_t8, t8_allowed;
    int type_left, type_top, cbp_left, cbp_top, cpm_left, cpm_top, nb_t8, last_qp, last_dqp, prev_coded;
    signed char *sub, *i4c, *cref;
    i16 (*cmv)[2], (*cmvd)[2];
    int n_ref1;                          // B slices: list 1 of the caches, the skip flags of direct blocks
    signed char *cref1, *cskip;
    i16 (*cmv1)[2], (*cmvd1)[2];
    u8 *nnz, *nz_l, *nz_t;
    u8 (*nz_lc)[2], (*nz_tc)[2];
    i16 (*lv4)[16], (*lv8)[64], *lv_dc, (*lv_cdc)[4], (*lv_cac)[16];
};
// trellis context handed to the quantising helpers: on = 0 -> plain dead-zone quantisation
struct SwTq { static constexpr bool PSY = false; int on; SwLdsRd *r; };
// ... and with psy-trellis (k_psy_raster): psy = h->mb.i_psy_trellis.
// src4 / src8: what h->mb.pic.fenc_dct4 / fenc_dct8 hold when this macroblock's blocks are quantised -- its own source's transform, the zeros x264_t
// was allocated with, or what an EARLIER macroblock (of this frame or of one before it) left: kept[512], the chain's slot of x264hip_slice_rd.psy_carry
enum { SW_PSY_OWN = 0, SW_PSY_ZERO = 1, SW_PSY_KEPT = 2 };
struct SwTqPsy { static constexpr bool PSY = true; int on; SwLdsRd *r; int psy, src4, src8; i16 *kept; };
__device__ __forceinline__ void sw_tq_set_psy(SwTq &, int, int, i16 *) {}
__device__ __forceinline__ void sw_tq_set_psy(SwTqPsy &tq, int psy, int src, i16 *kept) { tq.psy = psy; tq.src4 = tq.src8 = src; tq.kept = kept; }
__device__ __forceinline__ i16 *sw_psy_carry(const SwRd &rd, int bz)
{
    const unsigned long long p = ((unsigned long long)rd.psy_carry_hi << 32) | rd.psy_carry_lo;
    return p ? (i16 *)p + (size_t)bz * 512 : nullptr;
}
// x264_dct4_weight2_zigzag[0] / x264_dct8_weight2_zigzag[0] (R/common/dct.c:476-483) and x264_zigzag_scan4[0]
static __device__ const int d_w4z[16] = {800, 320, 320, 800, 128, 800, 320, 320, 320, 320, 128, 800, 128, 320, 320, 128};
static __device__ const u8 d_zz4[16] = {0, 4, 1, 2, 5, 8, 12, 9, 6, 3, 7, 10, 13, 14, 11, 15};
static __device__ const u8 d_zz2[4] = {0, 1, 2, 3};
static __device__ const u16 d_w8k[6] = {256, 201, 656, 227, 410, 363};
static __device__ const u8 d_w8cls[16] = {0, 3, 4, 3, 3, 1, 5, 1, 4, 5, 2, 5, 3, 1, 5, 1};
__device__ __forceinline__ int sw_w8z(int pos) { const int r = c_scan8[0][pos]; return d_w8k[d_w8cls[((r >> 1) & 12) | (r & 3)]]; }
struct SwW8 { __device__ __forceinline__ int operator[](int pos) const { return sw_w8z(pos); } };

// lanes exchange data through LDS only: order LDS traffic (lgkmcnt) and leave global loads / stores in flight
#define WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local"); __builtin_amdgcn_wave_barrier(); \
                         __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local"); } while (0)

__device__ __forceinline__ void sw_blk_xy(int k, int &x, int &y)
{
    x = ((k >> 2) & 1) * 8 + (k & 1) * 4;
    y = (k >> 3) * 8 + ((k >> 1) & 1) * 4;
}
__device__ __forceinline__ int sw_decimate(const i16 *lv, int n)
{   // R/common/quant.c:213-239 on scanned levels lv[0..n)
    int i = n - 1, score = 0;
    while (i >= 0 && lv[i] == 0) i--;
    while (i >= 0) {
        if ((unsigned)(lv[i--] + 1) > 2u) return 9;
        int run = 0;
        while (i >= 0 && lv[i] == 0) { i--; run++; }
        score += c_decimate4[run];
    }
    return score;
}
__device__ __forceinline__ int sw_ue_size(int v) { return v == 0 ? 1 : v < 3 ? 3 : 5; }   // bs_size_ue for 0..6

// ---- motion compensation of one 16x16 vector into s.fd (x264_mb_mc_0xywh, R/common/macroblock.c:462-476)
__device__ __forceinline__ void sw_mc16(SwLds &s, const SwRefs &refs, const SwArgs &a, int ri, int mvx, int mvy, ptrdiff_t oy, ptrdiff_t oc,
                                        size_t by, size_t bc, int lane, bool do_chroma)
{
    {
        const int r = lane >> 2, x = (lane & 3) * 4;
        const int qx = mvx & 3, qy = mvy & 3, idx = qy * 4 + qx;
        const ptrdiff_t base = oy + (ptrdiff_t)((mvy >> 2) + r) * a.sy + (mvx >> 2) + x + (ptrdiff_t)by;
        const u8 *pa = refs.y[ri][c_qpel_a[idx]] + base + (qy == 3) * a.sy;
        const u8 *pb = refs.y[ri][c_qpel_b[idx]] + base + (qx == 3);
#pragma unroll
        for (int i = 0; i < 4; i++)
            s.fd[FDY + r * FD + x + i] = (idx & 5) ? (u8)(((int)pa[i] + (int)pb[i] + 1) >> 1) : pa[i];
    }
    if (do_chroma) {
        const int cx = lane & 7, cy = lane >> 3;
        const int dx = mvx & 7, dyy = mvy & 7;
        const int ca = (8 - dx) * (8 - dyy), cb = dx * (8 - dyy), cc = (8 - dx) * dyy, cd = dx * dyy;
        const ptrdiff_t cbase = oc + (ptrdiff_t)((mvy >> 3) + cy) * a.sc + (mvx >> 3) + cx + (ptrdiff_t)bc;
        const u8 *pu = refs.u[ri] + cbase, *pv = refs.v[ri] + cbase;
        s.fd[FDU + cy * FD + cx] = (u8)((ca * pu[0] + cb * pu[1] + cc * pu[a.sc] + cd * pu[a.sc + 1] + 32) >> 6);
        s.fd[FDV + cy * FD + cx] = (u8)((ca * pv[0] + cb * pv[1] + cc * pv[a.sc] + cd * pv[a.sc + 1] + 32) >> 6);
    }
}

// x264_mb_mc for any P partition: every pixel with the vector of its 4x4 block and the reference of its 8x8 (s.mv4 / s.ref8)
// clip: x264_mb_mc_0xywh's clip of the vector to h->mb.mv_min / mv_max (R/common/macroblock.c:465-466); the analysis never leaves a vector
// outside them, the candidates of the RD refinement (subme 8+) may sit a quarter sample or two beyond
__device__ __forceinline__ void sw_mc_parts(SwLds &s, const SwRefs &refs, const SwArgs &a, ptrdiff_t oy, ptrdiff_t oc, size_t by, size_t bc, int lane,
                                            bool clip = false, int mbx = 0, int mby = 0)
{
    const int lox = 4 * (-16 * mbx - 24), hix = 4 * (16 * (a.mb_w - mbx - 1) + 24), loy = 4 * (-16 * mby - 24), hiy = 4 * (16 * (a.mb_h - mby - 1) + 24);
    {
        const int r = lane >> 2, x = (lane & 3) * 4, blk = (r >> 2) * 4 + (x >> 2);
        int mvx = s.mv4[blk][0], mvy = s.mv4[blk][1];
        const int ri = s.ref8[(r >> 3) * 2 + (x >> 3)];
        if (clip) { mvx = clip3(mvx, lox, hix); mvy = clip3(mvy, loy, hiy); }
        const int qx = mvx & 3, qy = mvy & 3, idx = qy * 4 + qx;
        const ptrdiff_t base = oy + (ptrdiff_t)((mvy >> 2) + r) * a.sy + (mvx >> 2) + x + (ptrdiff_t)by;
        const u8 *pa = refs.y[ri][c_qpel_a[idx]] + base + (qy == 3) * a.sy;
        const u8 *pb = refs.y[ri][c_qpel_b[idx]] + base + (qx == 3);
#pragma unroll
        for (int i = 0; i < 4; i++)
            s.fd[FDY + r * FD + x + i] = (idx & 5) ? (u8)(((int)pa[i] + (int)pb[i] + 1) >> 1) : pa[i];
    }
    {
        const int cx = lane & 7, cy = lane >> 3, blk = (cy >> 1) * 4 + (cx >> 1);
        int mvx = s.mv4[blk][0], mvy = s.mv4[blk][1];
        const int ri = s.ref8[(cy >> 2) * 2 + (cx >> 2)];
        if (clip) { mvx = clip3(mvx, lox, hix); mvy = clip3(mvy, loy, hiy); }
        const int dx = mvx & 7, dyy = mvy & 7;
        const int ca = (8 - dx) * (8 - dyy), cb = dx * (8 - dyy), cc = (8 - dx) * dyy, cd = dx * dyy;
        const ptrdiff_t cbase = oc + (ptrdiff_t)((mvy >> 3) + cy) * a.sc + (mvx >> 3) + cx + (ptrdiff_t)bc;
        const u8 *pu = refs.u[ri] + cbase, *pv = refs.v[ri] + cbase;
        s.fd[FDU + cy * FD + cx] = (u8)((ca * pu[0] + cb * pu[1] + cc * pu[a.sc] + cd * pu[a.sc + 1] + 32) >> 6);
        s.fd[FDV + cy * FD + cx] = (u8)((ca * pv[0] + cb * pv[1] + cc * pv[a.sc] + cd * pv[a.sc + 1] + 32) >> 6);
    }
}

// ---- block costs between s.fe and s.fd ---------------------------------------------------------
// one row of an 8x4 block per lane (lanes of one block are l, l^1, l^2, l^3); returns the block SATD
__device__ __forceinline__ int sw_satd_row8(const u8 *f, const u8 *p, int lane)
{
    int d[8];
#pragma unroll
    for (int x = 0; x < 8; x++) d[x] = (int)f[x] - (int)p[x];
    u32 p0 = (u32)d[0] + ((u32)d[4] << 16), p1 = (u32)d[1] + ((u32)d[5] << 16);
    u32 p2 = (u32)d[2] + ((u32)d[6] << 16), p3 = (u32)d[3] + ((u32)d[7] << 16);
    u32 t0, t1, t2, t3;
    wht4(t0, t1, t2, t3, p0, p1, p2, p3);
    return satd_rows4(t0, t1, t2, t3, lane);
}
// mbcmp[PIXEL_16x16](fdec luma, fenc luma): SATD above subme 1, else SAD (R/encoder/encoder.c:608-618)
__device__ __forceinline__ int sw_cmp_luma16(const SwLds &s, int satd, int lane)
{
    int v = 0;
    if (satd) {
        if (lane < 32) {
            const int blk = lane >> 2, r = lane & 3, bx = (blk & 1) * 8, y = (blk >> 1) * 4 + r;
            v = sw_satd_row8(s.fe + y * 16 + bx, s.fd + FDY + y * FD + bx, lane);
            if (r) v = 0;
        }
    } else {
        const int r = lane >> 2, x = (lane & 3) * 4;
        v = (int)sad4(*(const u32 *)(s.fe + r * 16 + x), *(const u32 *)(s.fd + FDY + r * FD + x), 0);
    }
    return wave_sum(v);
}
// mbcmp[PIXEL_8x8] of both chroma planes, summed
__device__ __forceinline__ int sw_cmp_chroma(const SwLds &s, int satd, int lane)
{
    int v = 0;
    if (satd) {
        if (lane < 16) {
            const int pl = lane >> 3, blk = (lane >> 2) & 1, r = lane & 3, y = blk * 4 + r;
            v = sw_satd_row8(s.fe + 256 + 64 * pl + y * 8, s.fd + (pl ? FDV : FDU) + y * FD, lane);
            if (r) v = 0;
        }
    } else {
        const int x = lane & 7, y = lane >> 3;
        v = iabs((int)s.fe[256 + y * 8 + x] - (int)s.fd[FDU + y * FD + x]) + iabs((int)s.fe[320 + y * 8 + x] - (int)s.fd[FDV + y * FD + x]);
    }
    return wave_sum(v);
}

// ---- intra prediction into s.fd ----------------------------------------------------------------
// x264_predict_16x16_* (R/common/predict.c:52-170): the sums the DC and plane modes need are reduced
// across the wave once per call instead of per pixel
// x264_predict_lossless_* (R/encoder/macroblock.c:405-470): vertical / horizontal prediction take the SOURCE one row up / one column
// left.  Everything coded so far reconstructs to its source, so outside the macroblock that is the neighbour row / column
// already in s.fd and inside it the macroblock's own source in s.fe.  (x, y) relative to the macroblock; plane 0 luma, 1 U, 2 V.
__device__ __forceinline__ int sw_ll_px(const SwLds &s, int plane, int horiz, int x, int y)
{
    const int st = plane ? 8 : 16;
    const u8 *fe = s.fe + (plane == 0 ? 0 : plane == 1 ? 256 : 320), *fd = s.fd + (plane == 0 ? FDY : plane == 1 ? FDU : FDV);
    if (horiz) return x == 0 ? fd[y * FD - 1] : fe[y * st + x - 1];
    return y == 0 ? fd[x - FD] : fe[(y - 1) * st + x];
}
__device__ __forceinline__ void sw_pred16(SwLds &s, int mode, int lane, int ll = 0)
{
    const int r = lane >> 2, x = (lane & 3) * 4;
    const u8 *top = s.fd + FDY - FD, *left = s.fd + FDY - 1;
    int v[4];
    if (mode == 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = top[x + i];
    } else if (mode == 1) {
        v[0] = v[1] = v[2] = v[3] = left[r * FD];
    } else if (mode == 3) {
        int h = 0, w = 0;
        if (lane < 8) { h = (lane + 1) * ((int)top[8 + lane] - (int)top[6 - lane]); w = (lane + 1) * ((int)left[(8 + lane) * FD] - (int)left[(6 - lane) * FD]); }
        const int H = wave_sum(h), V = wave_sum(w);
        const int a = 16 * ((int)left[15 * FD] + (int)top[15]), b = (5 * H + 32) >> 6, c = (5 * V + 32) >> 6;
        const int i00 = a - 7 * b - 7 * c + 16 + c * r;
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = clip_u8((i00 + b * (x + i)) >> 5);
    } else {
        int dc = 128;
        if (mode != 6) {
            const int t = wave_sum(lane < 16 ? (int)top[lane] : 0), l = wave_sum(lane < 16 ? (int)left[lane * FD] : 0);
            dc = mode == 2 ? (t + l + 16) >> 5 : mode == 4 ? (l + 8) >> 4 : (t + 8) >> 4;
        }
        v[0] = v[1] = v[2] = v[3] = dc;
    }
    if (ll && mode < 2) {
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = sw_ll_px(s, 0, mode, x + i, r);
    }
    WAVE_SYNC();
#pragma unroll
    for (int i = 0; i < 4; i++) s.fd[FDY + r * FD + x + i] = (u8)v[i];
    WAVE_SYNC();
}
__device__ __forceinline__ void sw_pred8c(SwLds &s, int mode, int lane, int ll = 0)
{
    const int x = lane & 7, y = lane >> 3;
    int pu = pred_px(1, mode, s.fd + FDU, FD, x, y), pv = pred_px(1, mode, s.fd + FDV, FD, x, y);
    if (ll && (mode == 1 || mode == 2)) { pu = sw_ll_px(s, 1, mode == 1, x, y); pv = sw_ll_px(s, 2, mode == 1, x, y); }
    WAVE_SYNC();
    s.fd[FDU + y * FD + x] = (u8)pu; s.fd[FDV + y * FD + x] = (u8)pv;
    WAVE_SYNC();
}
// predict_16x16_mode_available / predict_8x8chroma_mode_available, R/encoder/analyse.c:374-433
// the list is a packed word, one nibble per mode in the reference's order (an array indexed in a loop would live in scratch memory)
__device__ __forceinline__ u32 sw_modes16(int nb, int &n)
{
    if (nb & NB_TOPLEFT) { n = 4; return 0x3210; }
    if (nb & NB_LEFT) { n = 2; return 0x14; }
    if (nb & NB_TOP) { n = 2; return 0x05; }
    n = 1; return 6;
}
__device__ __forceinline__ u32 sw_modes8c(int nb, int &n)
{
    if (nb & NB_TOPLEFT) { n = 4; return 0x3012; }
    if (nb & NB_LEFT) { n = 2; return 0x14; }
    if (nb & NB_TOP) { n = 2; return 0x25; }
    n = 1; return 6;
}
__device__ __forceinline__ int sw_fix16(int m) { return m < 4 ? m : 2; }      // x264_mb_pred_mode16x16_fix
__device__ __forceinline__ int sw_fix8c(int m) { return m < 4 ? m : 0; }      // x264_mb_pred_mode8x8c_fix

// ---- psy-trellis: the source block's own transform in scan order (x264_psy_trellis_init, R/encoder/analyse.c:488-507) ----
// The reference transforms the source macroblock at most once and keeps 1 KiB of it in x264_t (h->mb.pic.fenc_dct4 [16][16], fenc_dct8 [4][64]), which it
// never clears: a block is quantised against whatever the arrays hold.  Where that is the macroblock's own source (SW_PSY_OWN) the block(s) about to be
// quantised are transformed again from s.fe right before the trellis, into 128 bytes of the motion search's patch behind the trellis' level lists (the
// patch is idle while a block is quantised): no LDS is added.  Where it is what an earlier macroblock left (SW_PSY_KEPT) they come from the chain's 1 KiB
// of global memory (x264hip_slice_rd.psy_carry: fenc_dct4 | fenc_dct8, in scan order), which sw_psy_keep4 / sw_psy_keep8 write where the reference writes
// its arrays; where nobody ever wrote them, zeros (SW_PSY_ZERO).
#define SW_PSY_FENC(s_) ((i16 *)((s_).patch + 16 * TDW_TREE_STRIDE))
static_assert(4 * TDW_TREE_STRIDE >= TDW_TREE_ENTRIES && 16 * TDW_TREE_STRIDE + 128 <= MX_PATCH_BYTES, "the source coefficients sit behind the level lists");
// x264_dct4_weight_tab / x264_dct8_weight_tab (R/common/dct.h:25-53) by raster index
struct SwPw4 { __device__ __forceinline__ int operator[](int r) const { const int n = ((r >> 2) & 1) + (r & 1); return n == 0 ? 453 : n == 1 ? 286 : 181; } };
struct SwPw8 {
    __device__ __forceinline__ int operator[](int r) const
    {
        const int k = d_w8cls[((r >> 1) & 12) | (r & 3)];
        return k == 0 ? 256 : k == 1 ? 227 : k == 2 ? 410 : k == 3 ? 241 : k == 4 ? 324 : 305;
    }
};
__device__ __forceinline__ int sw_fwd4_quad(int v, int k);
// x264_zigzag_scan4's position of raster coefficient l16
__device__ __forceinline__ int sw_psy_zz4(int l16) { return (int)((0xFDC6EB75A8419320ull >> (4 * l16)) & 15); }
// the 16-lane group of `lane` transforms the source's 4x4 block k, as sw_encode_i4x4 does the residual: lane l16 returns dct[l16] (raster)
__device__ __forceinline__ int sw_psy_dct4(SwLds &s, int k, int lane)
{
    int bx, by;
    sw_blk_xy(k, bx, by);
    const int l16 = lane & 15, x = l16 & 3, y = l16 >> 2, tl = (lane & 48) | (x << 2) | y;
    int v = (int)s.fe[(by + y) * 16 + bx + x];
    v = sw_fwd4_quad(v, x);
    v = __shfl(v, tl, 64);
    return sw_fwd4_quad(v, x);
}
// the source's 8x8 block j through the 8x8 transform's intermediate (s.t8: the residual's passes are over when the trellis runs): leaves dct[r] (raster) in s.t8[64 + r]
__device__ __forceinline__ void sw_psy_dct8(SwLds &s, int j, int lane)
{
    i16 *tmp = s.t8;
    const int k8 = lane & 7;
    if (lane < 8) {
        const u8 *p1 = s.fe + (j >> 1) * 8 * 16 + (j & 1) * 8 + k8;
        int v[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = (int)p1[k * 16];
        fwd8_1d(o, v);
#pragma unroll
        for (int k = 0; k < 8; k++) tmp[k * 8 + k8] = (i16)o[k];
    }
    WAVE_SYNC();
    if (lane < 8) {
        int v[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = tmp[k8 * 8 + k];
        fwd8_1d(o, v);
#pragma unroll
        for (int k = 0; k < 8; k++) tmp[64 + k * 8 + k8] = (i16)o[k];
    }
    WAVE_SYNC();
}
// every lane calls it: the source coefficients of 4x4 block k (the 16-lane group's own) into the group's 16 entries of SW_PSY_FENC
template <class TQ>
__device__ __forceinline__ void sw_psy_src4(SwLds &s, TQ tq, int k, int lane)
{
    const int l16 = lane & 15;
    if (tq.src4 != SW_PSY_OWN) SW_PSY_FENC(s)[(lane & 48) + l16] = tq.src4 == SW_PSY_ZERO ? (i16)0 : tq.kept[k * 16 + l16];
    else SW_PSY_FENC(s)[(lane & 48) + sw_psy_zz4(l16)] = (i16)sw_psy_dct4(s, k, lane);
    WAVE_SYNC();
}
// ... and of 8x8 block j, one per lane
template <class TQ>
__device__ __forceinline__ void sw_psy_src8(SwLds &s, TQ tq, int j, int lane)
{
    if (tq.src8 != SW_PSY_OWN) SW_PSY_FENC(s)[lane] = tq.src8 == SW_PSY_ZERO ? (i16)0 : tq.kept[256 + j * 64 + lane];
    else {
        sw_psy_dct8(s, j, lane);
        SW_PSY_FENC(s)[lane] = s.t8[64 + c_scan8[0][lane]];
    }
    WAVE_SYNC();
}
// x264_psy_trellis_init's two halves: the source macroblock's sixteen 4x4 transforms / four 8x8 transforms into the chain's kept arrays.  The
// fence makes the stores visible to the lanes that read them back in a later macroblock (WAVE_SYNC orders LDS only).
__device__ __forceinline__ void sw_psy_keep4(SwLds &s, i16 *kept, int lane)
{
#pragma nounroll
    for (int it = 0; it < 4; it++) {
        const int k = 4 * it + (lane >> 4);
        kept[k * 16 + sw_psy_zz4(lane & 15)] = (i16)sw_psy_dct4(s, k, lane);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
}
__device__ __forceinline__ void sw_psy_keep8(SwLds &s, i16 *kept, int lane)
{
#pragma nounroll
    for (int j = 0; j < 4; j++) {
        sw_psy_dct8(s, j, lane);
        kept[256 + j * 64 + lane] = s.t8[64 + c_scan8[0][lane]];
        WAVE_SYNC();
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
}
// x264_psy_trellis_init( h, 0 ) after the analysis (--trellis 1, analyse.c:2770-2771): ONLY the size h->mb.b_transform_8x8 (f8) names at that moment is
// refreshed.  An inter macroblock is then coded with that size; an I_4x4 / I_16x16 one with f8 set (left by the transform decision of the inter candidate
// it beat) and an I_8x8 one with f8 clear (the flag turns 1 only in x264_macroblock_encode, macroblock.c:533, or in x264_rd_cost_i8x8 of the
// refinement, rdo.c:249) are quantised against what an earlier macroblock left.
__device__ __forceinline__ void sw_psy_after_analysis(SwLds &, SwTq &, int, int) {}
__device__ __forceinline__ void sw_psy_after_analysis(SwLds &s, SwTqPsy &tq, int f8, int lane)
{
    if (f8) { sw_psy_keep8(s, tq.kept, lane); tq.src8 = SW_PSY_OWN; tq.src4 = SW_PSY_KEPT; }
    else { sw_psy_keep4(s, tq.kept, lane); tq.src4 = SW_PSY_OWN; tq.src8 = SW_PSY_KEPT; }
}
// x264_psy_trellis_init( h, param.analyse.b_transform_8x8 ) in x264_mb_cache_fenc_satd (--trellis 2, analyse.c:515-516)
__device__ __forceinline__ void sw_psy_before_trials(SwLds &, SwTq &, int, int) {}
__device__ __forceinline__ void sw_psy_before_trials(SwLds &s, SwTqPsy &tq, int both, int lane)
{
    if (both) sw_psy_keep8(s, tq.kept, lane);
    sw_psy_keep4(s, tq.kept, lane);
}

// ---- encode pieces (R/encoder/macroblock.c:116-363, 596-768; no trellis, not lossless) ------------
// luma 4x4 transform + quant + scan + dequant of the 16 blocks, lanes 0-15.  cat: 0 intra, 1 inter.
// i16 mode takes the DC out first (s.dc16 in raster order) and scores with decimate_score15.
// x264_denoise_dct (R/common/quant.c:180-192) on coefficient v with offset off: returns the new coefficient, la = |v|
__device__ __forceinline__ int sw_denoise(int v, int off, int &la)
{
    const int sign = v >> 15;
    int level = (v + sign) ^ sign;
    la = level;
    level -= off;
    return level < 0 ? 0 : (level ^ sign) - sign;
}
// mask8: the 8x8 blocks to do (x264_macroblock_encode_p8x8 codes one); lanes of other blocks leave everything of theirs alone
template <class TQ>
__device__ __forceinline__ void sw_luma4x4_fwd(SwLds &s, const SwArgs &a, const SwQp &Q, TQ tq, int cat, bool dc_out, int lane, int *nr_acc4 = nullptr, int nr_on = 0,
                                               int mask8 = 0xf, int mask16 = 0xffff)
{   // mask16: the 4x4 blocks to do among those of mask8 (x264_macroblock_encode_p4x4 codes one)
    i16 c[16], lv[16];
    const bool mine = lane < 16 && ((mask8 >> (lane >> 2)) & 1) && (mask16 == 0xffff || ((mask16 >> lane) & 1));
    if (mine) {
        int bx, by, r[16];
        sw_blk_xy(lane, bx, by);
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int i = 0; i < 4; i++)
                r[4 * j + i] = (int)s.fe[(by + j) * 16 + bx + i] - (int)s.fd[FDY + (by + j) * FD + bx + i];
        fwd4x4(c, r);
        if (nr_acc4 && nr_on) {
            // --nr: every coefficient but the first of every block, and the sum of magnitudes per coefficient index over the 16
            // blocks (lane i keeps index i's running sum for the whole row; added to the chain's totals at the end of the row)
#pragma unroll
            for (int i = 1; i < 16; i++) {
                int la;
                c[i] = (i16)sw_denoise(c[i], s.nr_off4[i], la);
                const int t = row_sum16(la);
                if (lane == i) *nr_acc4 += t;
            }
        }
        if (dc_out) { s.dc16[(by >> 2) * 4 + (bx >> 2)] = c[0]; c[0] = 0; }
        if (tq.on) {
#pragma unroll
            for (int i = 0; i < 16; i++) s.coef[lane][i] = c[i];
        }
    }
    if (tq.on) {
        // x264_quant_4x4_trellis (R/encoder/rdo.c:641-650): four blocks at a time, sixteen lanes each (trellis_wave.h)
        WAVE_SYNC();
#pragma nounroll
        for (int it = 0; it < 4; it++)
            if ((mask8 >> it) & 1) {
            if constexpr (TQ::PSY) {
                sw_psy_src4(s, tq, 4 * it + (lane >> 4), lane);
                td_trellis_wave(tq.r->tw, (u32 *)s.patch, &s.coef[4 * it + (lane >> 4)][0], mask16 == 0xffff || ((mask16 >> (4 * it + (lane >> 4))) & 1), s.qmf[cat], tq.r->unq4[cat], tq.r->w4z, tq.r->zz4, tq.r->cabac, dc_out ? 1 : 2,
                                d_trellis_lambda2[cat == 0][Q.qp], dc_out ? 1 : 0, 0, 16, lane, SW_PSY_FENC(s) + (lane & 48), SwPw4(), tq.psy);
            } else
            td_trellis_wave(tq.r->tw, (u32 *)s.patch, &s.coef[4 * it + (lane >> 4)][0], mask16 == 0xffff || ((mask16 >> (4 * it + (lane >> 4))) & 1), s.qmf[cat], tq.r->unq4[cat], tq.r->w4z, tq.r->zz4, tq.r->cabac, dc_out ? 1 : 2,
                            d_trellis_lambda2[cat == 0][Q.qp], dc_out ? 1 : 0, 0, 16, lane);
            }
        WAVE_SYNC();
    }
    if (mine) {
        const u16 *mf = s.qmf[cat], *bs = s.qbias[cat];
        const int *dq = s.qdq[cat];
        int nz = 0, bits = Q.qp / 6 - 4;
        if (tq.on) {
#pragma unroll
            for (int i = 0; i < 16; i++) { c[i] = s.coef[lane][i]; nz |= c[i]; }
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) { int q = quant_one(c[i], mf[i], bs[i]); c[i] = (i16)q; nz |= q; }
        }
        SCAN4_FRAME(lv, c);
        u32 nzm, big;
        LEVEL_MASKS(lv, nzm, big);
#pragma unroll
        for (int i = 0; i < 16; i++) { s.lv_y[16 * lane + i] = lv[i]; s.coef[lane][i] = (i16)dequant_one(c[i], dq[i], bits); }
        s.score[lane] = (nz ? (dc_out ? decimate_masks(nzm >> 1, big >> 1) : decimate_masks(nzm, big)) : 0) | ((nz != 0) << 8);
    }
    WAVE_SYNC();
}
__device__ __forceinline__ void sw_luma4x4_add(SwLds &s, int lane, int keep8, int keep16 = 0xffff)
{
    if (lane < 16 && ((keep8 >> (lane >> 2)) & 1) && (keep16 == 0xffff || ((keep16 >> lane) & 1))) {
        int bx, by, res[16];
        sw_blk_xy(lane, bx, by);
        inv4x4(res, s.coef[lane]);
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                u8 *p = s.fd + FDY + (by + j) * FD + bx + i;
                *p = (u8)clip_u8((int)*p + res[4 * j + i]);
            }
    }
    WAVE_SYNC();
}
__device__ __forceinline__ void sw_ll_i4x4(SwLds &s, int idx, int &cbp_luma, int lane);
__device__ __forceinline__ void sw_ll_i8x8(SwLds &s, int idx, int &cbp_luma, int lane);
__device__ __forceinline__ int sw_ll_luma16(SwLds &s, bool dc_out, int lane);
__device__ __forceinline__ int sw_ll_chroma(SwLds &s, int lane);
// x264_macroblock_encode's inter 4x4-transform branch; returns cbp_luma, fills s.nnz[0..15]
template <class TQ>
__device__ __forceinline__ int sw_encode_inter_luma(SwLds &s, const SwArgs &a, const SwQp &Q, TQ tq, int lane, int *nr_acc4 = nullptr, int nr_on = 0)
{
    if (a.lossless) return sw_ll_luma16(s, false, lane);
    sw_luma4x4_fwd(s, a, Q, tq, 1, false, lane, nr_acc4, nr_on);
    if (lane == 0) {
        int cbp = 0, dec_mb = 0;
        for (int i8 = 0; i8 < 4; i8++) {
            int dec8 = 0, any = 0;
            for (int i4 = 0; i4 < 4; i4++) {
                int v = s.score[4 * i8 + i4];
                s.nnz[4 * i8 + i4] = (u8)(v >> 8);
                if (v >> 8) { any = 1; if (a.dct_decimate && dec8 < 6) dec8 += v & 255; }
            }
            dec_mb += dec8;
            if (a.dct_decimate) {
                if (dec8 < 4) s.nnz[4 * i8] = s.nnz[4 * i8 + 1] = s.nnz[4 * i8 + 2] = s.nnz[4 * i8 + 3] = 0;
                else cbp |= 1 << i8;
            } else if (any) cbp |= 1 << i8;
        }
        if (a.dct_decimate && dec_mb < 6) { cbp = 0; for (int i = 0; i < 16; i++) s.nnz[i] = 0; }
        s.keep8 = cbp;
    }
    WAVE_SYNC();
    const int keep = __builtin_amdgcn_readfirstlane(s.keep8);
    sw_luma4x4_add(s, lane, keep);
    return keep;
}
// x264_mb_encode_i16x16 (prediction already in s.fd); returns cbp_luma, fills s.nnz[0..15], s.nnz[24]
template <class TQ>
__device__ __forceinline__ int sw_encode_i16x16(SwLds &s, const SwArgs &a, const SwQp &Q, TQ tq, int lane, bool b_slice = false)
{
    if (a.lossless) return sw_ll_luma16(s, true, lane);
    sw_luma4x4_fwd(s, a, Q, tq, 0, true, lane);
    i16 d[16], t[16];
    int nz = 0, cbp = 0;
    if (lane == 0) {
        const int b_decimate = b_slice || (a.dct_decimate && a.slice_type == 0);     // macroblock.c:193: B always, P with dct_decimate
        int score = b_decimate ? 0 : 9;
        for (int i = 0; i < 16; i++) {
            int v = s.score[i];
            s.nnz[i] = (u8)(v >> 8);
            if (v >> 8) { if (score < 6) score += v & 255; cbp = 0xf; }
        }
        if (score < 6) { cbp = 0; for (int i = 0; i < 16; i++) s.nnz[i] = 0; }
        // dct4x4dc (R/common/dct.c:39-71), quant_4x4_dc, scan, idct4x4dc, dequant_4x4_dc (quant.c:151-178)
#pragma unroll
        for (int i = 0; i < 16; i++) d[i] = s.dc16[i];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            int p = d[4 * r] + d[4 * r + 1], q = d[4 * r] - d[4 * r + 1], u = d[4 * r + 2] + d[4 * r + 3], w = d[4 * r + 2] - d[4 * r + 3];
            t[r] = (i16)(p + u); t[4 + r] = (i16)(p - u); t[8 + r] = (i16)(q - w); t[12 + r] = (i16)(q + w);
        }
        for (int r = 0; r < 4; r++) {
            int p = t[4 * r] + t[4 * r + 1], q = t[4 * r] - t[4 * r + 1], u = t[4 * r + 2] + t[4 * r + 3], w = t[4 * r + 2] - t[4 * r + 3];
            d[4 * r] = (i16)((p + u + 1) >> 1); d[4 * r + 1] = (i16)((p - u + 1) >> 1);
            d[4 * r + 2] = (i16)((q - w + 1) >> 1); d[4 * r + 3] = (i16)((q + w + 1) >> 1);
        }
        const int mf = (int)s.qmf[0][0] >> 1, bias = (int)s.qbias[0][0] << 1;
        if (tq.on) {
#pragma unroll
            for (int i = 0; i < 16; i++) s.dc16[i] = d[i];
        } else
            for (int i = 0; i < 16; i++) { int q = quant_one(d[i], mf, bias); d[i] = (i16)q; nz |= q; }
    }
    if (tq.on) {                                       // x264_quant_dc_trellis( .., DCT_LUMA_DC, 1 ), macroblock.c:247-248
        WAVE_SYNC();
        td_trellis_wave(tq.r->tw, (u32 *)s.patch, &s.dc16[0], lane < 16, s.qmf[0], tq.r->unq4[0], tq.r->w4z, tq.r->zz4, tq.r->cabac, 0, d_trellis_lambda2[1][Q.qp], 0, 1, 16, lane);
        WAVE_SYNC();
    }
    if (lane == 0) {
        if (tq.on) {
#pragma unroll
            for (int i = 0; i < 16; i++) { d[i] = s.dc16[i]; nz |= d[i]; }
        }
        s.nnz[24] = (u8)(nz != 0);
        if (nz) {
            { i16 lvd[16]; SCAN4_FRAME(lvd, d);
#pragma unroll
              for (int i = 0; i < 16; i++) s.lv_dc[i] = lvd[i]; }
            for (int r = 0; r < 4; r++) {
                int p = d[4 * r] + d[4 * r + 1], q = d[4 * r] - d[4 * r + 1], u = d[4 * r + 2] + d[4 * r + 3], w = d[4 * r + 2] - d[4 * r + 3];
                t[r] = (i16)(p + u); t[4 + r] = (i16)(p - u); t[8 + r] = (i16)(q - w); t[12 + r] = (i16)(q + w);
            }
            for (int r = 0; r < 4; r++) {
                int p = t[4 * r] + t[4 * r + 1], q = t[4 * r] - t[4 * r + 1], u = t[4 * r + 2] + t[4 * r + 3], w = t[4 * r + 2] - t[4 * r + 3];
                d[4 * r] = (i16)(p + u); d[4 * r + 1] = (i16)(p - u); d[4 * r + 2] = (i16)(q - w); d[4 * r + 3] = (i16)(q + w);
            }
            const int m = s.qdq[0][0], bits = Q.qp / 6 - 6;
            for (int i = 0; i < 16; i++) s.dc16[i] = (i16)dequant_one(d[i], m, bits);
        }
        s.keep8 = cbp; s.nzdc16 = nz != 0;
    }
    WAVE_SYNC();
    const int keep = __builtin_amdgcn_readfirstlane(s.keep8), nzdc = __builtin_amdgcn_readfirstlane(s.nzdc16);
    if (keep) {
        if (lane < 16) {
            int bx, by;
            sw_blk_xy(lane, bx, by);
            if (nzdc) s.coef[lane][0] = s.dc16[(by >> 2) * 4 + (bx >> 2)];
        }
        WAVE_SYNC();
        sw_luma4x4_add(s, lane, 0xf);
    } else if (nzdc) {
        // add16x16_idct_dc, R/common/dct.c:369-382
        const int r = lane >> 2, x = (lane & 3) * 4;
        const int dc = (int)(i16)((s.dc16[(r >> 2) * 4 + (x >> 2)] + 32) >> 6);
#pragma unroll
        for (int i = 0; i < 4; i++) { u8 *p = s.fd + FDY + r * FD + x + i; *p = (u8)clip_u8((int)*p + dc); }
        WAVE_SYNC();
    }
    return keep;
}
// x264_mb_encode_8x8_chroma; returns cbp_chroma, fills s.nnz[16..23], s.nnz[25..26]
template <class TQ>
__device__ __forceinline__ int sw_encode_chroma(SwLds &s, const SwArgs &a, const SwQp &Q, TQ tq, int b_inter, int lane)
{
    if (a.lossless) return sw_ll_chroma(s, lane);
    const int cat = 2 + b_inter, b_decimate = b_inter && a.dct_decimate;
    const u16 *mf = s.qmf[cat], *bs = s.qbias[cat];
    i16 c[16], lv[16];
    if (lane < 8) {
        int ch = lane >> 2, i4 = lane & 3, bx = (i4 & 1) * 4, by = (i4 >> 1) * 4, r[16];
        const u8 *fe = s.fe + 256 + 64 * ch, *pr = s.fd + (ch ? FDV : FDU);
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int i = 0; i < 4; i++)
                r[4 * j + i] = (int)fe[(by + j) * 8 + bx + i] - (int)pr[(by + j) * FD + bx + i];
        fwd4x4(c, r);
        s.cdc[lane] = c[0];
        c[0] = 0;                                     // dct2x2dc takes the DCs out (macroblock.c:73-85)
        if (tq.on) {
#pragma unroll
            for (int i = 0; i < 16; i++) s.ccoef[lane][i] = c[i];
        }
    }
    if (tq.on) {                                      // x264_quant_4x4_trellis( .., DCT_CHROMA_AC, !b_inter, 0 ), macroblock.c:310-311
        WAVE_SYNC();
#pragma nounroll
        for (int it = 0; it < 2; it++)
            td_trellis_wave(tq.r->tw, (u32 *)s.patch, &s.ccoef[4 * it + (lane >> 4)][0], true, s.qmf[cat], tq.r->unq4[cat], tq.r->w4z, tq.r->zz4, tq.r->cabac, 4, d_trellis_lambda2[!b_inter][Q.qpc], 1, 0, 16, lane);
        WAVE_SYNC();
    }
    if (lane < 8) {
        const int *dq = s.qdq[cat];
        int nz = 0, bits = Q.qpc / 6 - 4;
        if (tq.on) {
#pragma unroll
            for (int i = 0; i < 16; i++) { c[i] = s.ccoef[lane][i]; nz |= c[i]; }
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) { int q = quant_one(c[i], mf[i], bs[i]); c[i] = (i16)q; nz |= q; }
        }
        SCAN4_FRAME(lv, c);
        u32 nzm, big;
        LEVEL_MASKS(lv, nzm, big);
#pragma unroll
        for (int i = 0; i < 16; i++) { s.lv_cac[16 * lane + i] = lv[i]; s.ccoef[lane][i] = nz ? (i16)dequant_one(c[i], dq[i], bits) : (i16)0; }
        s.cscore[lane] = (nz ? decimate_masks(nzm >> 1, big >> 1) : 0) | ((nz != 0) << 8);
    }
    WAVE_SYNC();
    i16 d2[4] = {0, 0, 0, 0};                          // [0][0] [0][1] [1][0] [1][1]
    if (lane < 2) {
        const int ch = lane;
        int b0 = s.cdc[4 * ch], b1 = s.cdc[4 * ch + 1], b2 = s.cdc[4 * ch + 2], b3 = s.cdc[4 * ch + 3];
        int a0 = b0 + b1, a1 = b2 + b3, a2 = b0 - b1, a3 = b2 - b3;
        d2[0] = (i16)(a0 + a1); d2[1] = (i16)(a0 - a1); d2[2] = (i16)(a2 + a3); d2[3] = (i16)(a2 - a3);
        if (tq.on) { s.cdcout[4 * ch] = d2[0]; s.cdcout[4 * ch + 1] = d2[1]; s.cdcout[4 * ch + 2] = d2[2]; s.cdcout[4 * ch + 3] = d2[3]; }
    }
    if (tq.on) {                                      // x264_quant_dc_trellis( .., DCT_CHROMA_DC, !b_inter ), macroblock.c:325-326
        WAVE_SYNC();
        td_trellis_wave(tq.r->tw, (u32 *)s.patch, &s.cdcout[4 * ((lane >> 4) & 1)], lane < 32, s.qmf[cat], tq.r->unq4[cat], tq.r->w4z, tq.r->zz2, tq.r->cabac, 3, d_trellis_lambda2[!b_inter][Q.qpc], 0, 1, 4, lane);
        WAVE_SYNC();
    }
    if (lane < 2) {
        const int ch = lane;
        int nz_dc = 0;
        if (tq.on) { for (int i = 0; i < 4; i++) { d2[i] = s.cdcout[4 * ch + i]; nz_dc |= d2[i]; } }
        else for (int i = 0; i < 4; i++) { int q = quant_one(d2[i], (int)mf[0] >> 1, (int)bs[0] << 1); d2[i] = (i16)q; nz_dc |= q; }
        int score = 0, nz_ac = 0;
        u8 nzf[4];
        for (int i = 0; i < 4; i++) { int v = s.cscore[4 * ch + i]; nzf[i] = (u8)(v >> 8); if (v >> 8) { nz_ac = 1; if (b_decimate) score += v & 255; } }
        int e0 = d2[0] + d2[1], e1 = d2[2] + d2[3], e2 = d2[0] - d2[1], e3 = d2[2] - d2[3];
        int dmf = s.qdq[cat][0], qbits = Q.qpc / 6 - 5;
        if (qbits > 0) { dmf <<= qbits; qbits = 0; }
        int mode;
        if ((b_decimate && score < 7) || !nz_ac) { nzf[0] = nzf[1] = nzf[2] = nzf[3] = 0; mode = nz_dc ? 1 : 0; }
        else mode = 2;
        const bool put = nz_dc != 0;
        s.lv_cdc[4 * ch] = put ? d2[0] : (i16)0; s.lv_cdc[4 * ch + 1] = put ? d2[2] : (i16)0;
        s.lv_cdc[4 * ch + 2] = put ? d2[1] : (i16)0; s.lv_cdc[4 * ch + 3] = put ? d2[3] : (i16)0;
        s.cdcout[4 * ch + 0] = (i16)((e0 + e1) * dmf >> -qbits); s.cdcout[4 * ch + 1] = (i16)((e0 - e1) * dmf >> -qbits);
        s.cdcout[4 * ch + 2] = (i16)((e2 + e3) * dmf >> -qbits); s.cdcout[4 * ch + 3] = (i16)((e2 - e3) * dmf >> -qbits);
        if (!nz_dc) s.cdcout[4 * ch] = s.cdcout[4 * ch + 1] = s.cdcout[4 * ch + 2] = s.cdcout[4 * ch + 3] = 0;
        s.cmode[ch] = mode | (nz_dc ? 16 : 0);
        for (int i = 0; i < 4; i++) s.nnz[16 + 4 * ch + i] = nzf[i];
        s.nnz[25 + ch] = (u8)(nz_dc != 0);
    }
    WAVE_SYNC();
    if (lane < 8) {
        int ch = lane >> 2, i4 = lane & 3, bx = (i4 & 1) * 4, by = (i4 >> 1) * 4, mode = s.cmode[ch] & 15;
        u8 *pr = s.fd + (ch ? FDV : FDU);
        if (mode == 2) {
            int res[16];
            s.ccoef[lane][0] = s.cdcout[lane];
            inv4x4(res, s.ccoef[lane]);
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int i = 0; i < 4; i++) { u8 *p = pr + (by + j) * FD + bx + i; *p = (u8)clip_u8((int)*p + res[4 * j + i]); }
        } else if (mode == 1) {
            int dc = (int)(i16)((s.cdcout[lane] + 32) >> 6);
            for (int j = 0; j < 4; j++)
                for (int i = 0; i < 4; i++) { u8 *p = pr + (by + j) * FD + bx + i; *p = (u8)clip_u8((int)*p + dc); }
        }
    }
    WAVE_SYNC();
    const int m0 = __builtin_amdgcn_readfirstlane(s.cmode[0]), m1 = __builtin_amdgcn_readfirstlane(s.cmode[1]);
    return ((m0 & 15) == 2 || (m1 & 15) == 2) ? 2 : (((m0 | m1) & 16) ? 1 : 0);
}
// x264_macroblock_probe_skip, P path (R/encoder/macroblock.c:797-883); leaves the P-skip prediction in s.fd
__device__ __forceinline__ int sw_probe_pskip(SwLds &s, const SwRefs &refs, const SwArgs &a, const SwQp &Q, int pmx, int pmy, int mbx, int mby,
                                              ptrdiff_t oy, ptrdiff_t oc, size_t by_, size_t bc_, int lane, bool b_bidir = false)
{
    if (!b_bidir) {                 // x264_macroblock_probe_bskip: the (direct) prediction is in fdec already
        const int vx = clip3(pmx, 4 * (-16 * mbx - 24), 4 * (16 * (a.mb_w - mbx - 1) + 24));
        const int vy = clip3(pmy, 4 * (-16 * mby - 24), 4 * (16 * (a.mb_h - mby - 1) + 24));
        sw_mc16(s, refs, a, 0, vx, vy, oy, oc, by_, bc_, lane, true);
        WAVE_SYNC();
    }
    int score = 0, dc = 0, ssd = 0;
    if (lane < 24) {
        const bool luma = lane < 16;
        int bx, by, r[16];
        const u8 *fe, *pr; int st;
        if (luma) { sw_blk_xy(lane, bx, by); fe = s.fe; pr = s.fd + FDY; st = 16; }
        else { int l = lane - 16, i4 = l & 3; bx = (i4 & 1) * 4; by = (i4 >> 1) * 4; fe = s.fe + 256 + 64 * (l >> 2); pr = s.fd + ((l >> 2) ? FDV : FDU); st = 8; }
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                r[4 * j + i] = (int)fe[(by + j) * st + bx + i] - (int)pr[(by + j) * FD + bx + i];
                ssd += r[4 * j + i] * r[4 * j + i];
            }
        i16 c[16], lv[16];
        fwd4x4(c, r);
        const int cat = luma ? 1 : 3;
        const u16 *mf = s.qmf[cat], *bs = s.qbias[cat];
        if (!luma) { dc = c[0]; c[0] = 0; }
        int nz = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) { int qq = quant_one(c[i], mf[i], bs[i]); c[i] = (i16)qq; nz |= qq; }
        SCAN4_FRAME(lv, c);
        u32 nzm, big;
        LEVEL_MASKS(lv, nzm, big);
        if (nz) score = luma ? decimate_masks(nzm, big) : decimate_masks(nzm >> 1, big >> 1);
    }
    int luma_sum = 0, c_sum[2] = {0, 0}, c_ssd[2] = {0, 0}, c_dc[2][4];
#pragma unroll
    for (int k = 0; k < 16; k++) luma_sum += __builtin_amdgcn_readlane(score, k);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        c_sum[k >> 2] += __builtin_amdgcn_readlane(score, 16 + k);
        c_ssd[k >> 2] += __builtin_amdgcn_readlane(ssd, 16 + k);
        c_dc[k >> 2][k & 3] = __builtin_amdgcn_readlane(dc, 16 + k);
    }
    int ok = luma_sum < 6;
    const u16 *mf = s.qmf[3], *bs = s.qbias[3];
    for (int ch = 0; ch < 2 && ok; ch++) {
        if (c_ssd[ch] < Q.skip_thresh) continue;
        int b0 = c_dc[ch][0], b1 = c_dc[ch][1], b2 = c_dc[ch][2], b3 = c_dc[ch][3];
        int a0 = b0 + b1, a1 = b2 + b3, a2 = b0 - b1, a3 = b2 - b3;
        int d2[4] = {(i16)(a0 + a1), (i16)(a0 - a1), (i16)(a2 + a3), (i16)(a2 - a3)};
        int nzdc = 0;
        for (int i = 0; i < 4; i++) nzdc |= quant_one(d2[i], (int)mf[0] >> 1, (int)bs[0] << 1);
        if (nzdc || c_sum[ch] >= 7) ok = 0;
    }
    return ok;
}

// ---- 8x8 transform path (R/common/dct.c:238-349, quant 8x8, scan, decimate_score64) --------------
// forward transform + quant + scan of the 8x8 luma blocks in `mask`, all at once: lane = (block b, column / row k)
// for the two 1-D passes (32 lanes), then 64 lanes x one coefficient per block.  Leaves the quantised
// coefficients (transposed storage) in s.coef[4*b..][..] = [4][64], levels in s.lv_y8, per block
// s.score[b] = decimate_score64 | nz << 8.  cat: 0 intra, 1 inter.
template <class TQ>
__device__ __forceinline__ void sw_luma8x8_fwd(SwLds &s, const SwQp &Q, TQ tq, int cat, int mask, int lane, int *nr_acc8 = nullptr, int nr_on = 0)
{
    i16 *tmp = s.t8, *coef = &s.coef[0][0];
    const int b = lane >> 3, k8 = lane & 7;
    const bool on = lane < 32 && ((mask >> b) & 1);
    if (on) {
        const u8 *p1 = s.fe + (b >> 1) * 8 * 16 + (b & 1) * 8 + k8, *p2 = s.fd + FDY + (b >> 1) * 8 * FD + (b & 1) * 8 + k8;
        int v[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = (int)p1[k * 16] - (int)p2[k * FD];
        fwd8_1d(o, v);                                 // column k8
#pragma unroll
        for (int k = 0; k < 8; k++) tmp[64 * b + k * 8 + k8] = (i16)o[k];
    }
    WAVE_SYNC();
    if (on) {
        int v[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = tmp[64 * b + k8 * 8 + k];
        fwd8_1d(o, v);                                 // row k8, stored transposed (dct.c:278-283)
#pragma unroll
        for (int k = 0; k < 8; k++) coef[64 * b + k * 8 + k8] = (i16)o[k];
    }
    WAVE_SYNC();
    const int mfl = s.q8mf[cat][lane], bsl = s.q8bias[cat][lane];
    unsigned long long nzmask[4] = {0, 0, 0, 0}, bigmask[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; j++)
        if ((mask >> j) & 1) {
            if (nr_acc8 && nr_on && lane) {      // --nr: lane = coefficient index, the first one is left alone
                int la;
                coef[64 * j + lane] = (i16)sw_denoise(coef[64 * j + lane], s.nr_off8[lane], la);
                *nr_acc8 += la;
            }
            if (!tq.on) {
                int q = quant_one(coef[64 * j + lane], mfl, bsl);
                coef[64 * j + lane] = (i16)q;
                nzmask[j] = __ballot(q != 0);
            }
        }
    WAVE_SYNC();
    if (tq.on) {                                      // x264_quant_8x8_trellis (R/encoder/rdo.c:652-660): one block at a time (its level lists fill the scratch area), sixteen lanes
#pragma nounroll
        for (int j = 0; j < 4; j++)
            if ((mask >> j) & 1) {
                if constexpr (TQ::PSY) {
                    sw_psy_src8(s, tq, j, lane);
                    td_trellis_wave(tq.r->tw, (u32 *)s.patch, coef + 64 * j, lane < 16, s.q8mf[cat], tq.r->unq8[cat], tq.r->w8z, tq.r->zz8, tq.r->cabac, 5, d_trellis_lambda2[cat == 0][Q.qp], 0, 0, 64, lane,
                                    SW_PSY_FENC(s), SwPw8(), tq.psy);
                } else
                td_trellis_wave(tq.r->tw, (u32 *)s.patch, coef + 64 * j, lane < 16, s.q8mf[cat], tq.r->unq8[cat], tq.r->w8z, tq.r->zz8, tq.r->cabac, 5, d_trellis_lambda2[cat == 0][Q.qp], 0, 0, 64, lane);
            }
        WAVE_SYNC();
#pragma unroll
        for (int j = 0; j < 4; j++)
            if ((mask >> j) & 1) nzmask[j] = __ballot(coef[64 * j + lane] != 0);
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
        if ((mask >> j) & 1) {
            int lvv = nzmask[j] ? (int)coef[64 * j + c_scan8[0][lane]] : 0;
            s.lv_y8[64 * j + lane] = (i16)lvv;
            nzmask[j] = __ballot(lvv != 0);
            bigmask[j] = __ballot((unsigned)(lvv + 1) > 2u);
        }
    if (lane < 4 && ((mask >> lane) & 1)) {
        unsigned long long m = lane == 0 ? nzmask[0] : lane == 1 ? nzmask[1] : lane == 2 ? nzmask[2] : nzmask[3];
        unsigned long long bg = lane == 0 ? bigmask[0] : lane == 1 ? bigmask[1] : lane == 2 ? bigmask[2] : bigmask[3];
        int sc = 0;
        if (bg) sc = 9;
        else {
            int idx = m ? 63 - __clzll(m) : -1;
            while (idx >= 0) {
                unsigned long long below = idx ? (m & ((1ull << idx) - 1)) : 0ull;
                int prev = below ? 63 - __clzll(below) : -1;
                sc += c_decimate8[idx - prev - 1];
                idx = prev;
            }
        }
        s.score[lane] = sc | ((m != 0) << 8);
    }
    WAVE_SYNC();
}
// dequant + inverse 8x8 + add for the blocks in `keep`
__device__ __forceinline__ void sw_luma8x8_add(SwLds &s, int cat, int qp, int keep, int lane)
{
    i16 *coef = &s.coef[0][0];
    const int b = lane >> 3, k8 = lane & 7, bits = qp / 6 - 6, dql = s.q8dq[cat][lane];
#pragma unroll
    for (int j = 0; j < 4; j++)
        if ((keep >> j) & 1) {
            int v = dequant_one(coef[64 * j + lane], dql, bits);
            if (lane == 0) v = (int)(i16)(v + 32);           // rounding term, dct.c:326
            coef[64 * j + lane] = (i16)v;
        }
    WAVE_SYNC();
    const bool on = lane < 32 && ((keep >> b) & 1);
    if (on) {
        int v[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = coef[64 * b + k * 8 + k8];
        inv8_1d(o, v);
#pragma unroll
        for (int k = 0; k < 8; k++) coef[64 * b + k * 8 + k8] = (i16)o[k];
    }
    WAVE_SYNC();
    if (on) {
        u8 *dst = s.fd + FDY + (b >> 1) * 8 * FD + (b & 1) * 8;
        int v[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = coef[64 * b + k8 * 8 + k];
        inv8_1d(o, v);
#pragma unroll
        for (int k = 0; k < 8; k++) { u8 *p = dst + k8 + k * FD; *p = (u8)clip_u8((int)*p + (o[k] >> 6)); }
    }
    WAVE_SYNC();
}
// inter, 8x8 transform (R/encoder/macroblock.c:627-669); returns cbp_luma, fills s.nnz[0..15]
template <class TQ>
__device__ __forceinline__ int sw_encode_inter_luma8(SwLds &s, const SwArgs &a, const SwQp &Q, TQ tq, int lane, int *nr_acc8 = nullptr, int nr_on = 0)
{
    sw_luma8x8_fwd(s, Q, tq, 1, 0xf, lane, nr_acc8, nr_on);
    const int b_decimate = a.dct_decimate && !tq.on;           // "8x8 trellis is inherently optimal decimation", macroblock.c:630
    int cbp = 0, dec_mb = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int v = __builtin_amdgcn_readfirstlane(s.score[i]);
        if (v >> 8) {
            if (b_decimate) { dec_mb += v & 255; if ((v & 255) >= 4) cbp |= 1 << i; }
            else cbp |= 1 << i;
        }
    }
    if (b_decimate && dec_mb < 6) cbp = 0;
    if (lane < 16) s.nnz[lane] = (u8)((cbp >> (lane >> 2)) & 1);
    WAVE_SYNC();
    sw_luma8x8_add(s, 1, Q.qp, cbp, lane);
    return cbp;
}
// x264_mb_encode_i8x8 for block idx (prediction already in s.fd)
template <class TQ>
__device__ __forceinline__ void sw_encode_i8x8(SwLds &s, const SwArgs &a, const SwQp &Q, TQ tq, int idx, int &cbp_luma, int lane)
{
    if (a.lossless) { sw_ll_i8x8(s, idx, cbp_luma, lane); return; }
    sw_luma8x8_fwd(s, Q, tq, 0, 1 << idx, lane);
    const int nz = (__builtin_amdgcn_readfirstlane(s.score[idx]) >> 8) & 1;
    if (lane < 4) s.nnz[4 * idx + lane] = (u8)nz;
    WAVE_SYNC();
    if (nz) { cbp_luma |= 1 << idx; sw_luma8x8_add(s, 0, Q.qp, 1 << idx, lane); }
}
// x264_mb_encode_i4x4 for block idx (prediction already in s.fd): one lane per coefficient (the four 16-lane rows of the
// wave run the same block; only the first stores).  The 1-D transforms work on the four values of a quad (DPP
// broadcasts); between the passes the 4x4 is transposed with one ds_bpermute, so after the forward pair lane i holds
// dct[i] in the reference's (transposed) storage order and the quantiser rows / zigzag are indexed by the lane.
__device__ __forceinline__ void sw_quad4(int v, int &v0, int &v1, int &v2, int &v3)
{
    v0 = __builtin_amdgcn_update_dpp(0, v, 0x00, 0xf, 0xf, false); v1 = __builtin_amdgcn_update_dpp(0, v, 0x55, 0xf, 0xf, false);
    v2 = __builtin_amdgcn_update_dpp(0, v, 0xAA, 0xf, 0xf, false); v3 = __builtin_amdgcn_update_dpp(0, v, 0xFF, 0xf, 0xf, false);
}
__device__ __forceinline__ int sw_fwd4_quad(int v, int k)        // dct.c:122-145, one 1-D pass: output k of this quad's four inputs
{
    int v0, v1, v2, v3;
    sw_quad4(v, v0, v1, v2, v3);
    const int s03 = v0 + v3, s12 = v1 + v2, d03 = v0 - v3, d12 = v1 - v2;
    return (int)(i16)(k == 0 ? s03 + s12 : k == 1 ? 2 * d03 + d12 : k == 2 ? s03 - s12 : d03 - 2 * d12);
}
__device__ __forceinline__ int sw_inv4_quad(int v, int k, int last)   // dct.c:174-206
{
    int d0, d1, d2, d3;
    sw_quad4(v, d0, d1, d2, d3);
    const int e = d0 + d2, f = d0 - d2, g = d1 + (d3 >> 1), h = (d1 >> 1) - d3;
    const int r = k == 0 ? e + g : k == 1 ? f + h : k == 2 ? f - h : e - g;
    return (int)(i16)(last ? (r + 32) >> 6 : r);
}
template <class TQ>
__device__ __forceinline__ void sw_encode_i4x4(SwLds &s, const SwArgs &a, const SwQp &Q, TQ tq, int idx, int &cbp_luma, int lane)
{
    if (a.lossless) { sw_ll_i4x4(s, idx, cbp_luma, lane); return; }
    int bx, by;
    sw_blk_xy(idx, bx, by);
    const int l16 = lane & 15, x = l16 & 3, y = l16 >> 2, tl = (lane & 48) | (x << 2) | y;
    int v = (int)s.fe[(by + y) * 16 + bx + x] - (int)s.fd[FDY + (by + y) * FD + bx + x];
    v = sw_fwd4_quad(v, x);
    v = __shfl(v, tl, 64);
    v = sw_fwd4_quad(v, x);                                        // dct[l16]
    int q;
    if (tq.on) {                                      // x264_quant_4x4_trellis( .., DCT_LUMA_4x4, 1, idx ), macroblock.c:134
        if (lane < 16) s.coef[idx][l16] = (i16)v;
        WAVE_SYNC();
        if constexpr (TQ::PSY) {
            sw_psy_src4(s, tq, idx, lane);
            td_trellis_wave(tq.r->tw, (u32 *)s.patch, &s.coef[idx][0], lane < 16, s.qmf[0], tq.r->unq4[0], tq.r->w4z, tq.r->zz4, tq.r->cabac, 2, d_trellis_lambda2[1][Q.qp], 0, 0, 16, lane,
                            SW_PSY_FENC(s), SwPw4(), tq.psy);
        } else
        td_trellis_wave(tq.r->tw, (u32 *)s.patch, &s.coef[idx][0], lane < 16, s.qmf[0], tq.r->unq4[0], tq.r->w4z, tq.r->zz4, tq.r->cabac, 2, d_trellis_lambda2[1][Q.qp], 0, 0, 16, lane);
        WAVE_SYNC();
        q = s.coef[idx][l16];
    } else
        q = quant_one(v, s.qmf[0][l16], s.qbias[0][l16]);
    const int nz = (__ballot(q != 0) & 0xffffull) != 0;
    if (lane == 0) s.nnz[idx] = (u8)nz;
    if (nz) {
        if (lane < 16) s.lv_y[16 * idx + (int)((0xFDC6EB75A8419320ull >> (4 * l16)) & 15)] = (i16)q;      // zigzag position of dct[l16]
        int d = dequant_one(q, s.qdq[0][l16], Q.qp / 6 - 4);
        d = __shfl(d, tl, 64);                                     // lane (c = l16 >> 2, p = l16 & 3) holds dct[4p + c]
        d = sw_inv4_quad(d, x, 0);                                 // ... now mid[l16]
        d = __shfl(d, tl, 64);
        d = sw_inv4_quad(d, x, 1);                                 // ... now the residual of pixel (row x, column y)
        if (lane < 16) { u8 *p = s.fd + FDY + (by + x) * FD + bx + y; *p = (u8)clip_u8((int)*p + d); }
        cbp_luma |= 1 << (idx >> 2);
    }
    WAVE_SYNC();
}

// ---- intra 4x4 / 8x8 analysis helpers ------------------------------------------------------------
// i_neighbour4 / i_neighbour8 (R/common/macroblock.c:733-743, 1172-1186)
// ---- lossless (R/encoder/macroblock.c:123-130,160-167,196-213,288-303,602-626; zigzag_sub_*, R/common/dct.c:564-606) ----
// The levels are the prediction error itself in zigzag order and the reconstruction is the source.  Lane = zigzag position.
#define SW_ZZ4(p) ((int)((0xFBEDA7369C852140ull >> (4 * (p))) & 15))      /* position -> 4 * x + y */
__device__ __forceinline__ void sw_ll_i4x4(SwLds &s, int idx, int &cbp_luma, int lane)
{
    int bx, by;
    sw_blk_xy(idx, bx, by);
    const int c = SW_ZZ4(lane & 15), o_e = (by + (c & 3)) * 16 + bx + (c >> 2), o_d = FDY + (by + (c & 3)) * FD + bx + (c >> 2);
    const int v = (int)s.fe[o_e] - (int)s.fd[o_d];
    const int nz = (__ballot(v != 0) & 0xffffull) != 0;
    if (lane < 16) { s.lv_y[16 * idx + lane] = (i16)v; s.fd[o_d] = s.fe[o_e]; }
    if (lane == 0) s.nnz[idx] = (u8)nz;
    cbp_luma |= nz << (idx >> 2);
    WAVE_SYNC();
}
__device__ __forceinline__ void sw_ll_i8x8(SwLds &s, int idx, int &cbp_luma, int lane)
{
    const int c = c_scan8[0][lane], bx = 8 * (idx & 1), by = 8 * (idx >> 1);
    const int o_e = (by + (c & 7)) * 16 + bx + (c >> 3), o_d = FDY + (by + (c & 7)) * FD + bx + (c >> 3);
    const int v = (int)s.fe[o_e] - (int)s.fd[o_d];
    const int nz = __ballot(v != 0) != 0;
    s.lv_y8[64 * idx + lane] = (i16)v; s.fd[o_d] = s.fe[o_e];
    if (lane < 4) s.nnz[4 * idx + lane] = (u8)nz;
    cbp_luma |= nz << idx;
    WAVE_SYNC();
}
// the 16 luma 4x4 blocks (inter, or I_16x16 with dc_out: the first level of every block goes to the DC block); returns cbp_luma
__device__ __forceinline__ int sw_ll_luma16(SwLds &s, bool dc_out, int lane)
{
    int cbp = 0, dc_any = 0;
#pragma unroll
    for (int pass = 0; pass < 4; pass++) {
        const int blk = 4 * pass + (lane >> 4), p = lane & 15, c = SW_ZZ4(p);
        int bx, by;
        sw_blk_xy(blk, bx, by);
        const int o_e = (by + (c & 3)) * 16 + bx + (c >> 2), o_d = FDY + (by + (c & 3)) * FD + bx + (c >> 2);
        int v = (int)s.fe[o_e] - (int)s.fd[o_d];
        s.fd[o_d] = s.fe[o_e];
        if (dc_out) {
            dc_any |= __ballot(p == 0 && v != 0) != 0;
            if (p == 0) { s.dc16[(bx >> 2) * 4 + (by >> 2)] = (i16)v; v = 0; }
        }
        s.lv_y[16 * blk + p] = (i16)v;
        const unsigned long long m = __ballot(v != 0);
        if (lane < 4) s.nnz[4 * pass + lane] = (u8)(((m >> (16 * lane)) & 0xffffull) != 0);
        if (m) cbp |= dc_out ? 0xf : 1 << pass;
    }
    if (dc_out) {
        WAVE_SYNC();
        if (lane < 16) s.lv_dc[lane] = s.dc16[SW_ZZ4(lane)];
        if (lane == 0) s.nnz[24] = (u8)dc_any;
    }
    WAVE_SYNC();
    return cbp;
}
// both chroma planes; returns cbp_chroma
__device__ __forceinline__ int sw_ll_chroma(SwLds &s, int lane)
{
    int ac = 0, dc = 0;
#pragma unroll
    for (int ch = 0; ch < 2; ch++) {
        const int blk = lane >> 4, p = lane & 15, c = SW_ZZ4(p), bx = (blk & 1) * 4, by = (blk >> 1) * 4;
        const int o_e = 256 + 64 * ch + (by + (c & 3)) * 8 + bx + (c >> 2), o_d = (ch ? FDV : FDU) + (by + (c & 3)) * FD + bx + (c >> 2);
        int v = (int)s.fe[o_e] - (int)s.fd[o_d];
        s.fd[o_d] = s.fe[o_e];
        const unsigned long long md = __ballot(p == 0 && v != 0);
        if (p == 0) { s.lv_cdc[4 * ch + blk] = (i16)v; v = 0; }
        s.lv_cac[(4 * ch + blk) * 16 + p] = (i16)v;
        const unsigned long long m = __ballot(v != 0);
        if (lane < 4) s.nnz[16 + 4 * ch + lane] = (u8)(((m >> (16 * lane)) & 0xffffull) != 0);
        if (lane == 0) s.nnz[25 + ch] = (u8)(md != 0);
        ac |= m != 0; dc |= md != 0;
    }
    WAVE_SYNC();
    return ac ? 2 : dc ? 1 : 0;
}
__device__ __forceinline__ int sw_nb4(int idx, int nb)
{
    const int all = NB_LEFT | NB_TOP | NB_TOPLEFT | NB_TOPRIGHT;
    switch (idx) {
    case 0: return (nb & (NB_TOP | NB_LEFT | NB_TOPLEFT)) | ((nb & NB_TOP) ? NB_TOPRIGHT : 0);
    case 1: case 4: return NB_LEFT | ((nb & NB_TOP) ? (NB_TOP | NB_TOPLEFT | NB_TOPRIGHT) : 0);
    case 2: case 8: case 10: return NB_TOP | NB_TOPRIGHT | ((nb & NB_LEFT) ? (NB_LEFT | NB_TOPLEFT) : 0);
    case 5: return NB_LEFT | (nb & NB_TOPRIGHT) | ((nb & NB_TOP) ? NB_TOP | NB_TOPLEFT : 0);
    case 6: case 9: case 12: case 14: return all;
    default: return NB_LEFT | NB_TOP | NB_TOPLEFT;          // 3 7 11 13 15
    }
}
__device__ __forceinline__ int sw_nb8(int idx, int nb)
{
    switch (idx) {
    case 0: return (nb & (NB_TOP | NB_LEFT | NB_TOPLEFT)) | ((nb & NB_TOP) ? NB_TOPRIGHT : 0);
    case 1: return NB_LEFT | (nb & NB_TOPRIGHT) | ((nb & NB_TOP) ? NB_TOP | NB_TOPLEFT : 0);
    case 2: return NB_TOP | NB_TOPRIGHT | ((nb & NB_LEFT) ? (NB_LEFT | NB_TOPLEFT) : 0);
    default: return NB_LEFT | NB_TOP | NB_TOPLEFT;
    }
}
// predict_4x4_mode_available (R/encoder/analyse.c:435-471) as a nibble list: mode i = (list >> 4i) & 15
__device__ __forceinline__ unsigned long long sw_modes4(int nb, int &n)
{
    if ((nb & NB_LEFT) && (nb & NB_TOP)) {
        if (nb & NB_TOPLEFT) { n = 9; return 0x876543012ull; }
        n = 6; return 0x873012ull;
    }
    if (nb & NB_LEFT) { n = 3; return 0x819ull; }
    if (nb & NB_TOP) { n = 4; return 0x730Aull; }
    n = 1; return 0xBull;
}
// x264_mb_predict_intra4x4_mode on the sweep's mode cache
__device__ __forceinline__ int sw_pred_i4mode(const SwLds &s, int idx)
{
    return mb_pred_i4mode(__builtin_amdgcn_readfirstlane((int)s.i4c[mb_scan8_luma(idx) - 1]), __builtin_amdgcn_readfirstlane((int)s.i4c[mb_scan8_luma(idx) - 8]));
}
// SATD / SAD of a 4x4 block from one row of differences per lane (rows of a block in lanes l, l^1, l^2, l^3); pixel.c:187-212
__device__ __forceinline__ int sw_cost4x4_rows(int d0, int d1, int d2, int d3, int satd, int lane)
{
    if (!satd) return quad_sum4(iabs(d0) + iabs(d1) + iabs(d2) + iabs(d3));
    const u32 e0 = (u32)(d0 + d1) + ((u32)(d0 - d1) << 16), e1 = (u32)(d2 + d3) + ((u32)(d2 - d3) << 16);
    u32 c[2] = {e0 + e1, e0 - e1}, acc = 0;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        u32 v = c[k], o = (u32)dpp_mov<DPP_XOR1>((int)v);
        v = (lane & 1) ? o - v : v + o;
        o = (u32)dpp_mov<DPP_XOR2>((int)v);
        v = (lane & 2) ? o - v : v + o;
        acc += lanes_abs(v);
    }
    acc = (u32)quad_sum4((int)acc);
    return (int)(((acc & 0xffffu) + (acc >> 16)) >> 1);
}
// unnormalised 8x8 Hadamard SATD of a block from one row per lane (rows in 8 consecutive lanes); pixel.c:256-289
__device__ __forceinline__ int sw_sa8d_rows(const u8 *f, const u8 *p, int lane)
{
    u32 e[4], t[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int d0 = (int)f[2 * k] - (int)p[2 * k], d1 = (int)f[2 * k + 1] - (int)p[2 * k + 1];
        e[k] = (u32)(d0 + d1) + ((u32)(d0 - d1) << 16);
    }
    wht4(t[0], t[1], t[2], t[3], e[0], e[1], e[2], e[3]);
    u32 acc = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        u32 v = t[k], o = (u32)dpp_mov<DPP_XOR1>((int)v);
        v = (lane & 1) ? o - v : v + o;
        o = (u32)dpp_mov<DPP_XOR2>((int)v);
        v = (lane & 2) ? o - v : v + o;
        o = (u32)__shfl_xor((int)v, 4, 64);
        v = (lane & 4) ? o - v : v + o;
        acc += lanes_abs(v);
    }
    return half_sum8((int)((acc & 0xffffu) + (acc >> 16)));
}

// the 4x4 block's prediction table (intra_pred.h) from the pixels around dst (stride FD): 13 edge samples, their two- and
// three-tap filtered forms, the three DC values and 128
__device__ __forceinline__ void sw_pred4_table(SwLds &s, const u8 *dst, int lane)
{
    const int k = lane < 13 ? lane : 12;
    const int e = (int)(k < 4 ? dst[-1 + (3 - k) * FD] : k == 4 ? dst[-1 - FD] : dst[(k - 5) - FD]);
    int prev = dpp_mov<0x111>(e), next = dpp_mov<0x101>(e);      // row_shr:1 / row_shl:1: lanes k - 1 / k + 1
    if (lane == 0) prev = e;
    if (lane >= 12) next = e;
    if (lane < 13) { s.pt4[lane] = (u8)e; s.pt4[13 + lane] = (u8)((e + next + 1) >> 1); s.pt4[26 + lane] = (u8)((prev + 2 * e + next + 2) >> 2); }
    int dv = 0;
    if (lane >= 16 && lane < 20) dv = dst[(lane - 16) - FD];
    else if (lane >= 20 && lane < 24) dv = dst[-1 + (lane - 20) * FD];
    dv = quad_sum4(dv);
    const int t = __builtin_amdgcn_readlane(dv, 16), l = __builtin_amdgcn_readlane(dv, 20);
    if (lane >= 24 && lane < 28) s.pt4[39 + lane - 24] = (u8)(lane == 24 ? (t + l + 4) >> 3 : lane == 25 ? (l + 2) >> 2 : lane == 26 ? (t + 2) >> 2 : 128);
}
// x264_predict_8x8_filter with every filter on (R/common/predict.c:499-540): one lane per edge entry 7..32
__device__ __forceinline__ void sw_pred8_filter_all(u8 *edge, const u8 *src, int neigh, int lane)
{
#define PX(xx, yy) ((int)src[(xx) + (yy) * FD])
    const int have_tl = neigh & NB_TOPLEFT, have_tr = neigh & NB_TOPRIGHT;
    if (lane < 26) {
        const int i = 7 + lane;
        int av, bv, cv;
        if (i < 15) {                                    // left y = 14 - i
            const int y = 14 - i;
            av = y == 0 ? (have_tl ? PX(-1, -1) : PX(-1, 0)) : PX(-1, y - 1); bv = PX(-1, y); cv = y == 7 ? PX(-1, 7) : PX(-1, y + 1);
        } else if (i == 15) { av = PX(0, -1); bv = PX(-1, -1); cv = PX(-1, 0); }
        else if (i < 24) {                               // top x = i - 16
            const int x = i - 16;
            av = x == 0 ? (have_tl ? PX(-1, -1) : PX(0, -1)) : PX(x - 1, -1); bv = PX(x, -1); cv = x == 7 ? (have_tr ? PX(8, -1) : PX(7, -1)) : PX(x + 1, -1);
        } else if (have_tr) {                            // top right x = 8 .. 15, edge[32] = edge[31]
            const int x = i < 32 ? i - 16 : 15;
            av = PX(x - 1, -1); bv = PX(x, -1); cv = x == 15 ? PX(15, -1) : PX(x + 1, -1);
        } else av = bv = cv = PX(7, -1);
        edge[i] = (u8)((av + 2 * bv + cv + 2) >> 2);
    }
#undef PX
}
// the 8x8 block's prediction table from the filtered edge array (e[j] = edge[7 + j], j = 0..24)
__device__ __forceinline__ void sw_pred8_table(SwLds &s, int lane)
{
    if (lane < 25) {
        const int e = s.edge8[7 + lane], prev = lane == 0 ? e : (int)s.edge8[6 + lane], next = lane == 24 ? e : (int)s.edge8[8 + lane];
        s.pt8[lane] = (u8)e; s.pt8[25 + lane] = (u8)((e + next + 1) >> 1); s.pt8[50 + lane] = (u8)((prev + 2 * e + next + 2) >> 2);
    }
    int dv = 0;
    if (lane >= 32 && lane < 40) dv = s.edge8[16 + lane - 32];
    else if (lane >= 40 && lane < 48) dv = s.edge8[7 + lane - 40];
    dv = half_sum8(dv);
    const int t = __builtin_amdgcn_readlane(dv, 32), l = __builtin_amdgcn_readlane(dv, 40);
    if (lane >= 48 && lane < 52) s.pt8[75 + lane - 48] = (u8)(lane == 48 ? (l + t + 8) >> 4 : lane == 49 ? (l + 4) >> 3 : lane == 50 ? (t + 4) >> 3 : 128);
}
// unnormalised 8x8 Hadamard SATD from one row of differences per lane (rows in 8 consecutive lanes); pixel.c:256-289
__device__ __forceinline__ int sw_sa8d_rows_d(const int d[8], int lane)
{
    u32 e[4], t[4];
#pragma unroll
    for (int k = 0; k < 4; k++) e[k] = (u32)(d[2 * k] + d[2 * k + 1]) + ((u32)(d[2 * k] - d[2 * k + 1]) << 16);
    wht4(t[0], t[1], t[2], t[3], e[0], e[1], e[2], e[3]);
    u32 acc = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        u32 v = t[k], o = (u32)dpp_mov<DPP_XOR1>((int)v);
        v = (lane & 1) ? o - v : v + o;
        o = (u32)dpp_mov<DPP_XOR2>((int)v);
        v = (lane & 2) ? o - v : v + o;
        const u32 up = (u32)dpp_mov<0x104>((int)v), dn = (u32)dpp_mov<0x114>((int)v);     // row_shl:4 / row_shr:4: lanes + 4 / - 4 (both run in all lanes)
        o = (lane & 4) ? dn : up;                                                          // = lane ^ 4
        v = (lane & 4) ? o - v : v + o;
        acc += lanes_abs(v);
    }
    return half_sum8((int)((acc & 0xffffu) + (acc >> 16)));
}

// x264_mb_analyse_inter_p4x4_chroma (R/encoder/analyse.c:1373-1405): mc_chroma of the 8x8 block's sub-partitions into one 4x4 per
// plane, then mbcmp 4x4 against the source.  Lane = plane * 4 + row (lanes 8.. repeat the work); every pixel takes the vector
// of the sub-block that covers it (sub = 0 four 2x2, 1 two 4x2, 2 two 2x4), read from the lane-indexed records at rec0 + k.
__device__ __forceinline__ int sw_sub_chroma(const SwLds &s, const SwRefs &refs, const SwArgs &a, int r, int i8, int sub, int rec0, int sub_mx, int sub_my,
                                             int satd, ptrdiff_t oc, size_t bc, int lane)
{
    const int pl = (lane >> 2) & 1, y = lane & 3;
    const u8 *plane = (pl ? refs.v[r] : refs.u[r]) + bc + oc + 4 * (i8 & 1) + (ptrdiff_t)(4 * (i8 >> 1)) * a.sc;
    const u8 *src = s.fe + 256 + 64 * pl + (4 * (i8 >> 1) + y) * 8 + 4 * (i8 & 1);
    int d[4];
#pragma unroll
    for (int x = 0; x < 4; x++) {
        const int k = sub == 0 ? (y >> 1) * 2 + (x >> 1) : sub == 1 ? (y >> 1) : (x >> 1);
        const int mvx = __shfl(sub_mx, rec0 + k, 64), mvy = __shfl(sub_my, rec0 + k, 64);
        const int dx = mvx & 7, dy = mvy & 7;
        const u8 *p = plane + (ptrdiff_t)(y + (mvy >> 3)) * a.sc + x + (mvx >> 3);
        const int v = ((8 - dx) * (8 - dy) * p[0] + dx * (8 - dy) * p[1] + (8 - dx) * dy * p[a.sc] + dx * dy * p[a.sc + 1] + 32) >> 6;
        d[x] = (int)src[x] - v;
    }
    const int c4 = sw_cost4x4_rows(d[0], d[1], d[2], d[3], satd, lane);
    return __builtin_amdgcn_readlane(c4, 0) + __builtin_amdgcn_readlane(c4, 4);
}

__device__ __forceinline__ int sw_load_acq(const int *p) { return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT); }

// WPE = waves per SIMD the register allocation is held to.  A row wave spends most of its time waiting
// on dependent LDS / L2 round trips, so throughput comes from other chains' waves filling those gaps:
// fewer registers per wave (some spilled) and more waves resident beats one fat wave per SIMD.
// LL: lossless, as a compile-time constant (its branches cost the usual path nothing)
// RD: the raster-order variant.  With the RD levels (the trial encodes are priced against the live CABAC contexts), trellis
// (same) or adaptive quantisation (a macroblock's QP follows from the previous one's, R/encoder/ratecontrol.c:263-264) a slice is
// one serial chain of macroblocks; one wavefront then owns a whole frame of one chain and walks it in raster order, rows and all,
// and the entropy coder (cabac_dev.h) runs inside the loop exactly where x264_slice_write has it.  Throughput comes from the
// number of frames in flight (grid = batch), not from a wavefront schedule inside the frame.
static __device__ const u8 d_lambda_tab[52] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 6,
                                               6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 23, 25, 29, 32, 36, 40, 45, 51, 57, 64, 72, 81, 91};
static __device__ const int d_lambda2_tab[52] = {14, 18, 22, 28, 36, 45, 57, 72, 91, 115, 145, 182, 230, 290, 365, 460, 580, 731, 921, 1161, 1462, 1843, 2322, 2925,
    3686, 4644, 5851, 7372, 9289, 11703, 14745, 18578, 23407, 29491, 37156, 46814, 58982, 74313, 93628, 117964,
    148626, 187257, 235929, 297252, 374514, 471859, 594505, 749029, 943718, 1189010, 1498059, 1887436};
static __device__ const u8 d_chroma_qp[52] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
                                              29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39};

// RF: the I / P kernel with the RD refinement of subme 8-9 (x264_me_refine_qpel_rd, x264_intra_rd_refine: slice_refine.h)
// CH: the chain-table launch.  Chains that no longer move in lock step (adaptive B placement, per-chain QPs) each code their own
// frame type from their own pictures: block i takes ALL three argument structures from tab[i], built by the host exactly as for a
// launch of its own (x264hip_slice_sweep_chains), and codes batch element tab[i].a.chain.  The table is read through the constant
// address space, like the kernel-argument segment it replaces, so the same loads can be re-issued instead of kept in registers.
struct SwDesc { SwArgs a; SwRefs t; SwRd r; };
// The body of the sweep is slice_sweep_body.h, textually included (like slice_b_flow.h and slice_refine.h inside it) by the two kernel
// templates below.  Textually, not as a shared __device__ function: with the body in an always-inlined function template the code
// objects of EVERY existing instantiation came out different (other register allocation throughout; the extended B kernels went from
// 12-20 to about 200 bytes of private segment), and the lossy kernels must stay the ones that were measured.  Included, k_slice_sweep is
// token for token the kernel it was.
template <int WPE, bool LL = false, bool RD = false, bool BS = false, bool TD = false, bool RF = false, bool CH = false>       // TD: the extended B kernel (temporal direct prediction, lookahead candidates)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE))) void k_slice_sweep(SwArgs a, SwRefs refs_k, SwRd rd_k, const SwDesc *tab)
{
    constexpr bool PT = false;
#include "slice_sweep_body.h"
}

// The raster variant with lossless on (constant QP 0, h->mb.b_lossless): I and P slices with the CABAC writer in the loop, subme 0..9.
// Kernels of their own name -- the lossy raster kernels' instantiations stay the ones they were -- over the same body.  No DCT,
// quantiser, trellis or psy code is left in them (LL is a compile-time constant), so 256 registers hold the subme <= 7 body without a
// spill; the refinement variant (RF) gets a whole SIMD's register file (one wave per SIMD) instead of scratch memory.
template <bool RF, bool CH>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RF ? 1 : 2))) void k_lossless_raster(SwArgs a, SwRefs refs_k, SwRd rd_k, const SwDesc *tab)
{
    constexpr bool LL = true, RD = true, BS = false, TD = false, PT = false;
#include "slice_sweep_body.h"
}

// The lossy raster variant with psy-trellis (--psy-rd A:B with B > 0 under --trellis 1 or 2; PT, a compile-time constant that is false in the two
// templates above): the trellis quantiser's price of a luma coefficient gains rdo.c:555-562's term.  Kernels of their own name over the same body, like the
// lossless ones and for the same reason.  One B kernel, the extended one (TD): a lock-step B launch with psy-trellis goes there as a table's
// does.  All of them are allowed a whole SIMD's register file (one wave per SIMD where they take it) instead of scratch memory: held to 256 registers
// the chain-table I / P body and the B bodies spilled 4 to 47 registers with the psy code in them, and a kernel of this name may not spill.
template <bool BS, bool TD, bool RF, bool CH>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1))) void k_psy_raster(SwArgs a, SwRefs refs_k, SwRd rd_k, const SwDesc *tab)
{
    constexpr bool LL = false, RD = true, PT = true;
#include "slice_sweep_body.h"
}

// The two launches of the raster kernels.  Every instantiation has a translation unit of its own (frame_slice_<kind>.hip the lock-step
// launch, frame_slice_<kind>_ch.hip the chain-table one) so that the kernels compile side by side; each of them names its kernel here.
typedef void SwKernel(SwArgs, SwRefs, SwRd, const SwDesc *);
// lock-step: one block per chain of the batch, all of them with the arguments of the launch
static inline void sw_launch_frame(SwKernel *kernel, const SwArgs &a, const SwRefs &t, const SwRd &r, hipStream_t stream)
{
    hipLaunchKernelGGL(kernel, dim3((unsigned)a.batch), dim3(64), 0, stream, a, t, r, nullptr);
}
// chain table: block i takes its arguments from tab[i] (CH), and the launch's own are dummies
static inline void sw_launch_chains(SwKernel *kernel, const SwDesc *tab, int n, hipStream_t stream)
{
    SwArgs a; SwRefs t; SwRd r;
    memset(&a, 0, sizeof(a)); memset(&t, 0, sizeof(t)); memset(&r, 0, sizeof(r));
    hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3(64), 0, stream, a, t, r, tab);
}

// the launch functions of the instantiation files, and the table of kinds in which the host side finds them
#include "sweep_tables.h"
