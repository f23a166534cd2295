// sweep_tables.h -- the two tables the host side of the sweep walks (frame_slice.hip): the device arrays of an x264hip_mb_state, and
// the kernel variants ("kinds") of the sweep with everything the host decides about a launch: which kind codes a sweep, which kinds one
// chain table may hold, where its entries go, and which launch function runs on which stream.  Plain C++ over names its includer
// provides -- x264hip_mb_state (x264hip.h); SwArgs, SwRefs, SwRd, SwDesc, SW_MAX_REFS and hipStream_t (slice_kernel.h, which includes
// this file at its end) -- so that tests/sweep_tables_host.cpp compiles the same tables and walks for the host alone, with stand-ins
// for the launch functions.
#pragma once
#include <stddef.h>

// ---- the device arrays of an x264hip_mb_state, in the order x264hip_mb_state_alloc_ex allocates them
struct StateArray {
    size_t member;      // offsetof(x264hip_mb_state, ...): every one of them is a pointer
    int mb_bytes;       // bytes per macroblock; 0: `progress`, a word per macroblock row of every chain and the abort flag behind them
    bool level;         // a level array: 816 of a macroblock's 1184 bytes, left out with X264HIP_STATE_NO_LEVELS
};
#define SW_STATE_ARRAY(m, mb_bytes, level) {offsetof(x264hip_mb_state, m), mb_bytes, level}
static const StateArray k_state_arrays[] = {
    SW_STATE_ARRAY(mb_type, 1, false), SW_STATE_ARRAY(partition, 1, false), SW_STATE_ARRAY(sub_partition, 4, false), SW_STATE_ARRAY(ref, 4, false),
    SW_STATE_ARRAY(i4mode, 16, false), SW_STATE_ARRAY(i16mode, 1, false), SW_STATE_ARRAY(chroma_mode, 1, false), SW_STATE_ARRAY(qp, 1, false),
    SW_STATE_ARRAY(t8, 1, false), SW_STATE_ARRAY(mv, 64, false), SW_STATE_ARRAY(mvr, 4 * SW_MAX_REFS, false), SW_STATE_ARRAY(cbp, 2, false),
    SW_STATE_ARRAY(nnz, 27, false), SW_STATE_ARRAY(luma, 512, true), SW_STATE_ARRAY(luma_dc, 32, true), SW_STATE_ARRAY(chroma_dc, 16, true),
    SW_STATE_ARRAY(chroma_ac, 256, true), SW_STATE_ARRAY(cost_intra, 4, false), SW_STATE_ARRAY(cost_inter, 4, false),
    SW_STATE_ARRAY(cost_intra_alt, 4, false), SW_STATE_ARRAY(progress, 0, false), SW_STATE_ARRAY(mvd, 64, false), SW_STATE_ARRAY(mv1, 64, false),
    SW_STATE_ARRAY(ref1, 4, false), SW_STATE_ARRAY(mvr1, 4, false), SW_STATE_ARRAY(mvd1, 64, false), SW_STATE_ARRAY(skipbp, 1, false)};
#undef SW_STATE_ARRAY
static inline size_t state_progress_bytes(int mb_h, int batch) { return sizeof(int) * ((size_t)mb_h * batch + 1); }
static inline size_t state_array_bytes(const StateArray &s, int mb_w, int mb_h, int batch)
{
    return s.mb_bytes ? (size_t)s.mb_bytes * ((size_t)mb_w * mb_h * batch) : state_progress_bytes(mb_h, batch);
}
static inline void **state_array(x264hip_mb_state *st, const StateArray &s) { return (void **)((char *)st + s.member); }

// ---- the kinds of sweep: one row per kernel variant, and the one place a new variant is registered.  The rows stand in the order
// in which a chain-table launch enqueues its kernels -- the I / P kernels first: their wavefronts, the step's long ones, are dealt
// evenly over the SIMDs before the B kernel's fill the rest -- and the table's entries are sorted in the same order: [RD | RF | BT],
// [LL | LL_RF] or [PSY_RD | PSY_RF | PSY_BT].  A table is of one family or refused (sweep_mixed_family), so where the families stand
// relative to each other changes no sequence of launches there can be.
enum { SW_KIND_PLAIN = 0, SW_KIND_RD, SW_KIND_RF, SW_KIND_LL, SW_KIND_LL_RF, SW_KIND_B, SW_KIND_BT, SW_KIND_PSY_RD, SW_KIND_PSY_RF, SW_KIND_PSY_BT, SW_N_KINDS };
enum { SW_LOSSY = 0, SW_LOSSLESS, SW_PSY, SW_N_FAMILIES };      // lossless: k_lossless_raster; psy-trellis: k_psy_raster; lossy: the rest, k_slice_sweep
typedef void SwLaunch(const SwArgs &a, const SwRefs &t, const SwRd &r, hipStream_t stream);     // a lock-step launch (frame_slice_<kind>.hip; PLAIN: frame_slice.hip)
typedef void SwLaunchChains(const SwDesc *tab, int n, hipStream_t stream);                       // a chain-table launch (frame_slice_<kind>_ch.hip)
SwLaunch x264hip_launch_slice_plain, x264hip_launch_slice_rd, x264hip_launch_slice_rf, x264hip_launch_slice_ll, x264hip_launch_slice_ll_rf, x264hip_launch_slice_b,
    x264hip_launch_slice_bt, x264hip_launch_psy_rd, x264hip_launch_psy_rf, x264hip_launch_psy_bt;
SwLaunchChains x264hip_launch_slice_rd_ch, x264hip_launch_slice_rf_ch, x264hip_launch_slice_ll_ch, x264hip_launch_slice_ll_rf_ch, x264hip_launch_slice_bt_ch,
    x264hip_launch_psy_rd_ch, x264hip_launch_psy_rf_ch, x264hip_launch_psy_bt_ch;
struct SwKind {
    SwLaunch *frame;
    SwLaunchChains *chains;     // NULL: not launched from a chain table
    int in_table;               // the kind an entry of this kind is coded as in a chain-table launch
    int family;                 // a chain table holds one family
    bool b_stream;              // a chain-table launch runs it on the B stream, beside the I / P kernels
};
static const SwKind k_sweep_kinds[SW_N_KINDS] = {
    {x264hip_launch_slice_plain, nullptr, SW_KIND_PLAIN, SW_LOSSY, false},                              // PLAIN: the wavefront schedule (k_slice_sweep<WPE>), lossless included
    {x264hip_launch_slice_rd, x264hip_launch_slice_rd_ch, SW_KIND_RD, SW_LOSSY, false},                 // RD: the raster variant, I / P
    {x264hip_launch_slice_rf, x264hip_launch_slice_rf_ch, SW_KIND_RF, SW_LOSSY, false},                 // RF: with the RD refinement of subme 8-9 (slice_refine.h)
    {x264hip_launch_slice_ll, x264hip_launch_slice_ll_ch, SW_KIND_LL, SW_LOSSLESS, false},              // LL: the lossless raster kernels (k_lossless_raster)
    {x264hip_launch_slice_ll_rf, x264hip_launch_slice_ll_rf_ch, SW_KIND_LL_RF, SW_LOSSLESS, false},
    {x264hip_launch_slice_b, nullptr, SW_KIND_BT, SW_LOSSY, true},                                      // B: one B kernel in the table launches, the extended one
    {x264hip_launch_slice_bt, x264hip_launch_slice_bt_ch, SW_KIND_BT, SW_LOSSY, true},                  // BT: temporal direct prediction, lookahead candidates
    {x264hip_launch_psy_rd, x264hip_launch_psy_rd_ch, SW_KIND_PSY_RD, SW_PSY, false},                   // PSY_*: RD, RF and BT with psy-trellis (k_psy_raster)
    {x264hip_launch_psy_rf, x264hip_launch_psy_rf_ch, SW_KIND_PSY_RF, SW_PSY, false},
    {x264hip_launch_psy_bt, x264hip_launch_psy_bt_ch, SW_KIND_PSY_BT, SW_PSY, true}};                   // one B kernel with psy-trellis, lock-step launches too
// which kind codes a sweep: has_rd: the raster variant (x264hip_slice_params.rd); mbrd: the RD level, 0..2; extended_b: a B slice with
// temporal direct prediction or the lookahead's candidates (the plain B kernel is 6-8 % faster, so the extended one only where it is needed)
static inline int sweep_kind(bool has_rd, bool is_b, bool lossless, int mbrd, bool psy_trellis, bool extended_b)
{
    if (!has_rd) return SW_KIND_PLAIN;
    if (is_b) return psy_trellis ? SW_KIND_PSY_BT : extended_b ? SW_KIND_BT : SW_KIND_B;
    if (lossless) return mbrd >= 2 ? SW_KIND_LL_RF : SW_KIND_LL;
    if (psy_trellis) return mbrd >= 2 ? SW_KIND_PSY_RF : SW_KIND_PSY_RD;
    return mbrd >= 2 ? SW_KIND_RF : SW_KIND_RD;
}
// a chain table is all-lossless or not at all, and all-psy-trellis or not at all: the first such family that holds some of the table's
// entries but not all of them, and in *n_family how many; SW_LOSSY (0) where the table is of one family
static inline int sweep_mixed_family(const int cnt[SW_N_KINDS], int *n_family)
{
    int n = 0, of[SW_N_FAMILIES] = {0};
    for (int k = 0; k < SW_N_KINDS; k++) { n += cnt[k]; of[k_sweep_kinds[k].family] += cnt[k]; }
    for (int f = SW_LOSSY + 1; f < SW_N_FAMILIES; f++)
        if (of[f] && of[f] != n) { *n_family = of[f]; return f; }
    return SW_LOSSY;
}
// whether the B kernel of a table runs on a stream of its own: beside an I / P kernel, or where the caller does not have the context's stream wait for it
static inline bool sweep_two_streams(const int cnt[SW_N_KINDS], bool join)
{
    int n_b = 0, n_other = 0;
    for (int k = 0; k < SW_N_KINDS; k++) (k_sweep_kinds[k].b_stream ? n_b : n_other) += cnt[k];
    return n_b && (n_other || !join);
}
// where each kind's entries begin in a table that holds cnt[k] entries of kind k
static inline void sweep_place(const int cnt[SW_N_KINDS], int base[SW_N_KINDS])
{
    for (int k = 0, b = 0; k < SW_N_KINDS; b += cnt[k++]) base[k] = b;
}
// one launch per kind present; the B kernel on b_stream (the context's own stream again unless sweep_two_streams)
static inline void sweep_enqueue(const SwDesc *tab, const int cnt[SW_N_KINDS], const int base[SW_N_KINDS], hipStream_t stream, hipStream_t b_stream)
{
    for (int k = 0; k < SW_N_KINDS; k++)
        if (cnt[k]) k_sweep_kinds[k].chains(tab + base[k], cnt[k], k_sweep_kinds[k].b_stream ? b_stream : stream);
}
