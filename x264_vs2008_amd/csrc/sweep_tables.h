// sweep_tables.h -- the two tables the host side of the sweep walks (frame_slice.hip): the device arrays of an x264hip_mb_state, and
// the kernel variants ("kinds") of the sweep.  Plain C++ over names its includer provides -- x264hip_mb_state (x264hip.h); SwArgs, SwRefs,
// SwRd, SwDesc, SW_MAX_REFS and hipStream_t (slice_kernel.h, which includes this file at its end) -- so that tests/sweep_tables_host.cpp
// compiles the same tables and walks for the host alone, with stand-ins for the launch functions.
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
// evenly over the SIMDs before the B kernel's fill the rest -- and the table's entries are sorted in the same order: [RD | RF | BT], or
// [LL | LL_RF] when the launch is lossless (a table is all-lossless or not at all).
enum { SW_KIND_PLAIN = 0, SW_KIND_RD, SW_KIND_RF, SW_KIND_LL, SW_KIND_LL_RF, SW_KIND_B, SW_KIND_BT, SW_N_KINDS };
typedef void SwLaunch(const SwArgs &a, const SwRefs &t, const SwRd &r, hipStream_t stream);     // a lock-step launch (frame_slice_<kind>.hip)
typedef void SwLaunchChains(const SwDesc *tab, int n, hipStream_t stream);                       // a chain-table launch (frame_slice_*ch*.hip)
SwLaunch x264hip_launch_slice_rd, x264hip_launch_slice_rf, x264hip_launch_slice_ll, x264hip_launch_slice_ll_rf, x264hip_launch_slice_b, x264hip_launch_slice_bt;
SwLaunchChains x264hip_launch_slice_rd_ch, x264hip_launch_slice_rf_ch, x264hip_launch_slice_ll_ch, x264hip_launch_slice_ll_rf_ch, x264hip_launch_slice_bt_ch;
struct SwKind {
    SwLaunch *frame;            // NULL: x264hip_slice_sweep_frame launches it itself
    SwLaunchChains *chains;     // NULL: not launched from a chain table
    int in_table;               // the kind an entry of this kind is coded as in a chain-table launch
};
static const SwKind k_sweep_kinds[SW_N_KINDS] = {
    {nullptr, nullptr, SW_KIND_PLAIN},                                                  // PLAIN: the wavefront schedule (k_slice_sweep<WPE>)
    {x264hip_launch_slice_rd, x264hip_launch_slice_rd_ch, SW_KIND_RD},                  // RD: the raster variant, I / P
    {x264hip_launch_slice_rf, x264hip_launch_slice_rf_ch, SW_KIND_RF},                  // RF: with the RD refinement of subme 8-9 (slice_refine.h)
    {x264hip_launch_slice_ll, x264hip_launch_slice_ll_ch, SW_KIND_LL},                  // LL: the lossless raster kernels (k_lossless_raster)
    {x264hip_launch_slice_ll_rf, x264hip_launch_slice_ll_rf_ch, SW_KIND_LL_RF},
    {x264hip_launch_slice_b, nullptr, SW_KIND_BT},                                      // B: one B kernel in the table launches, the extended one
    {x264hip_launch_slice_bt, x264hip_launch_slice_bt_ch, SW_KIND_BT}};                 // BT: temporal direct prediction, lookahead candidates
// where each kind's entries begin in a table that holds cnt[k] entries of kind k
static inline void sweep_place(const int cnt[SW_N_KINDS], int base[SW_N_KINDS])
{
    for (int k = 0, b = 0; k < SW_N_KINDS; b += cnt[k++]) base[k] = b;
}
// one launch per kind present; the B kernel on b_stream (the context's own stream again unless it runs beside an I / P kernel)
static inline void sweep_enqueue(const SwDesc *tab, const int cnt[SW_N_KINDS], const int base[SW_N_KINDS], hipStream_t stream, hipStream_t b_stream)
{
    for (int k = 0; k < SW_N_KINDS; k++)
        if (cnt[k]) k_sweep_kinds[k].chains(tab + base[k], cnt[k], k == SW_KIND_BT ? b_stream : stream);
}
