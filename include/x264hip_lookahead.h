/* x264hip_lookahead.h -- the lookahead's device-side helpers that came after include/x264hip.h's "Lookahead and rate control" section
 * (x264hip_lookahead_* host state machine, x264hip_lookahead_cost_frames): storage of a lookahead slot and the per-chain indirections
 * the main encode needs once chains stop moving in lock step (adaptive B placement, CRF).  C ABI, plain pointers and sizes. */
#ifndef X264HIP_LOOKAHEAD_H
#define X264HIP_LOOKAHEAD_H
#include "x264hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* A lookahead slot's picture: Y, U, V and the four half-resolution planes, no half-pel planes (an input frame waiting in frames.next:
 * x264_frame_new with b_have_lowres, R/common/frame.c:80-96).  Freed with x264hip_picture_free. */
int x264hip_picture_alloc_lookahead(x264hip_frame_ctx *c, x264hip_picture *pic);


/* The macroblock sweep for chains that no longer move in lock step.  x264hip_slice_sweep_frame codes the same kind of frame in every
 * batch element; once x264_slicetype_decide places B frames per chain and the rate control prices every frame on its own, chain A
 * codes a P frame from references {9, 8} at QP 24 while chain B codes a B frame between 8 and 12 at QP 27.  Here every entry is ONE
 * chain's sweep, described exactly like a call of x264hip_slice_sweep_frame -- its own source picture, references, reconstruction,
 * states and slice parameters (QP, POCs, lowres vectors, list 1) -- and the chain (batch element) it applies to: the pictures and states
 * are the batch-wide ones, the entry touches element `chain` of each.  One launch per kernel kind (I / P, I / P with the subme 8-9
 * refinement, B), each block taking its arguments from its entry (csrc/slice_kernel.h, template argument CH).  The raster variant only
 * (params->rd): with the CABAC coder in the loop (write = 1) in every entry, or in none -- an all-CAVLC table (cabac = 0, write = 0, states
 * with level arrays), whose slices x264hip_cavlc_write_chains writes afterwards; a table that mixes the two is refused.  Every entry's `out` state gets the frame-level scalars later frames
 * read (poc, ref_poc ...): give each chain its own COPY of the x264hip_mb_state structure (same device arrays, its own scalars).  The
 * abort flag of every distinct state written must be cleared before the call (x264hip_mb_state_clear_progress).  staging_host (pinned)
 * and table_dev: n * x264hip_chain_sweep_bytes() each, left alone until the stream has passed the call. */
typedef struct {
    int chain;
    const x264hip_picture *fenc;
    const x264hip_picture *const *refs;
    int n_refs;
    x264hip_picture *recon;
    const x264hip_slice_params *params;
    const x264hip_mb_state *l0;
    x264hip_mb_state *out;
} x264hip_chain_sweep;
int x264hip_slice_sweep_chains(x264hip_frame_ctx *c, x264hip_chain_sweep *entries, int n, void *staging_host, void *table_dev);
size_t x264hip_chain_sweep_bytes(void);
int x264hip_mb_state_clear_progress(x264hip_frame_ctx *c, x264hip_mb_state *st);
/* x264hip_slice_sweep_chains with the completion of its two kernel kinds visible to the caller: ev_ip (x264hip_event_create) is recorded
 * behind the I / P kernels on the context's stream, ev_b behind the B kernel on the library's second stream of this context, and the
 * context's stream does not wait for the B kernel.  A scheduler polls the events (x264hip_event_query) and hands each chain its next
 * frame as soon as its own kernel is done instead of when the step's slowest chain is (x264_vs2008_amd/stream.py: AsyncStreamEncoder). */
int x264hip_slice_sweep_chains_events(x264hip_frame_ctx *c, x264hip_chain_sweep *entries, int n, void *staging_host, void *table_dev, void *ev_ip, void *ev_b);
int x264hip_event_query(void *ev);       /* 1 finished, 0 not yet, < 0 error */
/* a stream of the device's greatest priority (x264hip_stream_destroy frees it): its kernels' wavefronts are dispatched first when a slot
 * frees -- the lookahead's short kernels beside sweeps that keep the device full */
void *x264hip_stream_create_high_priority(void);
/* a stream whose kernels run on compute units [first, first + n) of 256 only; x264hip_frame_ctx_set_b_stream: the stream the B kernel of
 * this context's chain-table launches runs on (default, and again after NULL: one the library creates and x264hip_frame_ctx_delete destroys)
 * -- a caller may give the step's I / P chains and its B chains disjoint parts of the device (x264hip_frame_ctx_new takes the context's own
 * stream).  The stream stays the caller's: the context never destroys it, the caller does once the context is deleted or has been given another. */
void *x264hip_stream_create_cu_range(int first_cu, int n_cus);
int x264hip_frame_ctx_set_b_stream(x264hip_frame_ctx *c, void *hip_stream);
/* The batch elements the end-of-frame calls of this context touch from now on -- x264hip_deblock_frame, x264hip_expand_border,
 * x264hip_hpel_filter_frame: a device list of n element indices, or NULL = all.  With chains out of lock step a pool picture holds,
 * per element, either the frame that chain has just coded into it (to be filtered and kept as a reference) or an older reference of
 * another chain that must stay as it is. */
int x264hip_frame_ctx_elements(x264hip_frame_ctx *c, const int *elems_dev, int n);


/* The CAVLC writer: x264_macroblock_write_cavlc + x264_slice_write's skip runs (R/encoder/cavlc.c:60-620, R/encoder/encoder.c:1200-1280) for
 * every chain's I, P or B slice, as a pass over the state x264hip_slice_sweep_frame left (a `--no-cabac` slice below the RD levels: the wavefront
 * variant at constant QP, or the raster variant without its writer -- rd.write = 0 -- when adaptive quantisation gives every macroblock its QP
 * or the slice is a B slice; decisions and coefficient levels in the x264hip_mb_state -- allocate it WITH level arrays; a B slice also reads
 * the state's list-1 arrays ref1 / mv1).  payload: device
 * [batch][payload_cap] bytes, chain b's slice_data() starts X264HIP_PAYLOAD_LEAD (64) bytes into its slot, from bit 0, rbsp trailing bits
 * included; payload_len: device [batch] int32; mb_bits (optional): device [batch][n_mb], bit position after every macroblock.
 * Asynchronous on the context's stream.  I_PCM macroblocks and a slot too small end with x264hip_slice_sweep_status reporting an abort:
 * every slice, of x264hip_cavlc_write_frame (payload_cap >= 4096) and of x264hip_cavlc_write_chains alike, stops before a macroblock whose
 * worst case (2624 bytes, derived and measured in csrc/frame_cavlc.hip) might not fit. */
typedef struct {
    int slice_type;            /* 0 P, 1 B, 2 I */
    int n_ref0;                /* h->mb.pic.i_fref[0]: references of list 0 (the number te() is written against) */
    int analyse_inter;         /* param.analyse.inter (X264_ANALYSE_PSUB8x8 decides how sub-partition types are written) */
    int transform8x8;          /* pps->b_transform_8x8_mode */
    int cqm_custom;            /* param.i_cqm_preset != FLAT (High profile: level escapes beyond prefix 15) */
    uint8_t *payload; int payload_cap; int32_t *payload_len; int32_t *mb_bits;
    int slice_qp;              /* h->sh.i_qp: what mb_qp_delta of the first coded macroblock is relative to (per-macroblock QPs: the state's qp array) */
} x264hip_cavlc_params;
int x264hip_cavlc_write_frame(x264hip_frame_ctx *c, const x264hip_mb_state *st, const x264hip_cavlc_params *p);

/* The CABAC writer as a pass: x264_macroblock_write_cabac with x264_slice_write's terminal bins and skip flags (R/encoder/cabac.c:32-1022,
 * R/encoder/encoder.c:1192-1273) for every chain's I or P slice, from the state x264hip_slice_sweep_frame left.  Below the RD levels the
 * analysis never reads the CABAC contexts, so a CABAC slice there needs no writer in the macroblock loop: the wavefront variant codes it at
 * constant QP, the raster variant without its writer (cabac = 1, rd.write = 0) under adaptive quantisation, and this call writes the bytes
 * the in-loop writer would have.  The state is allocated WITH level arrays.  payload, payload_len, mb_bits: as x264hip_slice_rd's -- device
 * [batch][payload_cap] bytes with chain b's slice_data() X264HIP_PAYLOAD_LEAD bytes into its slot, [batch] lengths, and (optional)
 * [batch][n_mb] bit positions after every macroblock.  cabac_init_idc, i_frame, i_frame_stride: as x264hip_slice_rd's (chain b's flush takes
 * i_frame + b * i_frame_stride).  Asynchronous on the context's stream.  The pass stops before a macroblock whose worst case (8192 bytes,
 * the in-loop writer's bound) might not fit the slot, and at an I_PCM macroblock (none occurs below the RD levels): x264hip_slice_sweep_status
 * then reports an abort, and nothing is written past the slot.  B slices, states without level arrays, frames of more than 512 macroblocks
 * per row and payload slots below 8192 + 128 bytes are refused. */
typedef struct {
    int slice_type;            /* 0 P, 2 I */
    int n_ref0;                /* h->mb.pic.i_fref[0] */
    int analyse_inter;         /* param.analyse.inter (kept beside x264hip_cavlc_params; CABAC always codes the sub-partition types) */
    int transform8x8;          /* pps->b_transform_8x8_mode */
    int slice_qp;              /* h->sh.i_qp: the contexts' initial states and the first mb_qp_delta's base */
    int cabac_init_idc;
    int i_frame, i_frame_stride;
    uint8_t *payload; int payload_cap; int32_t *payload_len; int32_t *mb_bits;
} x264hip_cabac_params;
int x264hip_cabac_write_frame(x264hip_frame_ctx *c, const x264hip_mb_state *st, const x264hip_cabac_params *p);

/* The writer for chains that do not move in lock step: the counterpart of x264hip_slice_sweep_chains for an all-CAVLC chain table (every
 * entry of the sweep's table with cabac = 0 and rd.write = 0).  Every entry is ONE chain's slice: the chain (batch element), the state its
 * sweep wrote (that chain's copy of the x264hip_mb_state) and the slice's x264hip_cavlc_params -- slice type, n_ref0, slice QP and the
 * batch-wide payload / payload_len / mb_bits buffers, of which the entry writes element `chain` (its payload slot).  One launch writes all
 * entries, I, P and B slices side by side, one wavefront each; asynchronous on the context's stream, so behind a sweep enqueued before it.
 * staging_host (pinned) and table_dev: n * x264hip_chain_cavlc_bytes() each, left alone until the stream has passed the call.
 * payload_cap is at least X264HIP_PAYLOAD_LEAD + 2624. */
typedef struct {
    int chain;
    const x264hip_mb_state *state;
    const x264hip_cavlc_params *params;
} x264hip_chain_cavlc;
int x264hip_cavlc_write_chains(x264hip_frame_ctx *c, const x264hip_chain_cavlc *entries, int n, void *staging_host, void *table_dev);
size_t x264hip_chain_cavlc_bytes(void);

/* The same two calls with every lane writing: the macroblock-parallel CAVLC pass.  x264hip_cavlc_write_frame and _chains put one lane of one
 * wavefront on a slice; CAVLC has no adaptive state, so a macroblock's bits depend on the state arrays alone and only their position in the
 * slice is serial -- a prefix sum.  Three phases on the context's stream: count (one lane per macroblock: bit lengths, after a short kernel
 * that leaves every block's coefficient total for nC), scan (per slice: offsets, skip runs, mb_bits, payload_len, the aborts, and the zeroing
 * of the bytes about to be written), place (one lane per macroblock: its bits at its offset, words shared with a neighbour merged with
 * atomic OR).  Same parameter records, same bytes, payload_len, mb_bits, refusals and messages as the serial calls, the same aborts (I_PCM, a
 * slot too small by the same rule; payload_len 0 and nothing placed), and no limit on the macroblocks per row.  Nothing the caller has zeroed
 * is relied on; no byte outside the chain's slot is touched and the slot's X264HIP_PAYLOAD_LEAD bytes keep their values.  (Place merges a
 * macroblock's first and last 32-bit word with a 4-byte-aligned atomic OR.  The last word ends inside the slot: at least 20 bytes stay free
 * behind a slice that passed the space check.  Where a slot's start is no multiple of 4 -- a payload_cap that is none -- the first word of
 * the slice takes in up to 3 of the slot's own lead bytes: zeros are ORed into them, so they are read and written back unchanged, and must
 * not be written by anyone else while the pass runs.)  scratch_dev:
 * x264hip_cavlc_mp_scratch_bytes(c, n_slices) device bytes -- n_slices: the context's batch for _frame_mp, the table's entries for
 * _chains_mp --, left alone until the stream has passed the call.  At most 65535 slices per call.  Opt-in: nothing selects this pass by itself. */
int x264hip_cavlc_write_frame_mp(x264hip_frame_ctx *c, const x264hip_mb_state *st, const x264hip_cavlc_params *p, void *scratch_dev);
int x264hip_cavlc_write_chains_mp(x264hip_frame_ctx *c, const x264hip_chain_cavlc *entries, int n, void *staging_host, void *table_dev, void *scratch_dev);
size_t x264hip_cavlc_mp_scratch_bytes(const x264hip_frame_ctx *c, int n_slices);

#ifdef __cplusplus
}
#endif
#endif
