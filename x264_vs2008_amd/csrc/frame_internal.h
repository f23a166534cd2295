// frame_internal.h -- state of the frame level (planes resident in HBM)
#pragma once
#include "internal.h"

#define PADH 32   // R/common/frame.h:27-29
#define PADV 32

// A context describes `batch` independent frames of one size (one per GOP
// chain) that every frame-level call processes in the same launches
// (blockIdx.z = batch element).  Each plane of a picture is `batch`
// consecutive padded images `bs_*` bytes apart; per-macroblock arrays are
// `batch` consecutive [n_mb][...] blocks.
// A context belongs to one thread at a time: `sel`, `elems` and the B stream with its events are unguarded.  What it owns --
// ssd_dev, its stream if own_stream, the B stream if own_b_stream, the two events -- is released by x264hip_frame_ctx_delete and
// nowhere else; a stream the caller handed in (x264hip_frame_ctx_new, x264hip_frame_ctx_set_b_stream) stays the caller's.
struct x264hip_frame_ctx {
    x264hip_frame_dims d;
    hipStream_t stream;
    bool own_stream;
    // A chain-table launch runs its B kernel beside its I / P kernels, on b_stream, between the events b_ready and b_done.  All
    // three are made by the first launch that needs them (or by x264hip_frame_ctx_set_b_stream): most contexts never do.
    hipStream_t b_stream;
    bool own_b_stream;
    hipEvent_t b_ready, b_done;
    int width16, lines16;          // coded luma size
    int batch, sel;                // batch size; element addressed by upload / download
    size_t bs_y, bs_c, bs_l;       // bytes between batch elements: luma-sized, chroma-sized, lowres planes
    int stride_l, width_l, lines_l;
    unsigned long long *ssd_dev;   // [batch][3] accumulators for x264hip_ssd_frame
    int *abort_total;              // the sticky sweep-abort counter (x264hip_slice_sweep_status), in ssd_dev's allocation
    // x264hip_frame_ctx_elements: the batch elements the end-of-frame calls (deblock, border expansion, half-pel filter) touch;
    // NULL = all.  Chains that code different kinds of frames keep some of a picture's elements as they are (device list).
    const int *elems; int n_elems;
};

static inline int align_up(int v, int a) { return (v + a - 1) / a * a; }
static inline size_t align_up_sz(size_t v, size_t a) { return (v + a - 1) / a * a; }
