// frame_lookahead_cost.hip -- FRAME LEVEL, part 6: the lookahead's per-frame cost, x264_slicetype_frame_cost's uncached branch with
// x264_slicetype_mb_cost inside it (R/encoder/slicetype.c:43-253, 256-345), one TASK = (frame b scored against p0 and p1) per wavefront.
//
// Why one wavefront per task: the macroblocks of a task form a chain -- they are visited in reverse raster order so that the vectors of
// the right and the three lower neighbours are the candidates of the next search -- and a GPU full of GOP chains has thousands of
// independent tasks at a time, so parallelism comes from the tasks.  Inside the macroblock the wave is used as the main encode's search
// uses it (me_exact.h: x264_me_search_ref + refine_subpel as "trips" of 4 / 8 candidates, one per lane group), on an 8x8 block of the
// half-resolution planes at subme 4 with min(HEX, me); the bidirectional tries put one pixel on each lane (get_ref's blend, the
// (weighted) average and the 8x8 SATD as four cross-lane butterfly stages).  The intra half of the cost is read from
// x264hip_lookahead_intra_frame's output (every block independent there).
//
// Neighbour vectors travel through LDS (two rows of the task), never through global memory written by this launch; the arrays
// lowres_mvs / lowres_mv_costs in HBM are outputs here and inputs of later tasks and of the main encode (x264_mb_predict_mv_ref16x16).
#include "look_cost_dev.h"

// The task loop is look_cost_body.h, textually included with SAD in scope: false here, the SATD lookahead (subme >= 2); true in
// frame_lookahead_cost_sad.hip, the lossless one -- h->pixf.mbcmp is SAD in x264_me_search's sub-pel refinement at the lookahead's
// subme 4 and in the bidirectional tries alike.  Included rather than shared as a __device__ function, and the SAD kernel in a
// translation unit of its own, so that k_look_cost's code object stays the one it was.
__global__ __launch_bounds__(64) void k_look_cost(const LookTaskDev *__restrict__ tasks, int mb_w, int mb_h, int stride, int method, int me_range,
                                                  int weighted_bipred, int bframe_bias, const i16 *__restrict__ cost_g, int *__restrict__ out)
{
    constexpr bool SAD = false;
#include "look_cost_body.h"
}
void x264hip_launch_look_cost_sad(const void *tasks_dev, int n_tasks, int mb_w, int mb_h, int stride, int method, int me_range, int weighted_bipred,
                                  int bframe_bias, const int16_t *cost_g, int *out, hipStream_t stream);

// Host side: resolve the tasks' slots to device pointers, stage them, launch.
extern "C" int x264hip_lookahead_cost_frames(x264hip_frame_ctx *c, const x264hip_look_slot *slots, int n_slots, const x264hip_look_task *tasks,
                                             int n_tasks, const x264hip_look_params *p, void *staging_host, void *tasks_dev, int32_t *out_dev)
{
    const int mb_w = c->d.mb_w, mb_h = c->d.mb_h, n = mb_w * mb_h;
    if (n_tasks <= 0) return 0;
    if (mb_w <= 2 || mb_h <= 2) { set_error("lookahead_cost_frames: frames of at most two macroblock rows / columns are scored edge and all (slicetype.c:292-297): not built"); return -1; }
    if (mb_w > LK_MAX_W) { set_error("lookahead_cost_frames: %d macroblocks per row, at most %d", mb_w, LK_MAX_W); return -1; }
    // mbcmp is SAD below subme 2 and when lossless (encoder.c:610).  The lossless flavour is built (k_look_cost_sad); lossy subme < 2 stays
    // refused, with the message tests/test_gpu_lookahead.py::test_refusals pins: its SAD lookahead would also need the search's own subme < 2 paths
    if (p->subme_param < 2 && !p->lossless) { set_error("lookahead_cost_frames: mbcmp is SAD (subme < 2 or lossless); only the SATD lookahead is built"); return -1; }
    if (p->bframes < 0 || p->bframes > 16 || !staging_host || !tasks_dev || !out_dev || !p->cost_mv) { set_error("lookahead_cost_frames: bad arguments"); return -1; }
    LookTaskDev *st = (LookTaskDev *)staging_host;
    const int nd = p->bframes + 1;
    for (int i = 0; i < n_tasks; i++) {
        const x264hip_look_task &t = tasks[i];
        if (t.slot_b < 0 || t.slot_b >= n_slots || t.slot_p0 < 0 || t.slot_p0 >= n_slots || t.slot_p1 < 0 || t.slot_p1 >= n_slots || t.chain < 0 || t.chain >= c->batch ||
            t.d0 < 0 || t.d0 > nd || t.d1 < 0 || t.d1 > nd) { set_error("lookahead_cost_frames: task %d out of range", i); return -1; }
        const x264hip_look_slot *sl[3] = {&slots[t.slot_b], &slots[t.slot_p0], &slots[t.slot_p1]};
        LookTaskDev &d = st[i];
        for (int f = 0; f < 3; f++)
            for (int k = 0; k < 4; k++) d.pl[f][k] = sl[f]->pic->lowres[k] + c->bs_l * t.chain;
        // [batch][2][bframes + 1][n]
        const size_t per_chain = (size_t)2 * nd * n;
        d.mv[0] = t.d0 ? sl[0]->mv + ((size_t)t.chain * per_chain + (size_t)(0 * nd + t.d0 - 1) * n) * 2 : nullptr;
        d.mv[1] = t.d1 ? sl[0]->mv + ((size_t)t.chain * per_chain + (size_t)(1 * nd + t.d1 - 1) * n) * 2 : nullptr;
        d.mcost[0] = t.d0 ? sl[0]->mv_cost + (size_t)t.chain * per_chain + (size_t)(0 * nd + t.d0 - 1) * n : nullptr;
        d.mcost[1] = t.d1 ? sl[0]->mv_cost + (size_t)t.chain * per_chain + (size_t)(1 * nd + t.d1 - 1) * n : nullptr;
        d.mvr = t.d1 ? sl[2]->mv + ((size_t)t.chain * per_chain + (size_t)(0 * nd + t.d0 + t.d1 - 1) * n) * 2 : nullptr;
        if (t.d1 && t.d0 + t.d1 > nd) { set_error("lookahead_cost_frames: task %d spans %d frames, more than bframes + 1", i, t.d0 + t.d1); return -1; }
        d.intra = sl[0]->intra_cost + (size_t)t.chain * n;
        d.d0 = t.d0; d.d1 = t.d1; d.do_search[0] = t.do_search[0]; d.do_search[1] = t.do_search[1];
    }
    // tasks_dev == staging_host: the kernel reads the records in place, from pinned host memory (168 bytes per task, once) -- for callers that
    // keep the device full, where even a small upload's copy kernel would wait for a wave slot
    if (tasks_dev != staging_host) HIPCHK(hipMemcpyAsync(tasks_dev, st, sizeof(LookTaskDev) * (size_t)n_tasks, hipMemcpyHostToDevice, c->stream));
    if (p->lossless)
        x264hip_launch_look_cost_sad(tasks_dev, n_tasks, mb_w, mb_h, slots[0].pic->stride_lowres, p->me_method < 1 ? p->me_method : 1, p->me_range,
                                     p->weighted_bipred, p->bframe_bias, p->cost_mv + p->cost_mv_range, out_dev, c->stream);
    else
        hipLaunchKernelGGL(k_look_cost, dim3(n_tasks), dim3(64), 0, c->stream, (const LookTaskDev *)tasks_dev, mb_w, mb_h, slots[0].pic->stride_lowres,
                           p->me_method < 1 ? p->me_method : 1, p->me_range, p->weighted_bipred, p->bframe_bias, p->cost_mv + p->cost_mv_range, out_dev);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" size_t x264hip_lookahead_task_bytes(void) { return sizeof(LookTaskDev); }
