// frame_lookahead_cost_sad.hip -- the lookahead's cost kernel with SAD as mbcmp: lossless (x264hip_look_params.lossless).  The same task loop
// as k_look_cost (look_cost_body.h), in a translation unit of its own: see frame_lookahead_cost.hip.
#include "look_cost_dev.h"

__global__ __launch_bounds__(64) void k_look_cost_sad(const LookTaskDev *__restrict__ tasks, int mb_w, int mb_h, int stride, int method, int me_range,
                                                      int weighted_bipred, int bframe_bias, const i16 *__restrict__ cost_g, int *__restrict__ out)
{
    constexpr bool SAD = true;
#include "look_cost_body.h"
}

void x264hip_launch_look_cost_sad(const void *tasks_dev, int n_tasks, int mb_w, int mb_h, int stride, int method, int me_range, int weighted_bipred,
                                  int bframe_bias, const int16_t *cost_g, int *out, hipStream_t stream)
{
    hipLaunchKernelGGL(k_look_cost_sad, dim3(n_tasks), dim3(64), 0, stream, (const LookTaskDev *)tasks_dev, mb_w, mb_h, stride, method, me_range,
                       weighted_bipred, bframe_bias, cost_g, out);
}
