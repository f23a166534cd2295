// frame_slice_psy_bt.hip -- the extended B kernel (both kinds of lock-step B launch go here) with psy-trellis (slice_kernel.h: k_psy_raster): a kernel of its own name, in a
// translation unit of its own so that the psy-trellis kernels compile side by side; launched by x264hip_launch_slice_b / _bt when SwRd::psy_trellis is set.
#include "slice_kernel.h"

void x264hip_launch_psy_bt(const SwArgs &a, const SwRefs &t, const SwRd &r, hipStream_t stream)
{
    hipLaunchKernelGGL((k_psy_raster<true, true, false, false>), dim3((unsigned)a.batch), dim3(64), 0, stream, a, t, r, nullptr);
}
