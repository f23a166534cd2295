// frame_slice_psy_rd.hip -- the raster sweep's I / P kernel with psy-trellis (slice_kernel.h: k_psy_raster): a kernel of its own name, in a
// translation unit of its own so that the psy-trellis kernels compile side by side; launched by x264hip_launch_slice_rd when SwRd::psy_trellis is set.
#include "slice_kernel.h"

void x264hip_launch_psy_rd(const SwArgs &a, const SwRefs &t, const SwRd &r, hipStream_t stream)
{
    hipLaunchKernelGGL((k_psy_raster<false, false, false, false>), dim3((unsigned)a.batch), dim3(64), 0, stream, a, t, r, nullptr);
}
