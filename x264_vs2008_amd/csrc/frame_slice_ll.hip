// frame_slice_ll.hip -- the raster-order sweep with lossless on (constant QP 0, h->mb.b_lossless): I and P slices, subme 0..7, the CABAC
// writer in the loop.  k_lossless_raster (slice_kernel.h) is a kernel of its own name over the same sweep as k_slice_sweep, so the lossy
// raster kernels stay the instantiations they were.
#include "slice_kernel.h"

void x264hip_launch_slice_ll(const SwArgs &a, const SwRefs &t, const SwRd &r, hipStream_t stream) { sw_launch_frame(k_lossless_raster<false, false>, a, t, r, stream); }
