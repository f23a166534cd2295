// frame_slice_ll_rf.hip -- the lossless raster sweep with the RD refinement of subme 8-9 (slice_refine.h): see frame_slice_ll.hip.  One
// wave per SIMD: the refinement's state on top of the analysis records lives in registers, not in scratch memory.
#include "slice_kernel.h"

void x264hip_launch_slice_ll_rf(const SwArgs &a, const SwRefs &t, const SwRd &r, hipStream_t stream) { sw_launch_frame(k_lossless_raster<true, false>, a, t, r, stream); }
