// frame_slice_psy_rf.hip -- the I / P kernel with the RD refinement of subme 8-9 with psy-trellis (slice_kernel.h: k_psy_raster): a kernel
// of its own name, in a translation unit of its own so that the psy-trellis kernels compile side by side; kind PSY_RF (sweep_tables.h).
#include "slice_kernel.h"

void x264hip_launch_psy_rf(const SwArgs &a, const SwRefs &t, const SwRd &r, hipStream_t stream) { sw_launch_frame(k_psy_raster<false, false, true, false>, a, t, r, stream); }
