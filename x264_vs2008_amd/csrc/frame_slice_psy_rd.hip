// frame_slice_psy_rd.hip -- the raster sweep's I / P kernel with psy-trellis (slice_kernel.h: k_psy_raster): a kernel of its own name, in a
// translation unit of its own so that the psy-trellis kernels compile side by side; kind PSY_RD (sweep_tables.h).
#include "slice_kernel.h"

void x264hip_launch_psy_rd(const SwArgs &a, const SwRefs &t, const SwRd &r, hipStream_t stream) { sw_launch_frame(k_psy_raster<false, false, false, false>, a, t, r, stream); }
