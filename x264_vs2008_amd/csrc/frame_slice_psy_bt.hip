// frame_slice_psy_bt.hip -- the extended B kernel with psy-trellis (slice_kernel.h: k_psy_raster): a kernel of its own name, in a
// translation unit of its own so that the psy-trellis kernels compile side by side.  The one B kernel with psy-trellis: every B sweep
// with it is of kind PSY_BT (sweep_tables.h: sweep_kind).
#include "slice_kernel.h"

void x264hip_launch_psy_bt(const SwArgs &a, const SwRefs &t, const SwRd &r, hipStream_t stream) { sw_launch_frame(k_psy_raster<true, true, false, false>, a, t, r, stream); }
