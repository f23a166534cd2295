// frame_slice_b.hip -- the B-slice instantiation of the raster sweep (slice_kernel.h with slice_b_flow.h): one wavefront per chain,
// list 0 and list 1, direct prediction, bi-prediction, the CABAC B syntax.  A separate kernel so that the I / P one keeps its
// registers and LDS.  Lock-step launches only: a chain table codes its B entries with the extended kernel (frame_slice_bt_ch.hip).
#include "slice_kernel.h"

void x264hip_launch_slice_b(const SwArgs &a, const SwRefs &t, const SwRd &r, hipStream_t stream) { sw_launch_frame(k_slice_sweep<2, false, true, true>, a, t, r, stream); }
