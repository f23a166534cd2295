// frame_slice_ll_ch.hip -- the chain-table launch (slice_kernel.h, template argument CH) of the lossless raster sweep: see
// frame_slice_ll.hip and frame_slice_rd_ch.hip.
#include "slice_kernel.h"

void x264hip_launch_slice_ll_ch(const SwDesc *tab, int n, hipStream_t stream) { sw_launch_chains(k_lossless_raster<false, true>, tab, n, stream); }
