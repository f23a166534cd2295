// frame_slice_psy_rd_ch.hip -- the chain-table launch of the raster sweep's I / P kernel with psy-trellis (slice_kernel.h: k_psy_raster):
// see frame_slice_psy_rd.hip and frame_slice_rd_ch.hip.
#include "slice_kernel.h"

void x264hip_launch_psy_rd_ch(const SwDesc *tab, int n, hipStream_t stream) { sw_launch_chains(k_psy_raster<false, false, false, true>, tab, n, stream); }
