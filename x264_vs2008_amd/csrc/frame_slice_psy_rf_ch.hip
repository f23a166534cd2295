// frame_slice_psy_rf_ch.hip -- the chain-table launch of the I / P kernel with the RD refinement of subme 8-9 with psy-trellis
// (slice_kernel.h: k_psy_raster): see frame_slice_psy_rf.hip and frame_slice_rd_ch.hip.
#include "slice_kernel.h"

void x264hip_launch_psy_rf_ch(const SwDesc *tab, int n, hipStream_t stream) { sw_launch_chains(k_psy_raster<false, false, true, true>, tab, n, stream); }
