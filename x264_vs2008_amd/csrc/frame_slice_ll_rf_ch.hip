// frame_slice_ll_rf_ch.hip -- the chain-table launch of the lossless raster sweep with the RD refinement of subme 8-9: see
// frame_slice_ll_rf.hip and frame_slice_rd_ch.hip.
#include "slice_kernel.h"

void x264hip_launch_slice_ll_rf_ch(const SwDesc *tab, int n, hipStream_t stream) { sw_launch_chains(k_lossless_raster<true, true>, tab, n, stream); }
