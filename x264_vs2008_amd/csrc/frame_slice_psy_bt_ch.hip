// frame_slice_psy_bt_ch.hip -- the chain-table launch of the extended B kernel with psy-trellis (slice_kernel.h: k_psy_raster): see
// frame_slice_psy_bt.hip and frame_slice_rd_ch.hip.
#include "slice_kernel.h"

void x264hip_launch_psy_bt_ch(const SwDesc *tab, int n, hipStream_t stream) { sw_launch_chains(k_psy_raster<true, true, false, true>, tab, n, stream); }
