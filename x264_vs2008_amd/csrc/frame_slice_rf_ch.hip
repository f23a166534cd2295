// frame_slice_rf_ch.hip -- the chain-table launch (slice_kernel.h, template argument CH) of the I / P kernel with the RD refinement of
// subme 8-9: see frame_slice_rf.hip and frame_slice_rd_ch.hip.
#include "slice_kernel.h"

void x264hip_launch_slice_rf_ch(const SwDesc *tab, int n, hipStream_t stream) { sw_launch_chains(k_slice_sweep<2, false, true, false, false, true, true>, tab, n, stream); }
