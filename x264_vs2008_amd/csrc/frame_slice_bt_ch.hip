// frame_slice_bt_ch.hip -- the chain-table launch (slice_kernel.h, template argument CH) of the extended B kernel (temporal direct
// prediction, the lookahead's candidates): see frame_slice_bt.hip and frame_slice_rd_ch.hip.
#include "slice_kernel.h"

void x264hip_launch_slice_bt_ch(const SwDesc *tab, int n, hipStream_t stream) { sw_launch_chains(k_slice_sweep<2, false, true, true, true, false, true>, tab, n, stream); }
