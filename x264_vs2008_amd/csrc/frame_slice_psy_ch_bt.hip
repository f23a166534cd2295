// frame_slice_psy_ch_bt.hip -- the chain-table launch of the extended B kernel with psy-trellis (slice_kernel.h: k_psy_raster): see
// frame_slice_psy_bt.hip and frame_slice_ch_rd.hip; launched by x264hip_launch_slice_b_ch when the table is a psy-trellis one (sw_table_psy).
#include "slice_kernel.h"

void x264hip_launch_psy_bt_ch(const SwDesc *tab, int n, hipStream_t stream)
{
    SwArgs a; SwRefs t; SwRd r;
    memset(&a, 0, sizeof(a)); memset(&t, 0, sizeof(t)); memset(&r, 0, sizeof(r));
    hipLaunchKernelGGL((k_psy_raster<true, true, false, true>), dim3((unsigned)n), dim3(64), 0, stream, a, t, r, tab);
}
