// frame_slice_psy_ch_rd.hip -- the chain-table launch of the raster sweep's I / P kernel with psy-trellis (slice_kernel.h: k_psy_raster): see
// frame_slice_psy_rd.hip and frame_slice_ch_rd.hip; launched by x264hip_launch_slice_rd_ch when the table is a psy-trellis one (sw_table_psy).
#include "slice_kernel.h"

void x264hip_launch_psy_rd_ch(const SwDesc *tab, int n, hipStream_t stream)
{
    SwArgs a; SwRefs t; SwRd r;
    memset(&a, 0, sizeof(a)); memset(&t, 0, sizeof(t)); memset(&r, 0, sizeof(r));
    hipLaunchKernelGGL((k_psy_raster<false, false, false, true>), dim3((unsigned)n), dim3(64), 0, stream, a, t, r, tab);
}
