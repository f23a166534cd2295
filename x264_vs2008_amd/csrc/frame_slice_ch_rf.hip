// frame_slice_ch_rf.hip -- the chain-table launch (slice_kernel.h, template argument CH) of the I / P kernel with the RD refinement of
// subme 8-9: see frame_slice_ch_rd.hip.
#include "slice_kernel.h"

void x264hip_launch_slice_rf_ch(const SwDesc *tab, int n, hipStream_t stream)
{
    if (sw_table_psy) { x264hip_launch_psy_rf_ch(tab, n, stream); return; }
    SwArgs a; SwRefs t; SwRd r;
    memset(&a, 0, sizeof(a)); memset(&t, 0, sizeof(t)); memset(&r, 0, sizeof(r));
    hipLaunchKernelGGL((k_slice_sweep<2, false, true, false, false, true, true>), dim3((unsigned)n), dim3(64), 0, stream, a, t, r, tab);
}
