// frame_cabac.hip -- FRAME LEVEL, part 8: the CABAC writer as a pass (x264_macroblock_write_cabac with the terminal bins and skip flags of
// x264_slice_write, R/encoder/cabac.c:32-1022, R/encoder/encoder.c:1192-1273) for I and P slices, over the state a sweep left.
//
// Below the RD levels (subme < 6, no trellis) the analysis never reads the CABAC contexts, so nothing in a macroblock's decisions needs
// the writer beside it: the wavefront variant of the sweep codes such a slice at constant QP, the raster variant without its writer under
// adaptive quantisation, and this pass writes the bytes the in-loop writer of slice_sweep_body.h would have -- the same calls of
// cabac_dev.h, on a syntax record rebuilt from the state (cabac_pass_dev.h, text that also compiles for the host).
// Mapping: one wavefront per chain; the chains are the parallelism.  A slice's bit string is serial, so lane 0 drives the arithmetic coder;
// around it all 64 lanes build the record it walks: they issue the loads of the NEXT macroblock's share of the state (64-wide gathers of the
// levels and counts, one entry of the neighbour caches per lane) into registers before lane 0 codes the current one, so the loads are in
// flight meanwhile, and turn them into the record in LDS afterwards, the mvd of its 16 blocks on 16 lanes.  The 460 context states, the
// record, the row of mvd above and cabac_dev.h's cd_lds_* tables live in LDS; the bytes leave through lane 0's vector stores.  What the pass
// costs next to the sweep it follows is measured in DESIGN.md section 6.  Payload layout as the in-loop writer's: X264HIP_PAYLOAD_LEAD bytes of each chain's slot, then
// slice_data() from bit 0 to the flush; mb_bits: the position after every macroblock.
#include "device_prims.h"
#include "frame_internal.h"
#include "cabac_pass_dev.h"
#include "slice_kernel.h"            // SW_MB_BYTES_MAX alone: the bound the in-loop writer stops at

using namespace x264hip;

static_assert(CP_MB_BYTES_MAX == SW_MB_BYTES_MAX, "the pass and the in-loop writer stop before the same worst case of a macroblock");

// every chain's slice of one frame: the same arguments, the chain is the block
__global__ __launch_bounds__(64) void k_cabac_write(CpArgs a)
{
    __shared__ CpWork w;
    cd_load_tables((int)threadIdx.x);
    CP_SYNC();
    cp_write_slice(a, (int)blockIdx.x, (CpWorkP)&w);
}

extern "C" int x264hip_cabac_write_frame(x264hip_frame_ctx *c, const x264hip_mb_state *st, const x264hip_cabac_params *p)
{
    if (!c || !st || !p) { set_error("cabac_write_frame: context / state / parameters missing"); return -1; }
    if (p->slice_type == 1) { set_error("cabac_write_frame: B slices are not built as a pass (they keep the in-loop writer)"); return -1; }
    if (p->slice_type != 0 && p->slice_type != 2) { set_error("cabac_write_frame: slice type %d (0 P, 2 I)", p->slice_type); return -1; }
    if (!st->luma || !st->luma_dc || !st->chroma_dc || !st->chroma_ac) { set_error("cabac_write_frame: needs a state with coefficient levels (allocated without X264HIP_STATE_NO_LEVELS)"); return -1; }
    if (c->d.mb_w > CP_MAX_W) { set_error("cabac_write_frame: %d macroblocks per row, at most %d", c->d.mb_w, CP_MAX_W); return -1; }
    if (!p->payload || !p->payload_len || p->payload_cap < CP_MB_BYTES_MAX + 128) {
        set_error("cabac_write_frame: payload buffers missing or smaller than one macroblock's worst case (%d bytes)", CP_MB_BYTES_MAX + 128);
        return -1;
    }
    if (p->slice_qp < 0 || p->slice_qp > 51 || p->cabac_init_idc < 0 || p->cabac_init_idc > 2) { set_error("cabac_write_frame: slice_qp %d / cabac_init_idc %d", p->slice_qp, p->cabac_init_idc); return -1; }
    CpArgs a;
    cp_args(a, st, p, c->d.mb_w, c->d.mb_h, st->progress + (size_t)c->d.mb_h * c->batch, c->abort_total);
    hipLaunchKernelGGL(k_cabac_write, dim3((unsigned)c->batch), dim3(64), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}
