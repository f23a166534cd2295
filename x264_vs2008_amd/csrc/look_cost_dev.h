// look_cost_dev.h -- what the lookahead's two cost kernels share (frame_lookahead_cost.hip: k_look_cost, SATD; frame_lookahead_cost_sad.hip:
// k_look_cost_sad, lossless): the task record, get_ref's sample, the block metrics.  The task loop itself is look_cost_body.h.
#pragma once
#include "device_prims.h"
#include "frame_internal.h"
#include "me_exact.h"

using namespace x264hip;

#define LK_MAX_W 512                    // macroblocks per row the LDS rows hold (8192 luma samples)
#define LK_COST_MAX (1 << 28)

struct LookTaskDev {
    const u8 *pl[3][4];                 // lowres luma + H, V, HV of frame b, p0, p1 at this chain's picture origin
    i16 *mv[2];                         // frames[b]->lowres_mvs[l][dist - 1] of this chain, [n][2]
    int *mcost[2];                      // frames[b]->lowres_mv_costs[l][dist - 1], [n]
    const i16 *mvr;                     // frames[p1]->lowres_mvs[0][p1 - p0 - 1] (b < p1)
    const int *intra;                   // frames[b]->i_intra_cost, [n]
    int d0, d1;                         // b - p0, p1 - b
    int do_search[2];
};

#define LK_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_s_waitcnt(0); __builtin_amdgcn_wave_barrier(); \
                       __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); } while (0)

// hpel_ref0 / hpel_ref1 of get_ref (R/common/mc.c:176-177), two bits per quarter-pel phase
#define LK_HREF0 0x54FE5454u            // {0,1,1,1,0,1,1,1,2,3,3,3,0,1,1,1}
#define LK_HREF1 0xBABABA00u            // {0,0,0,0,2,2,3,2,2,2,3,2,2,2,3,2}

// get_ref's sample (x, y) of the 8x8 block at quarter-pel vector (mvx, mvy): mc.c:181-202
__device__ __forceinline__ int lk_ref_px(const u8 *p0, const u8 *p1, const u8 *p2, const u8 *p3, int stride, ptrdiff_t off, int mvx, int mvy)
{
    const int qi = ((mvy & 3) << 2) + (mvx & 3);
    const ptrdiff_t o = off + (ptrdiff_t)(mvy >> 2) * stride + (mvx >> 2);
    const int k0 = (LK_HREF0 >> (2 * qi)) & 3, k1 = (LK_HREF1 >> (2 * qi)) & 3;
    const u8 *a = k0 == 0 ? p0 : k0 == 1 ? p1 : k0 == 2 ? p2 : p3;
    int v = a[o + ((mvy & 3) == 3 ? stride : 0)];
    if (qi & 5) {
        const u8 *b = k1 == 0 ? p0 : k1 == 1 ? p1 : k1 == 2 ? p2 : p3;
        v = (v + (int)b[o + ((mvx & 3) == 3)] + 1) >> 1;
    }
    return v;
}
// x264_pixel_satd_8x8 of a difference block, one sample per lane (lane = 8 * y + x): two 8x4 halves, each the sum of its two 4x4
// Hadamards halved once (R/common/pixel.c:211-253)
__device__ __forceinline__ int lk_satd8x8(int d, int lane)
{
    int t = dpp_mov<DPP_XOR1>(d); d = (lane & 1) ? t - d : d + t;
    t = dpp_mov<DPP_XOR2>(d); d = (lane & 2) ? t - d : d + t;
    t = __shfl_xor(d, 8, 64); d = (lane & 8) ? t - d : d + t;
    t = __shfl_xor(d, 16, 64); d = (lane & 16) ? t - d : d + t;
    int a = row_sum16(iabs(d));
    const int top = __builtin_amdgcn_readlane(a, 0) + __builtin_amdgcn_readlane(a, 16);
    const int bot = __builtin_amdgcn_readlane(a, 32) + __builtin_amdgcn_readlane(a, 48);
    return (top >> 1) + (bot >> 1);
}

// x264_pixel_sad_8x8 of a difference block, one sample per lane: mbcmp when lossless (R/encoder/encoder.c:610)
__device__ __forceinline__ int lk_sad8x8(int d) { return wave_sum(iabs(d)); }
