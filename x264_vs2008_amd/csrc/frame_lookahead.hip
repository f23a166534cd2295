// frame_lookahead.hip -- FRAME LEVEL, part 5: the intra half of the lookahead's
// per-macroblock cost (x264_slicetype_mb_cost, R/encoder/slicetype.c:186-245):
// for every 8x8 block of the half-resolution luma plane, predict it from its
// SOURCE neighbours (not a reconstruction, so every block is independent) with
// the four 8x8 chroma-style predictors (DC, H, V, plane) and the six
// directional 8x8 luma predictors (DDL..HU) on the low-passed edge
// (x264_predict_8x8_filter with all neighbours), score each with SATD 8x8
// (mbcmp at subme > 1), keep the minimum and add the intra penalty (5).
// The result is frame->i_intra_cost[mb].
//
// Mapping: three lowres blocks per wavefront; lane = (block, mode 0..9, upper /
// lower 8x4 half).  Each lane builds its 32 predicted pixels in registers from
// the 17 + 8 neighbours, takes the two-lane SWAR Hadamard of the difference,
// the halves are added with one shuffle and a lane per block takes the minimum.
#include "device_prims.h"
#include "frame_internal.h"

using namespace x264hip;

#define LA_WAVES 4
#define LA_MB_PER_WAVE 3

__device__ __forceinline__ int la_f2(int a, int b, int c) { return (a + 2 * b + c + 2) >> 2; }
__device__ __forceinline__ int la_f1(int a, int b) { return (a + b + 1) >> 1; }

// directional 8x8 predictor for pixel (x,y) from the filtered edge e[]:
// e[7-k] = left k, e[8] = top-left, e[9+k] = top k (k < 16).  H.264 8.3.2.2 /
// R/common/predict.c:618-751; modes 3 DDL, 4 DDR, 5 VR, 6 HD, 7 VL, 8 HU.
__device__ int la_dir8(int mode, const int *e, int x, int y)
{
#define EL(k) e[7 - (k)]
#define ET(k) e[9 + (k)]
#define EZ(k) e[8 + (k)]
    switch (mode) {
    case 3:
        if (x == 7 && y == 7) return la_f2(ET(14), ET(15), ET(15));
        return la_f2(ET(x + y), ET(x + y + 1), ET(x + y + 2));
    case 4:
        return la_f2(EZ(x - y - 1), EZ(x - y), EZ(x - y + 1));
    case 5: {
        int z = 2 * x - y, i = x - (y >> 1);
        if (z >= 0) return (z & 1) ? la_f2(EZ(i - 1), EZ(i), EZ(i + 1)) : la_f1(EZ(i), EZ(i + 1));
        if (z == -1) return la_f2(EL(0), EZ(0), ET(0));
        return la_f2(EL(y - 2 * x - 1), EL(y - 2 * x - 2), EL(y - 2 * x - 3));
    }
    case 6: {
        int z = 2 * y - x, i = y - (x >> 1);
        if (z >= 0) return (z & 1) ? la_f2(EZ(-i + 1), EZ(-i), EZ(-i - 1)) : la_f1(EZ(-i), EZ(-i - 1));
        if (z == -1) return la_f2(EL(0), EZ(0), ET(0));
        return la_f2(ET(x - 2 * y - 1), ET(x - 2 * y - 2), ET(x - 2 * y - 3));
    }
    case 7: {
        int i = x + (y >> 1);
        return (y & 1) ? la_f2(ET(i), ET(i + 1), ET(i + 2)) : la_f1(ET(i), ET(i + 1));
    }
    default: {
        int z = x + 2 * y, i = y + (x >> 1);
        if (z > 13) return EL(7);
        if (z == 13) return la_f2(EL(6), EL(7), EL(7));
        return (z & 1) ? la_f2(EL(i), EL(i + 1), EL(i + 2)) : la_f1(EL(i), EL(i + 1));
    }
    }
#undef EL
#undef ET
#undef EZ
}

// The block scorer is look_intra_body.h, textually included by both kernels with SAD in scope: false = SATD 8x8; true = mbcmp is SAD
// (lossless, R/encoder/encoder.c:610), the same predictions scored by the sum of absolute differences.
__global__ __launch_bounds__(64 * LA_WAVES) void k_lookahead_intra(const u8 *__restrict__ low, size_t bs, int stride, int mb_w, int mb_count,
                                                                    int *__restrict__ out)
{
    constexpr bool SAD = false;
#include "look_intra_body.h"
}
__global__ __launch_bounds__(64 * LA_WAVES) void k_lookahead_intra_sad(const u8 *__restrict__ low, size_t bs, int stride, int mb_w, int mb_count,
                                                                        int *__restrict__ out)
{
    constexpr bool SAD = true;
#include "look_intra_body.h"
}

static int lookahead_intra(x264hip_frame_ctx *c, const x264hip_picture *pic, int32_t *out_cost_dev, bool sad)
{
    int n = c->d.mb_w * c->d.mb_h;
    int per_block = LA_WAVES * LA_MB_PER_WAVE;
    hipLaunchKernelGGL(sad ? k_lookahead_intra_sad : k_lookahead_intra, dim3((n + per_block - 1) / per_block, c->batch), dim3(64 * LA_WAVES), 0, c->stream,
                       pic->lowres[0], c->bs_l, pic->stride_lowres, c->d.mb_w, n, out_cost_dev);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int x264hip_lookahead_intra_frame(x264hip_frame_ctx *c, const x264hip_picture *pic, int32_t *out_cost_dev)
{
    return lookahead_intra(c, pic, out_cost_dev, false);
}
// the same when mbcmp is SAD: lossless (x264hip_look_params.lossless, which x264hip_lookahead_cost_frames then needs too)
extern "C" int x264hip_lookahead_intra_frame_sad(x264hip_frame_ctx *c, const x264hip_picture *pic, int32_t *out_cost_dev)
{
    return lookahead_intra(c, pic, out_cost_dev, true);
}
