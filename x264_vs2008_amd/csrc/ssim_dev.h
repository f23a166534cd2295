// ssim_dev.h -- the arithmetic of the structural similarity metric (R/common/pixel.c:432-471), shared by the table entries
// ssim_4x4x2_core / ssim_end4 (l1_tables.hip) and the frame-level quality pass (frame_quality.hip).  Integer block sums and ONE float
// expression; the sums of ssim_end1 values are the callers', in the order the reference nests them.
#pragma once
#include "device_prims.h"

// one 4x4 block of ssim_4x4x2_core: {s1, s2, ss, s12}.  P: any pointer to bytes (generic or typed by address space)
template <class P> __device__ __forceinline__ void ssim_4x4_sums(P p1, int s1, P p2, int s2, int o[4])
{
    u32 a1 = 0, a2 = 0, ss = 0, s12 = 0;
    for (int y = 0; y < 4; y++)
        for (int x = 0; x < 4; x++) {
            int u = p1[y * s1 + x], v = p2[y * s2 + x];
            a1 += u; a2 += v; ss += u * u + v * v; s12 += u * v;
        }
    o[0] = a1; o[1] = a2; o[2] = ss; o[3] = s12;
}

// ssim_end1 (pixel.c:463-471): float products and one float division, each rounded once
__device__ __forceinline__ float ssim_end1(int s1, int s2, int ss, int s12)
{
    const int c1 = 416, c2 = 235963;   // (int)(.01*.01*255*255*64+.5), (int)(.03*.03*255*255*64*63+.5)
    int vars = ss * 64 - s1 * s1 - s2 * s2;
    int covar = s12 * 64 - s1 * s2;
    float num = __fmul_rn((float)(2 * s1 * s2 + c1), (float)(2 * covar + c2));
    float den = __fmul_rn((float)(s1 * s1 + s2 * s2 + c1), (float)(vars + c2));
    return __fdiv_rn(num, den);
}
