// frame_quality.hip -- what x264_fdec_filter_row measures (PSNR's squared error and SSIM, R/encoder/encoder.c:1031-1056) and what x264_slice_write counts
// per macroblock (h->stat.frame, encoder.c:1229-1251), per coded frame, as one pass over the finished pictures and the state the sweep left: for every
// entry of a chain table -- chains that code different kinds of frames from different pictures -- in two launches on the context's stream.
//
// The reference measures in chunks: x264_fdec_filter_row runs once per macroblock row and once at the end, and call k (k = 1 .. mb_h) covers the pixel rows
// [max(16 (k - 1) - 8, 0), k == mb_h ? height : 16 k - 8).  The squared error is an integer sum and does not care.  SSIM does: every call returns a FLOAT
// (x264_pixel_ssim_wxh, R/common/pixel.c:485-509: a float accumulator over row pairs top to bottom and groups of four left to right, each group itself a
// float sum of at most four ssim_end1 values starting at zero), and the calls' floats are added into a double.  Float addition does not associate, so the
// adds are done here in exactly that nesting: k_quality_chunks gives each (entry, call) one workgroup, which computes the block sums and the ssim_end1
// values in parallel (integers and a pure function: order-free), the groups' sums side by side (each its own four ordered adds), and lets ONE lane chain
// the group sums of each row pair; k_quality_finish adds an entry's chunk floats in chunk order into the double and the chunks' squared errors into the
// record, and counts the macroblocks.  Nothing is read outside the visible picture: the block column ssim_4x4x2_core computes beyond an odd column count
// is never read by ssim_end4 and is not computed here.
#include "frame_internal.h"
#include "ssim_dev.h"
#include "mb_vocab.h"
#include "../../include/x264hip_stream.h"

using x264hip::set_error;

#define FQ_THREADS 256
typedef const __attribute__((address_space(1))) u8 *fq_pix;
typedef __attribute__((address_space(3))) int *fq_lds_i;
typedef __attribute__((address_space(3))) float *fq_lds_f;
typedef __attribute__((address_space(3))) unsigned long long *fq_lds_q;

// one entry as the kernels read it: the element's planes and state arrays already resolved
struct FqEntry {
    const u8 *src[3], *rec[3];
    const int8_t *mb_type, *partition, *sub_partition, *ref, *ref1, *t8, *qp;
    const int16_t *cbp;
    int slice_type, psnr, ssim, count_refs;
};
struct FqChunk { unsigned long long ssd[3]; float ssim; int pad; };
struct FqDims { int width, height, stride_y, stride_c, mb_w, mb_h; };

// squared error of `rows` rows of `w` pixels, this thread's share
__device__ __forceinline__ unsigned long long fq_ssd_rows(fq_pix a, fq_pix b, int stride, int w, int rows, int tid)
{
    unsigned long long part = 0;
    const int nq = (w + 3) >> 2;
    for (int i = tid; i < nq * rows; i += FQ_THREADS) {
        const int y = i / nq, x = (i - y * nq) * 4;
        fq_pix pa = a + (ptrdiff_t)y * stride + x, pb = b + (ptrdiff_t)y * stride + x;
        u32 s = 0;
        for (int j = 0; j < 4 && x + j < w; j++) { int d = (int)pa[j] - (int)pb[j]; s += (u32)(d * d); }
        part += s;
    }
    return part;
}

// LDS of k_quality_chunks (dynamic, every carve a multiple of 16 bytes): [0, 128) the waves' squared errors, then two rows of block sums
// (w4 x int[4] each: the reference's sum0 / sum1), then one float per group of four
extern __shared__ __attribute__((aligned(16))) char fq_smem[];
static size_t fq_lds_bytes(int width)
{
    const int w4 = (width - 2) >> 2;
    return 128 + (size_t)2 * (w4 > 0 ? w4 : 0) * 16 + align_up_sz((size_t)((w4 > 0 ? w4 : 0) / 4 + 1) * 4, 16);
}

// grid (mb_h, n): block (k - 1, e) is call k of x264_fdec_filter_row for entry e
__global__ __launch_bounds__(FQ_THREADS) void k_quality_chunks(const FqEntry *tab, FqDims d, FqChunk *scratch)
{
    const FqEntry &e = tab[blockIdx.y];
    const int tid = threadIdx.x, k = blockIdx.x + 1;
    const bool b_end = k == d.mb_h;
    int min_y = (k - 1) * 16 - 8;
    if (min_y < 0) min_y = 0;
    const int max_y = b_end ? d.height : k * 16 - 8;
    FqChunk *out = scratch + (size_t)blockIdx.y * d.mb_h + blockIdx.x;
    fq_lds_q s_ssd = (fq_lds_q)fq_smem;                                  // [4 waves][3]

    if (e.psnr) {                                                        // encoder.c:1034-1043
        for (int p = 0; p < 3; p++) {
            const int sh = p ? 1 : 0, st = p ? d.stride_c : d.stride_y;
            unsigned long long part = fq_ssd_rows((fq_pix)e.rec[p] + (ptrdiff_t)(min_y >> sh) * st, (fq_pix)e.src[p] + (ptrdiff_t)(min_y >> sh) * st, st,
                                                  d.width >> sh, (max_y - min_y) >> sh, tid);
            for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
            if ((tid & 63) == 0) s_ssd[(tid >> 6) * 3 + p] = part;
        }
    }
    __syncthreads();
    if (tid == 0) {
        for (int p = 0; p < 3; p++) out->ssd[p] = e.psnr ? s_ssd[p] + s_ssd[3 + p] + s_ssd[6 + p] + s_ssd[9 + p] : 0ull;
        out->pad = 0;
    }

    // encoder.c:1045-1056 and x264_pixel_ssim_wxh: luma from column 2 and row y0, (width - 2) x (max_y - y0)
    const int y0 = min_y == 0 ? 2 : min_y - 6;
    const int w4 = (d.width - 2) >> 2, h4 = (max_y - y0) >> 2;
    float ssim = 0.0f;                                                   // thread 0's: the call's accumulator
    if (e.ssim && w4 > 1 && h4 > 1) {
        fq_lds_i sums = (fq_lds_i)(fq_smem + 128);
        fq_lds_f gsum = (fq_lds_f)(fq_smem + 128 + (size_t)2 * w4 * 16);
        const int n_end1 = w4 - 1, n_grp = (n_end1 + 3) >> 2;
        fq_pix rec = (fq_pix)e.rec[0] + (ptrdiff_t)y0 * d.stride_y + 2, src = (fq_pix)e.src[0] + (ptrdiff_t)y0 * d.stride_y + 2;
        for (int z = 0; z < h4; z++) {
            fq_lds_i cur = sums + (z & 1) * w4 * 4;
            for (int x = tid; x < w4; x += FQ_THREADS) {                 // ssim_4x4x2_core for block row z (integers)
                int o[4];
                const ptrdiff_t off = (ptrdiff_t)(4 * z) * d.stride_y + 4 * x;
                ssim_4x4_sums(rec + off, d.stride_y, src + off, d.stride_y, o);
                for (int j = 0; j < 4; j++) cur[4 * x + j] = o[j];
            }
            __syncthreads();
            if (z >= 1) {
                fq_lds_i s0 = sums, s1 = sums + w4 * 4;
                for (int g = tid; g < n_grp; g += FQ_THREADS) {          // ssim_end4 of group g: its own float sum from zero, left to right
                    const int x = 4 * g, cnt = n_end1 - x < 4 ? n_end1 - x : 4;
                    float acc = 0.0f;
                    for (int i = x; i < x + cnt; i++) {
                        int t[4];
                        for (int j = 0; j < 4; j++) t[j] = s0[4 * i + j] + s0[4 * i + 4 + j] + s1[4 * i + j] + s1[4 * i + 4 + j];
                        acc = __fadd_rn(acc, ssim_end1(t[0], t[1], t[2], t[3]));
                    }
                    gsum[g] = acc;
                }
                __syncthreads();
                if (tid == 0)                                            // the ordered chain of this row pair
                    for (int g = 0; g < n_grp; g++) ssim = __fadd_rn(ssim, gsum[g]);
                __syncthreads();
            }
        }
    }
    if (tid == 0) out->ssim = ssim;
}

// grid (n): the entry's record -- chunk sums in chunk order, and h->stat.frame's counters from the state
__global__ __launch_bounds__(FQ_THREADS) void k_quality_finish(const FqEntry *tab, FqDims d, const FqChunk *scratch, x264hip_frame_report *out_all)
{
    enum { H_TYPE = 0, H_PART = 19, H_T8 = 36, H_REF = 38, H_QP = 102, H_N = 103 };
    __shared__ int h[H_N];
    const FqEntry &e = tab[blockIdx.x];
    const int tid = threadIdx.x;
    for (int i = tid; i < H_N; i += FQ_THREADS) h[i] = 0;
    __syncthreads();
    if (e.mb_type) {
        const int n_mb = d.mb_w * d.mb_h;
        int qp_sum = 0;
        for (int mb = tid; mb < n_mb; mb += FQ_THREADS) {
            const int type = e.mb_type[mb];
            qp_sum += e.qp[mb];
            if (type < 0 || type >= 19) continue;
            atomicAdd(&h[H_TYPE + type], 1);
            const bool intra = IS_INTRA_T(type);
            if (!intra && !IS_SKIP_T(type) && type != T_B_DIRECT) {
                const int part = e.partition[mb];
                if (part != D_8x8) { if (part >= 0 && part < 17) atomicAdd(&h[H_PART + part], 4); }
                else
                    for (int i = 0; i < 4; i++) { const int sp = e.sub_partition[4 * mb + i]; if (sp >= 0 && sp < 17) atomicAdd(&h[H_PART + sp], 1); }
                if (e.count_refs)
                    for (int l = 0; l <= (e.slice_type == 1 && e.ref1 ? 1 : 0); l++)
                        for (int i = 0; i < 4; i++) {
                            const int r = (l ? e.ref1 : e.ref)[4 * mb + i];
                            if (r >= 0 && r < 32) atomicAdd(&h[H_REF + 32 * l + r], 1);
                        }
            }
            if ((e.cbp[mb] & 15) && !intra) { atomicAdd(&h[H_T8], 1); if (e.t8[mb]) atomicAdd(&h[H_T8 + 1], 1); }
        }
        for (int m = 32; m >= 1; m >>= 1) qp_sum += __shfl_xor(qp_sum, m, 64);
        if ((tid & 63) == 0) atomicAdd(&h[H_QP], qp_sum);
    }
    __syncthreads();
    x264hip_frame_report *r = out_all + blockIdx.x;
    for (int i = tid; i < 19; i += FQ_THREADS) r->mb_count[i] = h[H_TYPE + i];
    for (int i = tid; i < 17; i += FQ_THREADS) r->mb_partition[i] = h[H_PART + i];
    for (int i = tid; i < 64; i += FQ_THREADS) r->mb_count_ref[i >> 5][i & 31] = h[H_REF + i];
    if (tid == 0) {
        r->mb_count_8x8dct[0] = h[H_T8]; r->mb_count_8x8dct[1] = h[H_T8 + 1];
        r->qp_sum = h[H_QP];
        r->reserved = 0;
        const FqChunk *ch = scratch + (size_t)blockIdx.x * d.mb_h;
        unsigned long long ssd[3] = {0, 0, 0};
        double f_ssim = 0.0;                                             // h->stat.frame.f_ssim += (float) x264_pixel_ssim_wxh(...)
        for (int k = 0; k < d.mb_h; k++) {
            for (int p = 0; p < 3; p++) ssd[p] += ch[k].ssd[p];
            f_ssim = __dadd_rn(f_ssim, (double)ch[k].ssim);
        }
        for (int p = 0; p < 3; p++) r->ssd[p] = (int64_t)ssd[p];
        r->ssim = f_ssim;
    }
}

static const u8 *fq_elem(const u8 *plane, size_t bs, int b) { return plane + bs * (size_t)b; }

static int fq_build(x264hip_frame_ctx *c, const x264hip_chain_report &e, int i, FqEntry &o)
{
    if (!e.fenc || !e.recon || !e.fenc->plane[0] || !e.recon->plane[0]) { set_error("frame_report: entry %d: source / reconstruction picture missing", i); return -1; }
    if (e.chain < 0 || e.chain >= c->batch || e.fenc_element < 0 || e.fenc_element >= c->batch || e.recon_element < 0 || e.recon_element >= c->batch) {
        set_error("frame_report: entry %d: chain %d, elements %d / %d of a batch of %d", i, e.chain, e.fenc_element, e.recon_element, c->batch);
        return -1;
    }
    if (e.slice_type < 0 || e.slice_type > 2) { set_error("frame_report: entry %d: slice type %d (0 P, 1 B, 2 I)", i, e.slice_type); return -1; }
    for (int p = 0; p < 3; p++) {
        o.src[p] = fq_elem(e.fenc->plane[p], p ? c->bs_c : c->bs_y, e.fenc_element);
        o.rec[p] = fq_elem(e.recon->plane[p], p ? c->bs_c : c->bs_y, e.recon_element);
    }
    const x264hip_mb_state *s = e.state;
    const size_t n = (size_t)c->d.mb_w * c->d.mb_h * e.chain;
    if (s && (!s->mb_type || !s->partition || !s->sub_partition || !s->ref || !s->t8 || !s->qp || !s->cbp)) { set_error("frame_report: entry %d: incomplete state", i); return -1; }
    o.mb_type = s ? s->mb_type + n : nullptr;
    o.partition = s ? s->partition + n : nullptr;
    o.sub_partition = s ? s->sub_partition + 4 * n : nullptr;
    o.ref = s ? s->ref + 4 * n : nullptr;
    o.ref1 = s && s->ref1 ? s->ref1 + 4 * n : nullptr;
    o.t8 = s ? s->t8 + n : nullptr;
    o.qp = s ? s->qp + n : nullptr;
    o.cbp = s ? s->cbp + n : nullptr;
    o.slice_type = e.slice_type; o.psnr = !!e.psnr; o.ssim = !!e.ssim; o.count_refs = !!e.count_refs;
    return 0;
}

extern "C" size_t x264hip_chain_report_bytes(void) { return sizeof(FqEntry); }
extern "C" size_t x264hip_frame_report_scratch_bytes(const x264hip_frame_ctx *c) { return c ? sizeof(FqChunk) * (size_t)c->d.mb_h : 0; }

extern "C" int x264hip_frame_report_chains(x264hip_frame_ctx *c, const x264hip_chain_report *e, int n, void *staging_host, void *table_dev, void *scratch_dev,
                                           x264hip_frame_report *out_dev)
{
    if (n <= 0) return 0;
    if (!c || !e || !staging_host || !table_dev || !scratch_dev || !out_dev) { set_error("frame_report_chains: entries / staging / table / scratch / output buffers missing"); return -1; }
    const size_t lds = fq_lds_bytes(c->d.width);
    if (lds > 64 * 1024) { set_error("frame_report_chains: a picture %d pixels wide needs %zu bytes of LDS per chunk, at most 65536", c->d.width, lds); return -1; }
    FqEntry *st = (FqEntry *)staging_host;
    for (int i = 0; i < n; i++)
        if (fq_build(c, e[i], i, st[i])) return -1;
    const FqDims d = {c->d.width, c->d.height, c->d.stride_y, c->d.stride_c, c->d.mb_w, c->d.mb_h};
    HIPCHK(hipMemcpyAsync(table_dev, st, sizeof(FqEntry) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_quality_chunks, dim3((unsigned)d.mb_h, (unsigned)n), dim3(FQ_THREADS), lds, c->stream, (const FqEntry *)table_dev, d, (FqChunk *)scratch_dev);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_quality_finish, dim3((unsigned)n), dim3(FQ_THREADS), 0, c->stream, (const FqEntry *)table_dev, d, (const FqChunk *)scratch_dev, out_dev);
    HIPCHK(hipGetLastError());
    return 0;
}

// lock step: every element of the batch, one source picture, one reconstruction, one state; out_dev [batch] records in element order
extern "C" int x264hip_frame_report_frame(x264hip_frame_ctx *c, const x264hip_picture *fenc, const x264hip_picture *recon, const x264hip_mb_state *state,
                                          int slice_type, int flags, void *staging_host, void *table_dev, void *scratch_dev, x264hip_frame_report *out_dev)
{
    if (!c || !staging_host) { set_error("frame_report_frame: context / staging buffer missing"); return -1; }
    // the entries themselves are built behind the kernel table in the staging buffer: x264hip_frame_report_frame_staging_bytes() per element
    x264hip_chain_report *e = (x264hip_chain_report *)((char *)staging_host + align_up_sz(sizeof(FqEntry) * (size_t)c->batch, 16));
    for (int b = 0; b < c->batch; b++) {
        e[b].chain = b; e[b].fenc = fenc; e[b].fenc_element = b; e[b].recon = recon; e[b].recon_element = b; e[b].state = state;
        e[b].slice_type = slice_type; e[b].psnr = flags & X264HIP_REPORT_PSNR; e[b].ssim = flags & X264HIP_REPORT_SSIM; e[b].count_refs = flags & X264HIP_REPORT_REFS;
    }
    return x264hip_frame_report_chains(c, e, c->batch, staging_host, table_dev, scratch_dev, out_dev);
}
extern "C" size_t x264hip_frame_report_frame_staging_bytes(void) { return sizeof(FqEntry) + sizeof(x264hip_chain_report) + 16; }
