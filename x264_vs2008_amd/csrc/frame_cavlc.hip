// frame_cavlc.hip -- FRAME LEVEL, part 7: the CAVLC writer (x264_macroblock_write_cavlc with block_residual_write_cavlc and the skip
// runs of x264_slice_write, R/encoder/cavlc.c:60-620, R/encoder/encoder.c:1200-1280) for I, P and B slices, as a pass over the state a sweep
// left: macroblock types, partitions, references, vectors (of either list), prediction modes, cbp and the coefficient levels.
//
// CAVLC has no adaptive state, so nothing forces it into the macroblock loop: the RD levels do not run with it (R/encoder/rdo.c prices
// CAVLC bits with a counting twin of this writer; refused, as before) and a `--no-cabac` slice is the wavefront variant's -- constant QP,
// decisions and levels in the x264hip_mb_state -- or the raster variant's without its writer (adaptive quantisation, B slices, the chains
// of the frame queue: x264hip_cavlc_write_chains writes one slice per table entry, I, P and B chains in the same launch).  What the writer needs beyond the state it derives as the reference's cache does:
// the predicted vector of every partition (x264_mb_predict_mv on a scan8-shaped cache of the neighbours' vectors and references), the
// predicted intra mode (min of the left and top block's, DC when either is unavailable), and nC from the left and top block's
// coefficient counts -- the TOTALS block_residual_write_cavlc stores back (an encode leaves only non-zero flags there), kept here for
// the row above and the macroblock to the left.
// Mapping of the serial pass (x264hip_cavlc_write_frame / _chains): one wavefront per chain, lane 0 writes the slice's macroblocks one after
// the other, carrying the bit position, the skip run and the neighbours' totals as it goes; its only parallelism is the chains (what it costs
// next to the sweep it follows is measured in DESIGN.md, "The CAVLC writer beside the B sweep": 3.6 % of a B chain's sweep, 19 % of an
// I / P chain's).  The writer itself is cavlc_dev.h, text that also compiles for the host; here are the kernels around it and the entry
// points.  Payload layout as the CABAC writer's: X264HIP_PAYLOAD_LEAD bytes of each chain's slot, then slice_data() from bit 0, rbsp
// trailing bits included.
// Beside it, opt-in, the macroblock-parallel pass (x264hip_cavlc_write_frame_mp / _chains_mp, at the end of this file): a slice's bit string
// is serial only in its positions, which are a prefix sum of lengths every lane can count on its own.
#include "device_prims.h"
#include "frame_internal.h"
#include "cavlc_dev.h"

using namespace x264hip;

// The worst case of one CAVLC macroblock, for the "slot too small" check of both entry points and every slice type: the writer checks
// for space at the START of a macroblock only and stops BEFORE one that might not fit, so nothing smaller than this may be kept free.
// Bits, every syntax element at the longest code its type can take in this writer:
//   mb_skip_run          ue(v) of a 32-bit count                                                        63
//   mb_type              ue(v <= 48)                                                                    11
//   prediction           the larger of: I_4x4 (1 + 16 x 4 + ue(3) = 70) and P_8x8 with sub-8x8
//                        (4 sub types x ue(3) = 20, 4 ref_idx x ue(15) = 36, 16 vectors x 2 components x se of an int16 difference,
//                        |d| <= 65535 -> 33 bits: 1056; sum 1112); B_8x8 has 8 ref_idx and 8 vectors, less              1112
//   coded_block_pattern  ue(v <= 47) 11, transform_size_8x8_flag 1, mb_qp_delta se(|d| <= 26) 11                       23
//   one residual block   coeff_token 16, trailing-one signs 3, 16 levels x 36 (an int16 level through the High profile's escape:
//                        level code < 65536 ends at prefix 19, 20 + 16 bits), total_zeros 9, 15 x run_before 11       769
//   residual             I_16x16: DC + 16 AC blocks, or 16 4x4 blocks: at most 17; 2 chroma DC (4 levels: 8 + 3 + 4 x 36 + 3 = 158); 8 chroma AC
//                        17 x 769 + 2 x 158 + 8 x 769                                                                19541
// 63 + 11 + 1112 + 23 + 19541 = 20750 bits = 2594 bytes; the slice's end (the last skip run and the trailing bits, 63 + 8 bits) and the
// 7 bits cv_put may hold back add 10: 2604, rounded up to the next multiple of 64.
// Measured (tests/test_cavlc_host.py on tests/cavlc_synth.py's hand-built 3x2 slices, every level -32768 or +-32767 in turn, the largest
// macroblock of each in bits, High / Baseline profile): all I_16x16 14049 / 10977, all I_4x4 14091 / 11018, all P_8x8 of 4x4 blocks on
// reference 15 of 16 with vector differences of +-65535 15138 / 12066, all B_8x8 of bi-predicted blocks 14615 / 11542 -- at most 1893
// bytes.  The sum above is not reachable as a whole: 16 non-zero levels leave no total_zeros or run_before (- 174 bits a block), a block of 15
// coefficients holds 15 levels, and no macroblock type has both the 17 luma blocks and the P_8x8 prediction.
#define CV_MB_BYTES_MAX 2624

// every chain's slice of one frame: the same arguments, the chain is the block
__global__ __launch_bounds__(64) void k_cavlc_write(CvArgs a)
{
    __shared__ CvWork w;
    if (threadIdx.x != 0) return;
    cv_write_slice(a, (int)blockIdx.x, (CvWorkP)&w);
}
// one slice per table entry, each with its own state, slice type, QP and payload slot
__global__ __launch_bounds__(64) void k_cavlc_write_chains(const CvArgs *tab)
{
    __shared__ CvWork w;
    if (threadIdx.x != 0) return;
    const CvArgs &a = tab[blockIdx.x];
    cv_write_slice(a, a.chain, (CvWorkP)&w);
}

// the kernel's arguments for one slice from the ABI's description of it; what: the entry point's name in the error strings
// row_buffer: the serial writer's CvWork::top_nnz holds CV_MAX_W macroblocks; the macroblock-parallel pass has no row buffer
static int cv_build(x264hip_frame_ctx *c, const x264hip_mb_state *st, const x264hip_cavlc_params *p, const char *what, CvArgs &a, bool row_buffer = true)
{
    if (!st || !p || !st->luma || !p->payload || !p->payload_len) { set_error("%s: needs a state with coefficient levels and payload buffers", what); return -1; }
    if (p->slice_type != 0 && p->slice_type != 1 && p->slice_type != 2) { set_error("%s: slice type %d (0 P, 1 B, 2 I)", what, p->slice_type); return -1; }
    if (p->slice_type == 1 && (!st->mv1 || !st->ref1)) { set_error("%s: a B slice needs a state with list-1 arrays", what); return -1; }
    if (row_buffer && c->d.mb_w > CV_MAX_W) { set_error("%s: %d macroblocks per row, at most %d", what, c->d.mb_w, CV_MAX_W); return -1; }
    cv_args(a, st, p, c->d.mb_w, c->d.mb_h, st->progress + (size_t)c->d.mb_h * c->batch, CV_MB_BYTES_MAX);
    return 0;
}

extern "C" int x264hip_cavlc_write_frame(x264hip_frame_ctx *c, const x264hip_mb_state *st, const x264hip_cavlc_params *p)
{
    CvArgs a;
    if (cv_build(c, st, p, "cavlc_write_frame", a)) return -1;
    static_assert(4096 >= X264HIP_PAYLOAD_LEAD + CV_MB_BYTES_MAX, "the precondition implies room for one macroblock's worst case");
    if (p->payload_cap < 4096) { set_error("cavlc_write_frame: payload_cap"); return -1; }
    hipLaunchKernelGGL(k_cavlc_write, dim3((unsigned)c->batch), dim3(64), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

// The chain-table launch: every entry is ONE chain's slice with its own state, slice type, list-0 size, QP and payload slot.
extern "C" int x264hip_cavlc_write_chains(x264hip_frame_ctx *c, const x264hip_chain_cavlc *e, int n, void *staging_host, void *table_dev)
{
    if (n <= 0) return 0;
    if (!e || !staging_host || !table_dev) { set_error("cavlc_write_chains: entries / staging / table buffers missing"); return -1; }
    CvArgs *st = (CvArgs *)staging_host;
    for (int i = 0; i < n; i++) {
        if (e[i].chain < 0 || e[i].chain >= c->batch) { set_error("cavlc_write_chains: entry %d: chain %d", i, e[i].chain); return -1; }
        if (cv_build(c, e[i].state, e[i].params, "cavlc_write_chains", st[i])) return -1;
        if (e[i].params->payload_cap < X264HIP_PAYLOAD_LEAD + CV_MB_BYTES_MAX) {
            set_error("cavlc_write_chains: entry %d: a payload slot of %d bytes is smaller than one macroblock's worst case (%d bytes)", i,
                      e[i].params->payload_cap, X264HIP_PAYLOAD_LEAD + CV_MB_BYTES_MAX);
            return -1;
        }
        st[i].chain = e[i].chain;
    }
    HIPCHK(hipMemcpyAsync(table_dev, st, sizeof(CvArgs) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_cavlc_write_chains, dim3((unsigned)n), dim3(64), 0, c->stream, (const CvArgs *)table_dev);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" size_t x264hip_chain_cavlc_bytes(void) { return sizeof(CvArgs); }


// ---- The macroblock-parallel pass: count, scan, place (cavlc_dev.h, "The macroblock-parallel form") -------------------------------------
// The same slices from the same arguments, written by every lane instead of one.  Three phases, four launches, on the context's stream:
//   1  k_cavlc_mp_totals   one lane per residual block: the side array of coefficient totals nC is predicted from
//      k_cavlc_mp_count    one lane per macroblock, 64 macroblocks per wavefront: cv_mb into the counting sink -> bit lengths
//   2  k_cavlc_mp_scan     one workgroup per slice.  Its first wavefront walks the slice in steps of 64 macroblocks: a ballot over "has no
//                          bits" gives every lane its skip run (the run's code joins the length of the coded macroblock behind it, the last
//                          run and the trailing bits are element n_mb), a shuffle scan the inclusive offsets, a carry joins the steps.  It
//                          writes mb_bits (cv_write_slice's values) and payload_len, decides the aborts -- a comparison once the offsets are
//                          known --, and the whole workgroup then zeroes the payload_len bytes phase 3 merges its words into.
//   3  k_cavlc_mp_place    one lane per element: cv_mb into the placing sink at the element's offset.
// Mapping: one lane per macroblock, the serial text as it stands; the lanes' work arrays are CvWorkMp records in LDS, 532 bytes a lane,
// 33.3 KB a wavefront -- four wavefronts a compute unit by LDS.  (One wavefront per macroblock with a lane per residual block was not built.)
// Either form of call (tab == nullptr: every chain's slice of one frame from `a0`, blockIdx.y the chain; else one slice per table entry).
#define CVM_SLICE(a0_, tab_) const CvArgs &a = (tab_) ? (tab_)[blockIdx.y] : (a0_); const int bz = (tab_) ? a.chain : (int)blockIdx.y; \
                             const int n = a.mb_w * a.mb_h; const CvMpScratch s = cv_mp_scratch(scratch, (int)blockIdx.y, n)

__global__ __launch_bounds__(256) void k_cavlc_mp_totals(CvArgs a0, const CvArgs *tab, void *scratch)
{
    CVM_SLICE(a0, tab);
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= n * 24) return;
    s.tot[t] = (u8)cv_total(a, (size_t)n * bz + t / 24, t % 24);
}
__global__ __launch_bounds__(64) void k_cavlc_mp_count(CvArgs a0, const CvArgs *tab, void *scratch)
{
    __shared__ CvWorkMp w[64];
    CVM_SLICE(a0, tab);
    const int mb = (int)(blockIdx.x * 64 + threadIdx.x);
    if (mb >= n) return;
    CvCnt c = {0};
    s.off[mb] = cv_mb(a, bz, mb, s.tot, c, (CvWorkMpP)&w[threadIdx.x]) ? -1 : c.bits;
}
__global__ __launch_bounds__(256) void k_cavlc_mp_scan(CvArgs a0, const CvArgs *tab, void *scratch)
{
    __shared__ int sh_total, sh_start_last, sh_bad;
    CVM_SLICE(a0, tab);
    const bool is_p = a.slice_type == 0 || a.slice_type == 1;
    if (threadIdx.x < 64) {
        const int lane = (int)threadIdx.x;
        int carry = 0, carry_run = 0;
        bool bad = false;
        if (lane == 0) sh_start_last = 0;
        for (int base = 0; base <= n; base += 64) {
            const int idx = base + lane;
            int len = idx < n ? s.off[idx] : 0;
            bad |= len < 0;
            const bool skip = is_p && idx < n && len == 0;
            // the skipped macroblocks directly in front of this lane: up to the nearest lane below that is not skipped, or on into the step before
            const unsigned long long m = __ballot(skip), below = ~m & ((1ull << lane) - 1ull);
            const int run = below ? lane - 1 - (63 - __builtin_clzll(below)) : lane + carry_run;
            if (idx < n && !skip && is_p) len += cv_skip_run_bits(run);
            int x = len;
            for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d); if (lane >= d) x += y; }
            x += carry;
            if (idx == n) { CvCnt c = {0}; cv_slice_end(c, is_p, run, x); x += c.bits; }       // (no length so far: x is the element's start)
            if (idx <= n) {
                s.off[idx] = x;
                s.run[idx] = skip ? 0 : run;
                if (idx < n && a.mb_bits) a.mb_bits[(size_t)n * bz + idx] = x;
                if (idx == n - 2) sh_start_last = x;
                if (idx == n) sh_total = x;
            }
            carry = __shfl(x, 63);
            carry_run = ~m ? __builtin_clzll(~m) : carry_run + 64;
        }
        bad = __any(bad);
        if (lane == 0) sh_bad = bad;
    }
    __syncthreads();
    const int bytes = sh_total >> 3;
    if (sh_bad || cv_slot_too_small(a, sh_start_last, bytes)) {
        if (threadIdx.x == 0) { CV_ABORT(a.abort_flag); a.payload_len[bz] = 0; }
        return;
    }
    if (threadIdx.x == 0) a.payload_len[bz] = bytes;
    // zero [0, bytes) of the slot's payload: single bytes up to the first 16-byte boundary and behind the last
    u8 *out = a.payload + (size_t)bz * a.payload_cap + 64;
    int head = (int)((16 - ((size_t)out & 15)) & 15);
    if (head > bytes) head = bytes;
    const int body = (bytes - head) >> 4, tail = bytes - head - (body << 4);
    for (int i = (int)threadIdx.x; i < head; i += 256) out[i] = 0;
    for (int i = (int)threadIdx.x; i < body; i += 256) ((uint4 *)(out + head))[i] = make_uint4(0, 0, 0, 0);
    for (int i = (int)threadIdx.x; i < tail; i += 256) out[head + (body << 4) + i] = 0;
}
__global__ __launch_bounds__(64) void k_cavlc_mp_place(CvArgs a0, const CvArgs *tab, void *scratch)
{
    __shared__ CvWorkMp w[64];
    CVM_SLICE(a0, tab);
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i > n || a.payload_len[bz] == 0) return;                                  // an aborted slice: nothing is placed
    const int start = i ? s.off[i - 1] : 0;
    if (s.off[i] == start) return;                                                // a skipped macroblock
    const bool is_p = a.slice_type == 0 || a.slice_type == 1;
    CvPl b;
    cv_pl_begin(b, a.payload + (size_t)bz * a.payload_cap + 64, start);
    if (i == n) cv_slice_end(b, is_p, s.run[n], start);
    else {
        if (is_p) cv_skip_run(b, s.run[i]);
        cv_mb(a, bz, i, s.tot, b, (CvWorkMpP)&w[threadIdx.x]);
    }
    cv_pl_end(b);
}

static int cvm_launch(x264hip_frame_ctx *c, const CvArgs &a0, const CvArgs *tab, int n_slices, void *scratch)
{
    const unsigned n = (unsigned)(c->d.mb_w * c->d.mb_h), S = (unsigned)n_slices;
    hipLaunchKernelGGL(k_cavlc_mp_totals, dim3((n * 24 + 255) / 256, S), dim3(256), 0, c->stream, a0, tab, scratch);
    hipLaunchKernelGGL(k_cavlc_mp_count, dim3((n + 63) / 64, S), dim3(64), 0, c->stream, a0, tab, scratch);
    hipLaunchKernelGGL(k_cavlc_mp_scan, dim3(1, S), dim3(256), 0, c->stream, a0, tab, scratch);
    hipLaunchKernelGGL(k_cavlc_mp_place, dim3((n + 1 + 63) / 64, S), dim3(64), 0, c->stream, a0, tab, scratch);
    HIPCHK(hipGetLastError());
    return 0;
}
#define CVM_MAX_SLICES 65535         // a launch's slices are its grid's second dimension

extern "C" size_t x264hip_cavlc_mp_scratch_bytes(const x264hip_frame_ctx *c, int n_slices)
{
    return c && n_slices > 0 ? cv_mp_scratch_bytes(c->d.mb_w * c->d.mb_h) * (size_t)n_slices : 0;
}

extern "C" int x264hip_cavlc_write_frame_mp(x264hip_frame_ctx *c, const x264hip_mb_state *st, const x264hip_cavlc_params *p, void *scratch_dev)
{
    CvArgs a;
    if (cv_build(c, st, p, "cavlc_write_frame", a, false)) return -1;
    if (p->payload_cap < 4096) { set_error("cavlc_write_frame: payload_cap"); return -1; }
    if (!scratch_dev) { set_error("cavlc_write_frame_mp: scratch buffer missing"); return -1; }
    if (c->batch > CVM_MAX_SLICES) { set_error("cavlc_write_frame_mp: %d chains, at most %d in one call", c->batch, CVM_MAX_SLICES); return -1; }
    return cvm_launch(c, a, nullptr, c->batch, scratch_dev);
}

extern "C" int x264hip_cavlc_write_chains_mp(x264hip_frame_ctx *c, const x264hip_chain_cavlc *e, int n, void *staging_host, void *table_dev, void *scratch_dev)
{
    if (n <= 0) return 0;
    if (!e || !staging_host || !table_dev) { set_error("cavlc_write_chains: entries / staging / table buffers missing"); return -1; }
    if (!scratch_dev) { set_error("cavlc_write_chains_mp: scratch buffer missing"); return -1; }
    if (n > CVM_MAX_SLICES) { set_error("cavlc_write_chains_mp: %d entries, at most %d in one call", n, CVM_MAX_SLICES); return -1; }
    CvArgs *st = (CvArgs *)staging_host;
    for (int i = 0; i < n; i++) {
        if (e[i].chain < 0 || e[i].chain >= c->batch) { set_error("cavlc_write_chains: entry %d: chain %d", i, e[i].chain); return -1; }
        if (cv_build(c, e[i].state, e[i].params, "cavlc_write_chains", st[i], false)) return -1;
        if (e[i].params->payload_cap < X264HIP_PAYLOAD_LEAD + CV_MB_BYTES_MAX) {
            set_error("cavlc_write_chains: entry %d: a payload slot of %d bytes is smaller than one macroblock's worst case (%d bytes)", i,
                      e[i].params->payload_cap, X264HIP_PAYLOAD_LEAD + CV_MB_BYTES_MAX);
            return -1;
        }
        st[i].chain = e[i].chain;
    }
    HIPCHK(hipMemcpyAsync(table_dev, st, sizeof(CvArgs) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    return cvm_launch(c, st[0], (const CvArgs *)table_dev, n, scratch_dev);
}
