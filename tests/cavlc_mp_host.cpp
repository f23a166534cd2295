// cavlc_mp_host.cpp -- the macroblock-parallel form of the product's CAVLC writer (x264_vs2008_amd/csrc/cavlc_dev.h: cv_total, cv_mb in its
// counting and its placing mode, cv_skip_run, cv_slice_end, cv_slot_too_small) compiled for the host alone, with g++ and no HIP.
// tests/cavlc_mp_host_util.py builds it as a shared library and tests/test_cavlc_mp_host.py feeds it one frame's state arrays; with
// -DCAVLC_MP_HOST_MAIN it is a program of its own that compares the three phases with cv_write_slice on made-up slices (the build the
// sanitizers take).  The phases visit the macroblocks in REVERSE raster order: whatever the text still carried from one macroblock to the
// next would show.  The scan between them is the plain serial one -- the kernels' wave scan is the device's business.
#define X264HIP_HOST_TEST 1
#include "cavlc_dev.h"
#include <vector>

// Count, scan, place for the slice `a` of chain 0 (n macroblocks).  Returns the number of aborts raised.
static int mp_write(const CvArgs &a, int n)
{
    std::vector<unsigned char> mem(cv_mp_scratch_bytes(n), 0xAA);
    const CvMpScratch s = cv_mp_scratch(mem.data(), 0, n);
    const bool is_p = a.slice_type == 0 || a.slice_type == 1;
    CvWorkMp w;
    // phase 1: totals, then lengths
    for (int mb = n - 1; mb >= 0; mb--)
        for (int k = 23; k >= 0; k--) s.tot[(size_t)mb * 24 + k] = (u8)cv_total(a, (size_t)mb, k);
    for (int mb = n - 1; mb >= 0; mb--) {
        memset(&w, 0xAA, sizeof(w));
        CvCnt c = {0};
        s.off[mb] = cv_mb(a, 0, mb, s.tot, c, &w) ? -1 : c.bits;
    }
    // phase 2: offsets and skip runs
    int pos = 0, run = 0, start_last = 0;
    bool bad = false;
    for (int mb = 0; mb < n; mb++) {
        int len = s.off[mb];
        bad |= len < 0;
        start_last = pos;
        s.run[mb] = 0;
        if (is_p && len == 0) run++;
        else if (is_p) { len += cv_skip_run_bits(run); s.run[mb] = run; run = 0; }
        pos += len;
        s.off[mb] = pos;
        if (a.mb_bits) a.mb_bits[mb] = pos;
    }
    CvCnt end = {0};
    cv_slice_end(end, is_p, run, pos);
    s.run[n] = run;
    s.off[n] = pos + end.bits;
    if (bad || cv_slot_too_small(a, start_last, s.off[n] >> 3)) { CV_ABORT(a.abort_flag); a.payload_len[0] = 0; return *a.abort_flag; }
    a.payload_len[0] = s.off[n] >> 3;
    u8 *out = a.payload + 64;
    memset(out, 0, (size_t)a.payload_len[0]);
    // phase 3: every element at its offset
    for (int i = n; i >= 0; i--) {
        const int start = i ? s.off[i - 1] : 0;
        if (s.off[i] == start) continue;
        CvPl b;
        cv_pl_begin(b, out, start);
        if (i == n) cv_slice_end(b, is_p, s.run[n], start);
        else {
            memset(&w, 0xAA, sizeof(w));
            if (is_p) cv_skip_run(b, s.run[i]);
            cv_mb(a, 0, i, s.tot, b, &w);
        }
        cv_pl_end(b);
    }
    return 0;
}

// The ABI's arguments as tests/cavlc_host.cpp takes them.  Returns 0 and the length in p->payload_len[0], 1 when the pass stopped (length 0).
extern "C" int cavlc_mp_host_write_slice(const x264hip_mb_state *st, const x264hip_cavlc_params *p, int mb_w, int mb_h, int margin)
{
    CvArgs a;
    int aborted = 0;
    cv_args(a, st, p, mb_w, mb_h, &aborted, margin);
    mp_write(a, mb_w * mb_h);
    return aborted;
}
// cv_write_slice on the same arguments (the yardstick, in the same build)
extern "C" int cavlc_mp_host_write_slice_serial(const x264hip_mb_state *st, const x264hip_cavlc_params *p, int mb_w, int mb_h, int margin)
{
    if (mb_w > CV_MAX_W) return -1;
    CvWork w;
    CvArgs a;
    int aborted = 0;
    memset(&w, 0xAA, sizeof(w));
    cv_args(a, st, p, mb_w, mb_h, &aborted, margin);
    cv_write_slice(a, 0, &w);
    return aborted;
}

#ifdef CAVLC_MP_HOST_MAIN
#include <stdio.h>
// Made-up slices of 5 x 3 macroblocks: I_16x16 and I_4x4 with random levels in an I slice; P_L0 16x16, P_8x8 and P_SKIP with random vectors
// and levels in a P slice whose runs of skipped macroblocks include the slice's first and last macroblocks.  The slot is exactly as long as
// the entry points demand and the buffer ends with the slot, so a byte touched behind it is the sanitizer's to report.
static unsigned rnd_state = 12345u;
static int rnd(int n) { rnd_state = rnd_state * 1664525u + 1013904223u; return (int)((rnd_state >> 8) % (unsigned)n); }

static int run_case(int slice_type, int variant)
{
    const int W = 5, H = 3, n = W * H, margin = 2624;
    std::vector<signed char> mb_type(n), partition(n, D_16x16), sub(n * 4, D_L0_8x8), ref(n * 4, 0), ref1(n * 4, -1), i4mode(n * 16), i16mode(n), chroma_mode(n), t8(n, 0), qp(n);
    std::vector<i16> mv(n * 32, 0), mv1(n * 32, 0), cbp(n), luma(n * 256, 0), luma_dc(n * 16, 0), chroma_dc(n * 8, 0), chroma_ac(n * 128, 0);
    int last_qp = 30;
    for (int m = 0; m < n; m++) {
        const int r = rnd(6);
        if (slice_type == 2) mb_type[m] = r < 3 ? T_I_16x16 : T_I_4x4;
        else mb_type[m] = (m < 2 || m > n - 3 || r < 2) ? T_P_SKIP : r == 2 ? T_I_16x16 : r == 3 ? T_P_8x8 : T_P_L0;
        if (variant == 1 && slice_type == 0) mb_type[m] = T_P_SKIP;                     // a slice that is one skip run and the trailing bits
        for (int k = 0; k < 16; k++) i4mode[m * 16 + k] = (signed char)rnd(9);
        i16mode[m] = (signed char)rnd(4); chroma_mode[m] = (signed char)rnd(4);
        const bool skip = mb_type[m] == T_P_SKIP, is16 = mb_type[m] == T_I_16x16;
        cbp[m] = skip ? 0 : (i16)((is16 ? (rnd(2) ? 15 : 0) : rnd(16)) | rnd(3) << 4);
        if (mb_type[m] == T_P_L0) partition[m] = (signed char)(D_16x8 + rnd(3));
        if (mb_type[m] == T_P_8x8) { partition[m] = D_8x8; for (int k = 0; k < 4; k++) sub[m * 4 + k] = (signed char)rnd(4); }
        if (mb_type[m] >= T_P_L0 && !skip) for (int k = 0; k < 32; k++) mv[m * 32 + k] = (i16)(rnd(64) - 32);
        if (!skip) {
            for (int k = 0; k < 256; k++) if (cbp[m] >> (k >> 6) & 1) luma[m * 256 + k] = (i16)(rnd(3) ? 0 : rnd(2) ? rnd(7) - 3 : rnd(4001) - 2000);
            if (is16) for (int k = 0; k < 16; k++) luma_dc[m * 16 + k] = (i16)(rnd(41) - 20);
            if (cbp[m] >> 4) for (int k = 0; k < 8; k++) chroma_dc[m * 8 + k] = (i16)(rnd(9) - 4);
            if (cbp[m] >> 5) for (int k = 0; k < 128; k++) chroma_ac[m * 128 + k] = (i16)(rnd(4) ? 0 : rnd(5) - 2);
        }
        // the state's convention: a macroblock without coefficients carries the QP before it
        if (!skip && (is16 || cbp[m])) { if (is16 && !cbp[m]) { /* an empty I_16x16 keeps the QP before it */ } else last_qp = 20 + rnd(20); }
        qp[m] = (signed char)last_qp;
    }
    x264hip_mb_state st;
    memset(&st, 0, sizeof(st));
    st.mb_type = (decltype(st.mb_type))mb_type.data(); st.partition = (decltype(st.partition))partition.data();
    st.sub_partition = (decltype(st.sub_partition))sub.data(); st.ref = (decltype(st.ref))ref.data(); st.ref1 = (decltype(st.ref1))ref1.data();
    st.i4mode = (decltype(st.i4mode))i4mode.data(); st.i16mode = (decltype(st.i16mode))i16mode.data();
    st.chroma_mode = (decltype(st.chroma_mode))chroma_mode.data(); st.t8 = (decltype(st.t8))t8.data(); st.qp = (decltype(st.qp))qp.data();
    st.mv = mv.data(); st.mv1 = mv1.data(); st.cbp = cbp.data(); st.luma = luma.data(); st.luma_dc = luma_dc.data(); st.chroma_dc = chroma_dc.data();
    st.chroma_ac = chroma_ac.data();
    const int cap = 64 + margin + n * 1200 + 3;                       // (odd on purpose: the slot's end is no multiple of 4)
    std::vector<u8> pay[2] = {std::vector<u8>(cap, 0x5A), std::vector<u8>(cap, 0xC3)};
    std::vector<int> bits[2] = {std::vector<int>(n, -1), std::vector<int>(n, -1)};
    int len[2] = {-1, -1}, rc[2];
    for (int k = 0; k < 2; k++) {
        x264hip_cavlc_params p;
        memset(&p, 0, sizeof(p));
        p.slice_type = slice_type; p.n_ref0 = 1; p.analyse_inter = 0x33; p.payload = pay[k].data(); p.payload_cap = cap; p.payload_len = &len[k];
        p.mb_bits = bits[k].data(); p.slice_qp = 30;
        rc[k] = k ? cavlc_mp_host_write_slice(&st, &p, W, H, margin) : cavlc_mp_host_write_slice_serial(&st, &p, W, H, margin);
    }
    int bad = rc[0] != 0 || rc[1] != 0 || len[0] != len[1] || len[0] <= 0 || bits[0] != bits[1] || memcmp(pay[0].data() + 64, pay[1].data() + 64, (size_t)len[0]);
    for (int k = 0; k < 64; k++) bad |= pay[1][k] != 0xC3;                                         // the lead bytes
    for (int k = 64 + len[1]; k < cap; k++) bad |= pay[1][k] != 0xC3;                             // and everything behind the slice
    printf("slice type %d variant %d: serial %d bytes (rc %d), count/scan/place %d bytes (rc %d): %s\n", slice_type, variant, len[0], rc[0], len[1], rc[1],
           bad ? "DIFFERENT" : "equal");
    return bad;
}

int main()
{
    int bad = 0;
    for (int round = 0; round < 20; round++) bad |= run_case(2, 0) | run_case(0, 0);
    bad |= run_case(0, 1);
    return bad;
}
#endif
