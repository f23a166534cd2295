// cabac_pass_host.cpp -- the CABAC pass of the product (x264_vs2008_amd/csrc/cabac_pass_dev.h over mb_vocab.h, mbsyn.h and cabac_dev.h)
// compiled for the host alone, with g++ and no HIP: tests/cabac_pass_host_util.py builds it and tests/test_cabac_pass_host.py feeds it one
// frame's state arrays and compares the slice's bytes and the bit position after every macroblock with the reference's.  The arguments are
// the ABI's: an x264hip_mb_state of one chain whose pointers are host arrays, and the x264hip_cabac_params of the slice (payload: one slot
// of payload_cap bytes, payload_len: one int, mb_bits: one int per macroblock).
//
// With -DCABAC_PASS_HOST_MAIN the file is a program of its own (for a sanitizer build: -fsanitize=address,undefined): it reads one frame from
// a file -- 16 int32 (magic 0x43504153, mb_w, mb_h, slice_type, n_ref0, analyse_inter, transform8x8, slice_qp, cabac_init_idc, i_frame, the
// expected length, 5 x 0), then the arrays mb_type partition sub_partition ref i4mode i16mode chroma_mode qp t8 (int8) nnz (uint8) mv cbp luma
// luma_dc chroma_dc chroma_ac (int16) in the state's shapes, each padded to 4 bytes, then the expected bytes -- writes the slice into a heap
// slot of the smallest size the entry point takes plus the expected length, and compares.
#define X264HIP_HOST_TEST 1
#include "cabac_pass_dev.h"

// Writes the slice.  Returns 0 and the length in p->payload_len[0] (the bytes start X264HIP_PAYLOAD_LEAD into the slot), 1 when the pass
// stopped (length 0: a slot too small, a macroblock type the slice cannot hold), -1 for what the entry point refuses.
extern "C" int cabac_pass_host_write_slice(const x264hip_mb_state *st, const x264hip_cabac_params *p, int mb_w, int mb_h)
{
    if (mb_w > CP_MAX_W || p->slice_type == 1 || !st->luma || !p->payload || !p->payload_len || p->payload_cap < CP_MB_BYTES_MAX + 128) return -1;
    CpWork *w = new CpWork;
    CpArgs a;
    int aborted = 0, total = 0;
    memset(w, 0xAA, sizeof(*w));             // LDS starts with whatever it held: the pass must not read what it has not written
    cp_args(a, st, p, mb_w, mb_h, &aborted, &total);
    cp_write_slice(a, 0, w);
    delete w;
    return aborted;
}

#ifdef CABAC_PASS_HOST_MAIN
#include <stdio.h>
#include <vector>
int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s frame.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t h[16];
    if (fread(h, 4, 16, f) != 16 || h[0] != 0x43504153) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t n = (size_t)h[1] * h[2];
    const size_t per_mb[16] = {1, 1, 4, 4, 16, 1, 1, 1, 1, 27, 64, 2, 512, 32, 16, 256};     // bytes per macroblock, in the file's order
    std::vector<std::vector<uint8_t>> arr(16);
    for (int i = 0; i < 16; i++) {
        arr[i].resize((n * per_mb[i] + 3) & ~(size_t)3);
        if (fread(arr[i].data(), 1, arr[i].size(), f) != arr[i].size()) { fprintf(stderr, "short file\n"); return 2; }
    }
    std::vector<uint8_t> want((size_t)h[10]);
    if (fread(want.data(), 1, want.size(), f) != want.size()) { fprintf(stderr, "short file\n"); return 2; }
    fclose(f);
    x264hip_mb_state st;
    memset(&st, 0, sizeof(st));
    st.mb_type = (int8_t *)arr[0].data(); st.partition = (int8_t *)arr[1].data(); st.sub_partition = (int8_t *)arr[2].data(); st.ref = (int8_t *)arr[3].data();
    st.i4mode = (int8_t *)arr[4].data(); st.i16mode = (int8_t *)arr[5].data(); st.chroma_mode = (int8_t *)arr[6].data(); st.qp = (int8_t *)arr[7].data();
    st.t8 = (int8_t *)arr[8].data(); st.nnz = arr[9].data(); st.mv = (int16_t *)arr[10].data(); st.cbp = (int16_t *)arr[11].data();
    st.luma = (int16_t *)arr[12].data(); st.luma_dc = (int16_t *)arr[13].data(); st.chroma_dc = (int16_t *)arr[14].data(); st.chroma_ac = (int16_t *)arr[15].data();
    const int cap = CP_MB_BYTES_MAX + 128 + X264HIP_PAYLOAD_LEAD + h[10];
    std::vector<uint8_t> slot((size_t)cap);
    std::vector<int32_t> bits(n);
    int32_t len = 0;
    x264hip_cabac_params p;
    memset(&p, 0, sizeof(p));
    p.slice_type = h[3]; p.n_ref0 = h[4]; p.analyse_inter = h[5]; p.transform8x8 = h[6]; p.slice_qp = h[7]; p.cabac_init_idc = h[8]; p.i_frame = h[9];
    p.payload = slot.data(); p.payload_cap = cap; p.payload_len = &len; p.mb_bits = bits.data();
    const int rc = cabac_pass_host_write_slice(&st, &p, h[1], h[2]);
    const bool same = rc == 0 && len == h[10] && !memcmp(slot.data() + X264HIP_PAYLOAD_LEAD, want.data(), want.size());
    printf("%dx%d macroblocks, slice type %d: rc %d, %d bytes (expected %d), %s\n", h[1], h[2], h[3], rc, len, h[10], same ? "equal" : "DIFFERENT");
    return same ? 0 : 1;
}
#endif
