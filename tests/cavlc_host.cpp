// cavlc_host.cpp -- the CAVLC slice writer of the product (x264_vs2008_amd/csrc/cavlc_dev.h over mb_vocab.h) compiled for the host
// alone, with g++ and no HIP: tests/cavlc_host_util.py builds it and tests/test_cavlc_host.py feeds it one frame's state arrays and
// compares the slice's bytes with the reference's.  The arguments are the ABI's: an x264hip_mb_state of one chain whose pointers are
// host arrays, and the x264hip_cavlc_params of the slice (payload: one slot of payload_cap bytes, payload_len: one int).
#define X264HIP_HOST_TEST 1
#include "cavlc_dev.h"

// Writes the slice; margin as the kernels' (the bytes kept free behind the macroblock about to be written).  Returns 0 and the
// length in p->payload_len[0] (the bytes start X264HIP_PAYLOAD_LEAD into the slot), 1 when the writer stopped (length 0), -1 for a
// frame wider than the writer's row buffer.
extern "C" int cavlc_host_write_slice(const x264hip_mb_state *st, const x264hip_cavlc_params *p, int mb_w, int mb_h, int margin)
{
    if (mb_w > CV_MAX_W) return -1;
    CvWork w;
    CvArgs a;
    int aborted = 0;
    memset(&w, 0xAA, sizeof(w));             // LDS starts with whatever it held: the writer must not read what it has not written
    cv_args(a, st, p, mb_w, mb_h, &aborted, margin);
    cv_write_slice(a, 0, &w);
    return aborted;
}
