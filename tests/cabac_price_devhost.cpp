// cabac_price_devhost.cpp -- the devhost_* entry points of oracle/devcheck.cpp with ONE difference: a bit count of a whole macroblock
// (devhost_cw_macroblock, rd = 1) runs the RD trials' pricing of x264_vs2008_amd/csrc/cabac_price.h -- residual blocks walked from
// ballot-built masks (a loop over 64 lanes stands for the ballot).  Everything else forwards to the old text.
// tests/test_cabac_price_chain_host.py links it with the CPU twin built with -DX264O_DEVCHECK, which replays every call it makes while it
// encodes a chain and compares count, states and record.
#define X264HIP_HOST_TEST 1
#include "cabac_price.h"
#include "trellis_dev.h"

extern "C" void devhost_context_init(uint8_t *st, int slice_type, int qp, int model)
{
    for (int i = 0; i < 460; i++) st[i] = (uint8_t)cd_context_init_one(i, slice_type, qp, model);
}
extern "C" void devhost_cw_macroblock(DCabac *cb, uint8_t *st, int rd, MbSyn *m, const uint8_t *fe, int i_frame)
{
    if (!rd) { cw_macroblock(*cb, st, rd, *m, fe, i_frame); return; }
    const MbSyn &y = *m;
    const CpMasks k = cp_masks([&](int q) -> cp_u64 { cp_u64 w = 0; for (int lane = 0; lane < 64; lane++) if (cp_mask_lane(y, q, lane)) w |= 1ull << lane; return w; });
    cp_macroblock(*cb, st, *m, k);
}
extern "C" void devhost_mb_skip(DCabac *cb, uint8_t *st, int type_left, int type_top, int b_skip) { cw_mb_skip(*cb, st, type_left, type_top, b_skip); }
extern "C" void devhost_terminal(DCabac *cb) { cd_encode_terminal(*cb); }
extern "C" void devhost_flush(DCabac *cb, int i_frame) { cd_encode_flush(*cb, i_frame); }
extern "C" int devhost_trellis(int16_t *dct, const uint16_t *mf, const int *unq, const int *weight, const uint8_t *zz, const uint8_t *st,
                               int cat, int lambda2, int b_ac, int dc, int n_coef)
{
    TrellisScratch ts;
    return td_trellis_quant(ts, dct, mf, unq, weight, zz, st, cat, lambda2, b_ac, dc, n_coef);
}
extern "C" void devhost_cw_part(DCabac *cb, uint8_t *st, MbSyn *m, int kind, int a, int b)
{
    if (kind == 0) cw_partition_size(*cb, st, *m, a, b);
    else if (kind == 1) cw_subpartition_size(*cb, st, *m, a, b);
    else if (kind == 2) cw_partition_i8x8_size(*cb, st, *m, a, b);
    else if (kind == 3) cw_partition_i4x4_size(*cb, st, *m, a, b);
    else cw_i8x8_chroma_size(*cb, st, *m);
}
