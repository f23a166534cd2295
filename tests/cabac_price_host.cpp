// cabac_price_host.cpp -- the RD trials' bit count of the product (x264_vs2008_amd/csrc/cabac_price.h over cabac_dev.h) compiled for the host
// alone, with g++ and no HIP, a loop over 64 lanes standing for the wave's ballot: tests/test_cabac_price_host.py builds it and holds it to
// cw_macroblock(rd = 1) over random syntax records -- the count f8, all 460 states and the record afterwards -- and the ballot-built masks
// to a plain loop over the coefficient arrays.
//
// With -DCABAC_PRICE_HOST_MAIN the file is a program of its own (for a sanitizer build: -fsanitize=address,undefined): it runs the same
// records for the three slice types and exits 0 when nothing differed.
#define X264HIP_HOST_TEST 1
#include "cabac_price.h"

namespace {
struct Rng {
    uint64_t s;
    uint32_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
    int range(int lo, int hi) { return lo + below(hi - lo + 1); }
    bool one_in(int n) { return below(n) == 0; }
};

// stats: [0..18] records per macroblock type, [32..44] 8x8 blocks per sub-partition, [64 + 8 * cat + cls] blocks per level pattern,
// [128..133] levels of magnitude 1, 2, 14, 15, 16, 2000, [140] records whose nnz / cbp disagree with the levels, [141] blocks the masks were
// checked on, [142] records with t8, [143] records with n_ref 3
enum { N_STATS = 160 };

int rnd_level(Rng &r, long long *stats)
{
    static const int mags[6] = {1, 2, 14, 15, 16, 2000};
    int a;
    if (r.one_in(2)) { const int k = r.below(6); a = mags[k]; stats[128 + k]++; }
    else a = r.one_in(4) ? r.range(1, 40) : r.range(1, 3);
    return r.one_in(2) ? -a : a;
}
// fills l[0..n): 0 all zero, 1 one coefficient at the first position, 2 one at the last, 3 full, 4 runs of zeros between coefficients, 5 random
void fill_block(Rng &r, int16_t *l, int n, int cat, long long *stats)
{
    const int cls = r.below(6);
    stats[64 + 8 * cat + cls]++;
    for (int i = 0; i < n; i++) l[i] = 0;
    if (cls == 1) l[0] = (int16_t)rnd_level(r, stats);
    else if (cls == 2) l[n - 1] = (int16_t)rnd_level(r, stats);
    else if (cls == 3) for (int i = 0; i < n; i++) l[i] = (int16_t)rnd_level(r, stats);
    else if (cls == 4) for (int i = r.below(3); i < n; i += r.range(2, n > 16 ? 20 : 6)) l[i] = (int16_t)rnd_level(r, stats);
    else if (cls == 5) { const int d = r.range(2, 8); for (int i = 0; i < n; i++) if (r.one_in(d)) l[i] = (int16_t)rnd_level(r, stats); }
}
bool any(const int16_t *l, int n) { for (int i = 0; i < n; i++) if (l[i]) return true; return false; }

void make_record(Rng &r, MbSyn &m, int slice_type, long long *stats)
{
    memset(&m, 0, sizeof(m));
    m.slice_type = slice_type;
    static const int itypes[4] = {T_I_4x4, T_I_8x8, T_I_16x16, T_I_PCM};
    const int pick = r.below(slice_type == 2 ? 4 : slice_type == 0 ? 10 : 24);
    m.partition = D_16x16;
    if (pick < 4) m.type = itypes[pick];
    else if (slice_type == 0) {
        if (pick < 7) { m.type = T_P_L0; m.partition = pick == 4 ? D_16x16 : pick == 5 ? D_16x8 : D_8x16; }
        else { m.type = T_P_8x8; m.partition = D_8x8; }
    } else {
        if (pick == 4) m.type = T_B_DIRECT;
        else if (pick < 8) { m.type = T_B_8x8; m.partition = D_8x8; }
        else if (pick < 11) m.type = pick == 8 ? T_B_L0_L0 : pick == 9 ? T_B_L1_L1 : T_B_BI_BI;          // the three 16x16 forms
        else { m.type = T_B_L0_L0 + r.below(9); m.partition = r.one_in(2) ? D_16x8 : D_8x16; }
    }
    stats[m.type]++;
    for (int i = 0; i < 4; i++) {
        static const int bsub[4] = {D_L0_8x8, D_L1_8x8, D_BI_8x8, D_DIRECT_8x8};
        m.sub[i] = (signed char)(slice_type == 1 ? bsub[r.below(4)] : r.below(4));
        if (m.type == T_P_8x8 || m.type == T_B_8x8) stats[32 + m.sub[i]]++;
    }
    m.i16mode = r.below(7); m.chroma_mode = r.below(7);
    m.pps_t8 = r.below(2); m.t8 = m.pps_t8 && r.below(2); m.t8_allowed = m.pps_t8 && m.type > T_I_PCM && r.below(4) != 0;
    if (m.type == T_I_8x8) m.t8 = r.below(8) != 0;
    if (m.type == T_I_16x16 && !r.one_in(16)) m.t8 = 0;
    stats[142] += m.t8;
    m.qp = r.below(52); m.last_qp = r.one_in(3) ? m.qp : r.below(52);
    m.n_ref = r.one_in(2) ? 1 : 3; m.n_ref1 = r.one_in(2) ? 1 : 2;
    stats[143] += m.n_ref == 3;
    m.type_left = r.range(-1, 18); m.type_top = r.range(-1, 18);
    m.cbp_left = r.one_in(6) ? -1 : (r.below(16) | (r.below(3) << 4) | (r.below(8) << 8));
    m.cbp_top = r.one_in(6) ? -1 : (r.below(16) | (r.below(3) << 4) | (r.below(8) << 8));
    m.cpm_left = r.below(4); m.cpm_top = r.below(4); m.nb_t8 = r.below(3);
    m.last_dqp = r.one_in(2) ? 0 : r.range(-6, 6); m.prev_coded = r.below(2);
    for (int i = 0; i < 48; i++) {
        m.i4c[i] = (signed char)r.range(-1, 11);
        m.cref[i] = (signed char)r.range(-2, m.n_ref - 1); m.cref1[i] = (signed char)r.range(-2, m.n_ref1 - 1);
        m.cskip[i] = (signed char)r.below(2);
        for (int c = 0; c < 2; c++) {
            const int big = r.one_in(8);
            m.cmv[i][c] = (int16_t)(big ? r.range(-2000, 2000) : r.range(-12, 12)); m.cmv1[i][c] = (int16_t)(big ? r.range(-2000, 2000) : r.range(-12, 12));
            m.cmvd[i][c] = (int16_t)(r.one_in(4) ? r.range(-70, 70) : r.range(-2, 2)); m.cmvd1[i][c] = (int16_t)(r.one_in(4) ? r.range(-70, 70) : r.range(-2, 2));
        }
    }
    for (int i = 0; i < 4; i++) { m.nz_l[i] = (uint8_t)(r.one_in(5) ? 0x80 : r.below(3)); m.nz_t[i] = (uint8_t)(r.one_in(5) ? 0x80 : r.below(3)); }
    for (int i = 0; i < 4; i++) { m.nz_lc[i >> 1][i & 1] = (uint8_t)(r.one_in(5) ? 0x80 : r.below(3)); m.nz_tc[i >> 1][i & 1] = (uint8_t)(r.one_in(5) ? 0x80 : r.below(3)); }
    // the levels.  What the count never reads is 0xAA: the luma array of the other transform, the first entry of an AC block
    const int use8 = cp_luma8(m);
    memset(m.lv4, 0xAA, sizeof(m.lv4)); memset(m.lv8, 0xAA, sizeof(m.lv8)); memset(m.lv_cac, 0xAA, sizeof(m.lv_cac));
    int cbp = 0;
    if (use8) {
        for (int i = 0; i < 4; i++) { fill_block(r, m.lv8[i], 64, 5, stats); if (any(m.lv8[i], 64)) cbp |= 1 << i; for (int k = 0; k < 4; k++) m.nnz[4 * i + k] = (uint8_t)r.below(3); }
    } else {
        const int ac = m.type == T_I_16x16;
        for (int i = 0; i < 16; i++) {
            fill_block(r, m.lv4[i] + ac, 16 - ac, ac ? 1 : 2, stats);
            m.nnz[i] = any(m.lv4[i] + ac, 16 - ac);
            if (m.nnz[i]) cbp |= 1 << (i >> 2);
        }
    }
    fill_block(r, m.lv_dc, 16, 0, stats); m.nnz[24] = any(m.lv_dc, 16);
    int cdc = 0, cac = 0;
    for (int c = 0; c < 2; c++) { fill_block(r, m.lv_cdc[c], 4, 3, stats); m.nnz[25 + c] = any(m.lv_cdc[c], 4); cdc |= m.nnz[25 + c]; }
    for (int i = 0; i < 8; i++) { fill_block(r, m.lv_cac[i] + 1, 15, 4, stats); m.nnz[16 + i] = any(m.lv_cac[i] + 1, 15); cac |= m.nnz[16 + i]; }
    m.cbp_luma = cbp; m.cbp_chroma = cac ? 2 : cdc ? 1 : 0;
    if (m.type == T_I_16x16 && cbp) m.cbp_luma = 15;
    if (r.one_in(4)) {          // counts and coded-block patterns that disagree with the levels, both ways: the walk follows cbp and nnz
        stats[140]++;
        for (int i = 0; i < 27; i++) if (r.one_in(3)) m.nnz[i] = (uint8_t)(m.nnz[i] ? 0 : 1 + r.below(2));
        if (r.one_in(2)) m.cbp_luma = r.below(16);
        if (r.one_in(2)) m.cbp_chroma = r.below(3);
    }
}

cp_u64 plain_mask(const int16_t *l, int n) { cp_u64 k = 0; for (int i = 0; i < n; i++) if (l[i]) k |= 1ull << i; return k; }
}

// Runs n random records of one slice type through both counts.  Returns the number of records that differ in the count, in a state or in
// the record afterwards, plus the number of blocks whose mask differs from a plain loop's (0: all equal); -1: bad arguments.
extern "C" int cabac_price_host_run(int slice_type, int n, unsigned seed, long long *stats)
{
    if (slice_type < 0 || slice_type > 2 || n < 0 || !stats) return -1;
    Rng r = {0x9E3779B97F4A7C15ull ^ ((uint64_t)seed << 20) ^ (uint64_t)slice_type};
    for (int i = 0; i < 8; i++) r.next();
    memset(stats, 0, N_STATS * sizeof(*stats));
    int bad = 0;
    MbSyn *ma = new MbSyn, *mb = new MbSyn;
    for (int rec = 0; rec < n; rec++) {
        make_record(r, *ma, slice_type, stats);
        *mb = *ma;
        uint8_t st_a[460], st_b[460];
        for (int i = 0; i < 460; i++) st_a[i] = st_b[i] = (uint8_t)r.below(128);
        // the old text
        DCabac ca = {0, 0x1FE, -1, 0, nullptr, 0}, cb = ca;
        cw_macroblock(ca, st_a, 1, *ma, (const uint8_t *)nullptr, 0);
        // the new: the masks as the wave ballots them (a loop over the 64 lanes), then the walk
        const MbSyn &y = *mb;
        const CpMasks k = cp_masks([&](int q) -> cp_u64 { cp_u64 w = 0; for (int lane = 0; lane < 64; lane++) if (cp_mask_lane(y, q, lane)) w |= 1ull << lane; return w; });
        cp_macroblock(cb, st_b, *mb, k);
        const int differ = ca.f8 != cb.f8 || memcmp(ma, mb, sizeof(MbSyn)) != 0 || memcmp(st_a, st_b, 460) != 0;
        bad += differ;
        // the masks against a plain loop, block by block
        const int use8 = cp_luma8(y), ac = y.type == T_I_16x16;
        if (use8) for (int i = 0; i < 4; i++) bad += cp_block_mask(k, 5, 4 * i) != plain_mask(y.lv8[i], 64);
        else for (int i = 0; i < 16; i++) bad += cp_block_mask(k, ac ? 1 : 2, i) != plain_mask(y.lv4[i] + ac, 16 - ac);
        bad += cp_block_mask(k, 0, 24) != plain_mask(y.lv_dc, 16);
        for (int c = 0; c < 2; c++) bad += cp_block_mask(k, 3, 25 + c) != plain_mask(y.lv_cdc[c], 4);
        for (int i = 0; i < 8; i++) bad += cp_block_mask(k, 4, 16 + i) != plain_mask(y.lv_cac[i] + 1, 15);
        stats[141] += (use8 ? 4 : 16) + 11;
    }
    delete ma; delete mb;
    return bad;
}

#ifdef CABAC_PRICE_HOST_MAIN
#include <stdio.h>
int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 20000;
    int rc = 0;
    for (int t = 0; t < 3; t++) {
        long long stats[N_STATS];
        const int bad = cabac_price_host_run(t, n, 1u, stats);
        printf("slice type %d: %d records, %lld blocks' masks checked, %d differ\n", t, n, stats[141], bad);
        rc |= bad != 0;
    }
    return rc;
}
#endif
