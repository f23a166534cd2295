// look_cost_body.h -- the body of the lookahead's cost kernels (frame_lookahead_cost.hip: k_look_cost, k_look_cost_sad), textually included
// with the kernel's parameters and the constant SAD (mbcmp: false SATD, true SAD) in scope.
    __shared__ u32 s_fe[16 * 4];                              // the source block in the macroblock layout the search reads (16-byte rows)
    __shared__ i16 s_costl[2 * MX_COST_LDS + 2];
    __shared__ u32 s_row[2][2][LK_MAX_W];                     // [list][row parity][mb x]: the vectors of this row and the one below
    __shared__ i16 s_mvc[8];
    const int lane = threadIdx.x;
    const LookTaskDev T = tasks[blockIdx.x];
    const int d0 = T.d0, d1 = T.d1, b_bidir = d1 > 0, intra_only = d0 == 0 && d1 == 0;
    int dist_scale_factor = 128;
    if (d0 + d1 != 0) dist_scale_factor = ((d0 << 8) + ((d0 + d1) >> 1)) / (d0 + d1);
    const int bipred_weight = weighted_bipred ? 64 - (dist_scale_factor >> 2) : 32;
    for (int i = lane; i < 2 * MX_COST_LDS + 1; i += 64) s_costl[i] = cost_g[i - MX_COST_LDS];
    for (int i = lane; i < 2 * 2 * LK_MAX_W; i += 64) (&s_row[0][0][0])[i] = 0;
    LK_SYNC();
    int score = 0, intra_mbs = 0, cost00 = 0;
    const int px = lane & 7, py = lane >> 3;
    for (int my = mb_h - 2; my > 0; my--)
        for (int mx = mb_w - 2; mx > 0; mx--) {
            const int xy = mx + my * mb_w;
            const ptrdiff_t off = 8 * ((ptrdiff_t)mx + (ptrdiff_t)my * stride);
            int bcost = LK_COST_MAX;
            if (!intra_only) {
                LK_SYNC();                                    // the previous block's readers are done with s_fe / s_mvc
                if (lane < 16) s_fe[(lane >> 1) * 4 + (lane & 1)] = *(const u32 *)(T.pl[0][0] + off + (ptrdiff_t)(lane >> 1) * stride + 4 * (lane & 1));
                LK_SYNC();
                const int fpx = (int)((const u8 *)s_fe)[py * 16 + px];
                MeLimits L;
                L.fmin0 = -8 * mx - 4; L.fmax0 = 8 * (mb_w - mx - 1) + 4; L.fmin1 = -8 * my - 4; L.fmax1 = 8 * (mb_h - my - 1) + 4;
                L.smin0 = 4 * (L.fmin0 - 8); L.smax0 = 4 * (L.fmax0 + 8); L.smin1 = 4 * (L.fmin1 - 8); L.smax1 = 4 * (L.fmax1 + 8);
                const ptrdiff_t poff = off + (ptrdiff_t)py * stride + px;
#define LK_TRY_BIDIR(ax_, ay_, bx_, by_, penalty_) do { \
                    const int r0_ = lk_ref_px(T.pl[1][0], T.pl[1][1], T.pl[1][2], T.pl[1][3], stride, poff, (ax_), (ay_)); \
                    const int r1_ = lk_ref_px(T.pl[2][0], T.pl[2][1], T.pl[2][2], T.pl[2][3], stride, poff, (bx_), (by_)); \
                    const int av_ = bipred_weight == 32 ? (r0_ + r1_ + 1) >> 1 : clip_u8((r0_ * bipred_weight + r1_ * (64 - bipred_weight) + 32) >> 6); \
                    const int c_ = (penalty_) + (SAD ? lk_sad8x8(fpx - av_) : lk_satd8x8(fpx - av_, lane)); \
                    if (bcost > c_) bcost = c_; } while (0)
                if (b_bidir) {
                    const int rx = MX_UNI((int)T.mvr[2 * xy]), ry = MX_UNI((int)T.mvr[2 * xy + 1]);
                    int ax = (rx * dist_scale_factor + 128) >> 8, ay = (ry * dist_scale_factor + 128) >> 8;
                    int bx = ax - rx, by = ay - ry;
                    ax = clip3(ax, L.smin0, L.smax0); ay = clip3(ay, L.smin1, L.smax1);
                    bx = clip3(bx, L.smin0, L.smax0); by = clip3(by, L.smin1, L.smax1);
                    LK_TRY_BIDIR(ax, ay, bx, by, 0);
                    if (ax | ay | bx | by) LK_TRY_BIDIR(0, 0, 0, 0, 0);
                }
                int mvx[2] = {0, 0}, mvy[2] = {0, 0};
                for (int l = 0; l < 1 + b_bidir; l++) {
                    int cost, vx, vy;
                    // (selects, not T.x[l]: a dynamically indexed member would put the whole task record into private memory)
                    i16 *const mv_l = l ? T.mv[1] : T.mv[0];
                    int *const mcost_l = l ? T.mcost[1] : T.mcost[0];
                    if (l ? T.do_search[1] : T.do_search[0]) {
                        // reverse-order predictors, slicetype.c:151-163: right, below, below-left, below-right (zero where absent)
                        const u32 *rc = s_row[l][my & 1], *rb = s_row[l][(my + 1) & 1];     // (LDS: indexing is free)
                        u32 cand[4] = {0, 0, 0, 0};
                        int n_mvc = 0;
                        if (mx < mb_w - 1) cand[n_mvc++] = rc[mx + 1];
                        if (my < mb_h - 1) {
                            cand[n_mvc++] = rb[mx];
                            if (mx > 0) cand[n_mvc++] = rb[mx - 1];
                            if (mx < mb_w - 1) cand[n_mvc++] = rb[mx + 1];
                        }
                        int cx[4], cy[4];
#pragma unroll
                        for (int k = 0; k < 4; k++) { cx[k] = MX_UNI((int)(i16)(cand[k] & 0xffff)); cy[k] = MX_UNI((int)(i16)(cand[k] >> 16)); }
                        const int mvpx = max(min(cx[0], cx[1]), min(max(cx[0], cx[1]), cx[2]));     // x264_median_mv of the first three
                        const int mvpy = max(min(cy[0], cy[1]), min(max(cy[0], cy[1]), cy[2]));
                        if (lane < 4) { s_mvc[2 * lane] = (i16)cx[lane == 0 ? 0 : lane == 1 ? 1 : lane == 2 ? 2 : 3]; s_mvc[2 * lane + 1] = (i16)cy[lane == 0 ? 0 : lane == 1 ? 1 : lane == 2 ? 2 : 3]; }
                        LK_SYNC();
                        MxCtx c;
                        c.fe = (MX_LDS(u32))s_fe; c.fe_u = (MX_LDS(u8))s_fe; c.fe_v = (MX_LDS(u8))s_fe;
                        c.pl[0] = (MX_GLB(u8))((l ? T.pl[2][0] : T.pl[1][0]) + off); c.pl[1] = (MX_GLB(u8))((l ? T.pl[2][1] : T.pl[1][1]) + off);
                        c.pl[2] = (MX_GLB(u8))((l ? T.pl[2][2] : T.pl[1][2]) + off); c.pl[3] = (MX_GLB(u8))((l ? T.pl[2][3] : T.pl[1][3]) + off);
                        c.cu = c.pl[0]; c.cv = c.pl[0];
                        c.cost_g = (MX_GLB(i16))cost_g; c.cost_l = (MX_LDS(i16))s_costl; c.has_cost_l = true;
                        c.patch = (MX_LDS(u8))s_fe; c.has_patch = false; c.patch_on = false;
                        c.px0 = c.py0 = c.cx0 = c.cy0 = 0;
                        c.mvpx = mvpx; c.mvpy = mvpy; c.sy = stride; c.sc = stride; c.lane = lane;
                        c.set_block(8, 8, 0, 0);
                        MeOpts o;
                        o.method = method; o.me_range = me_range; o.subme = 4; o.chroma_me = 0; o.sad_only = SAD;
                        int cmv;
                        cost = me_search_ref16(c, L, o, s_mvc, n_mvc, nullptr, vx, vy, cmv);
                        cost -= 2;                            // remove mvcost from skip mbs
                        if (vx | vy) cost += 5;
                        LK_SYNC();                            // s_mvc read; the row entry below is this block's own
                        if (lane == 0) {
                            s_row[l][my & 1][mx] = (u32)(u16)vx | ((u32)(u16)vy << 16);
                            *(u32 *)(mv_l + 2 * xy) = (u32)(u16)vx | ((u32)(u16)vy << 16);
                            mcost_l[xy] = cost;
                        }
                    } else {
                        vx = MX_UNI((int)mv_l[2 * xy]); vy = MX_UNI((int)mv_l[2 * xy + 1]); cost = MX_UNI(mcost_l[xy]);
                    }
                    if (l) { mvx[1] = vx; mvy[1] = vy; } else { mvx[0] = vx; mvy[0] = vy; }
                    bcost = min(bcost, cost);
                }
                if (b_bidir && (mvx[0] | mvy[0] | mvx[1] | mvy[1])) LK_TRY_BIDIR(mvx[0], mvy[0], mvx[1], mvy[1], 5);
            }
            if (!b_bidir) {                                   // no intra blocks in B frames
                const int icost = MX_UNI(T.intra[xy]);
                const int b_intra = icost < bcost;
                if (b_intra) bcost = icost;
                intra_mbs += b_intra; cost00 += icost;
            }
            score += bcost;
        }
    if (d1 != 0) score = score * 100 / (120 + bframe_bias);
    if (lane == 0) { out[4 * blockIdx.x] = score; out[4 * blockIdx.x + 1] = intra_mbs; out[4 * blockIdx.x + 2] = cost00; out[4 * blockIdx.x + 3] = 0; }
