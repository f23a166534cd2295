// slice_sweep_body.h -- the body of the macroblock sweep, textually included by the kernel templates at the end of slice_kernel.h
// (k_slice_sweep, k_lossless_raster and k_psy_raster).  In scope: the kernel's parameters (SwArgs a, SwRefs refs_k, SwRd rd_k, const SwDesc *tab) and the
// compile-time constants LL, RD, BS, TD, RF, CH, PT described there.
    static_assert(!CH || RD, "the chain table belongs to the raster variant");
    // SUB8: the kernels that code sub-8x8 P partitions under the RD levels (X264_ANALYSE_PSUB8x8 with subme 6-9) and keep the macroblock's own
    // non_zero_count / mvd cache entries from macroblock to macroblock and frame to frame (x264hip_slice_rd.mb_carry): the lossy refinement kernels
    constexpr bool SUB8 = RF && !LL;
    SwRd rd_l;
    if constexpr (CH) {
        typedef const __attribute__((address_space(4))) SwDesc *desc_p;
        const desc_p d = (desc_p)(uintptr_t)tab + blockIdx.x;
        typedef const __attribute__((address_space(4))) u32 *word_p;
        static_assert(sizeof(SwArgs) % 4 == 0 && sizeof(SwRd) % 4 == 0 && alignof(SwDesc) >= 4, "copied by dwords");
        const word_p wa = (word_p)&d->a, wr = (word_p)&d->r;
#pragma unroll
        for (unsigned i = 0; i < sizeof(SwArgs) / 4; i++) ((u32 *)&a)[i] = wa[i];
#pragma unroll
        for (unsigned i = 0; i < sizeof(SwRd) / 4; i++) ((u32 *)&rd_l)[i] = wr[i];
    }
    const SwRd &rd = CH ? rd_l : rd_k;
    const SwRefs &refs = CH ? tab[blockIdx.x].t : refs_k;
    // A step's I / P chains and B chains run side by side, and an I / P chain is the longer of the two (more references, more candidates):
    // where a SIMD holds one of each, the I / P wavefront issues first, so that both kernels end at about the same time instead of
    // the B chains' wave slots idling while the step waits for its P chains.
    if constexpr (CH && !BS) __builtin_amdgcn_s_setprio(3);
    static_assert(!BS || RD, "B slices run in the raster variant");
    static_assert(!TD || BS, "temporal direct prediction is a B-slice matter");
    static_assert(!RF || (RD && !BS), "the RD refinement is built for the raster variant's I / P kernel");
#undef IS_SKIP_T
#define IS_SKIP_T(t) (BS ? ((t) == T_P_SKIP || (t) == T_B_SKIP) : (t) == T_P_SKIP)      /* BS is a template constant: the other kernels keep their single compare */
    __builtin_assume(a.lossless == (int)LL);           // the host launches the matching variant; do not write to `a` (a modified
                                                        // kernel argument is copied to scratch memory whole)
    __shared__ SwLds s;
    __shared__ typename std::conditional<BS, SwLdsRdB, typename std::conditional<RF, SwLdsRdF, typename std::conditional<RD, SwLdsRd, SwLdsNone>::type>::type>::type sr_;
    SwLdsRd &sr = *(SwLdsRd *)&sr_;                     // only touched when RD
    SwLdsB &sb = *(SwLdsB *)((char *)&sr_ + sizeof(SwLdsRd));    // only touched when BS (then sr_ is an SwLdsRdB)
    SwLdsRf &sf = *(SwLdsRf *)((char *)&sr_ + sizeof(SwLdsRd));  // only touched when RF (then sr_ is an SwLdsRdF)
    (void)sf;
    const int lane_id = threadIdx.x, lane = lane_id;
    const int bz = CH ? a.chain : RD ? (int)blockIdx.x : (int)(blockIdx.x % a.batch_pad), mby0 = RD ? 0 : (int)(blockIdx.x / a.batch_pad);
    if (bz >= a.batch) return;
    const size_t nmb = (size_t)a.mb_w * a.mb_h, cb = nmb * bz, by_ = a.bs_y * bz, bc_ = a.bs_c * bz;
    // batch element
    a.fy += by_; a.fu += bc_; a.fv += bc_; a.dy += by_; a.du += bc_; a.dv += bc_;
    // only what every macroblock reads is adjusted here; the arrays that are written once per macroblock are addressed as base + cb
    // at the store (a base straight from the kernel arguments can be re-loaded; an adjusted one occupies two SGPRs for the whole body)
    a.mb_type += nmb * bz; a.ref += 4 * nmb * bz; a.i4mode += 16 * nmb * bz;
    a.mv += 32 * nmb * bz; a.mvr += 2 * SW_MAX_REFS * nmb * bz;
    if (a.l0_type) { a.l0_type += nmb * bz; a.l0_ref += 4 * nmb * bz; a.l0_mv += 32 * nmb * bz; }
    int *prog = a.progress + (size_t)bz * a.mb_h;

    const int satd = a.subme > 1 && !a.lossless, is_p = a.slice_type == 0;
    const MeOpts mo = {a.me_method, a.me_range, a.subme, a.chroma_me, a.lossless};
    SwQp Q = {a.qp, a.qpc, a.lambda, d_lambda2_tab[a.qp], a.chroma_skip_thresh};
    const i16 *cost_g = a.cost_mv + a.cost_center;     // p_cost_mv of the current QP, centred
    // tables of the current QP: into LDS (once per slice; again whenever adaptive quantisation changes the macroblock's QP)
    auto load_qp_tables = [&](int lane) {
        const int cat = lane >> 4, i = lane & 15, q = cat < 2 ? Q.qp : Q.qpc;
        s.qmf[cat][i] = a.q4mf[(cat * 52 + q) * 16 + i]; s.qbias[cat][i] = a.q4bias[(cat * 52 + q) * 16 + i];
        s.qdq[cat][i] = a.dq4[cat * 96 + (q % 6) * 16 + i];
        if (is_p || BS)
            for (int k = lane; k < 2 * MX_COST_LDS + 1; k += 64) s.costl[k] = cost_g[k - MX_COST_LDS];
        if (a.transform8x8)
            for (int c8 = 0; c8 < 2; c8++) {
                s.q8mf[c8][lane] = a.q8mf[(c8 * 52 + Q.qp) * 64 + lane]; s.q8bias[c8][lane] = a.q8bias[(c8 * 52 + Q.qp) * 64 + lane];
                s.q8dq[c8][lane] = a.dq8[c8 * 384 + (Q.qp % 6) * 64 + lane];
            }
        if constexpr (RD) {
            if (rd.trellis) {
                sr.unq4[cat][i] = rd.unq4[(cat * 52 + q) * 16 + i];
                if (a.transform8x8) for (int c8 = 0; c8 < 2; c8++) sr.unq8[c8][lane] = rd.unq8[(c8 * 52 + Q.qp) * 64 + lane];
            }
        }
    };
    load_qp_tables(lane);
    {
        if (a.nr) { s.nr_off8[lane] = a.nr_offset[(size_t)bz * 128 + 64 + lane]; if (lane < 16) s.nr_off4[lane] = a.nr_offset[(size_t)bz * 128 + lane]; }
        if (lane < 48) s.p4lut[lane] = ((const u32 *)&c_plut4)[lane];
        for (int k = lane; k < 192; k += 64) s.p8lut[k] = ((const u32 *)&c_plut8)[k];
    }
    // the entropy coder of this chain's slice (x264_slice_write, R/encoder/encoder.c:1155-1165)
    DCabac cab = {0, 0x1FE, -1, 0, nullptr, 0};
    // h->mb.cache.ref / mv [list][x264_scan8[12]] as the previous macroblock (or frame) left it: x264_macroblock_cache_load never rewrites
    // the cache's inner entries (SwRd::stale; only a B macroblock whose temporal direct prediction fails ever looks at it)
    int st0r = 0, st0x = 0, st0y = 0, st1r = 0, st1x = 0, st1y = 0;
    if constexpr (RD) {
        if (rd.stale) {
            const i16 *sp = rd.stale + (size_t)bz * 8;
            st0r = __builtin_amdgcn_readfirstlane(sp[0]); st0x = __builtin_amdgcn_readfirstlane(sp[1]); st0y = __builtin_amdgcn_readfirstlane(sp[2]);
            st1r = __builtin_amdgcn_readfirstlane(sp[3]); st1x = __builtin_amdgcn_readfirstlane(sp[4]); st1y = __builtin_amdgcn_readfirstlane(sp[5]);
        }
        if constexpr (TD) {         // the B flow keeps it in LDS (slice_b_flow.h)
            if (lane == 30) { sb.stale[0] = (i16)st0r; sb.stale[1] = (i16)st0x; sb.stale[2] = (i16)st0y; sb.stale[3] = (i16)st1r; sb.stale[4] = (i16)st1x; sb.stale[5] = (i16)st1y; }
        }
    }
    u8 *payload0 = nullptr;
    int last_qp = a.qp, last_dqp = 0, prev_coded = 0, intra_before = 0;      // h->mb.i_last_qp / i_last_dqp; the previous macroblock "has coefficients"
    int dscore0 = 0, dscore1 = 0;                                           // h->stat.frame.i_direct_score[temporal / spatial] (--direct auto)
    (void)dscore0; (void)dscore1;
    if constexpr (RD) {
        if (rd.write) {
            payload0 = rd.payload + (size_t)bz * rd.payload_cap + 64;
            cab.p = payload0;
            for (int k = lane; k < 460; k += 64) sr.cabac[k] = (u8)cd_context_init_one(k, a.slice_type, a.qp, rd.cabac_init_idc);
        }
        if (lane < 16) { sr.zero16[lane] = 0; sr.zz4[lane] = d_zz4[lane]; sr.w4z[lane] = d_w4z[lane]; }
        if (lane < 4) sr.zz2[lane] = (u8)lane;
        sr.zz8[lane] = c_scan8[0][lane]; sr.w8z[lane] = sw_w8z(lane);
        cd_load_tables(lane);
    }
    if constexpr (SUB8) {
        // h->mb.cache.non_zero_count / mvd[0] at the macroblock's own blocks as the chain's previous frame left them: x264_macroblock_cache_load
        // rewrites the neighbours' entries only, and a partial trial encode that runs before any full one prices against the leftovers
        // (R/encoder/analyse.c:1976-1977; oracle/slice_oracle.c: carry_nnz / carry_mvd)
        if (rd.mb_carry) {
            const u8 *cp = rd.mb_carry + (size_t)bz * 160;
            if (lane < 32) s.nnz[lane] = cp[lane];
            if (lane < 16) {
                const int k = 12 + (lane & 3) + 8 * (lane >> 2);
                sr.cmvd[k][0] = ((const i16 *)(cp + 32))[2 * lane]; sr.cmvd[k][1] = ((const i16 *)(cp + 32))[2 * lane + 1];
            }
        }
    }
    WAVE_SYNC();

    int nr_acc4 = 0, nr_acc8 = 0, nr_n4 = 0, nr_n8 = 0;      // --nr: this row's additions to nr_residual_sum (lane = coefficient index) / nr_count
    long long pacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ptime = a.prof ? (long long)wall_clock64() : 0;
#define PROF(k_) do { if (a.prof) { long long now_ = (long long)wall_clock64(); pacc[k_] += now_ - ptime; ptime = now_; } } while (0)
  for (int mby = mby0; mby < (RD ? a.mb_h : mby0 + 1); mby++) {
    if constexpr (RD) {
        // this wave's own stores of the row above (pixels, types, vectors ...) must be what its loads see
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    // the left neighbour = this wave's previous macroblock
    int left_type = -1, left_ref = -2, left_mvx = 0, left_mvy = 0, row_intra = 0;
    int left_cbp = -1, left_cpm = 0, left_t8 = 0;          // (RD) h->mb.cbp / chroma_pred_mode / mb_transform_size of the left macroblock
    u32 pre_y;
    u8 pre_u, pre_v;
    {
        const ptrdiff_t oy0 = (ptrdiff_t)16 * mby * a.sy, oc0 = (ptrdiff_t)8 * mby * a.sc;
        pre_y = *(const u32 *)(a.fy + oy0 + (ptrdiff_t)(lane >> 2) * a.sy + (lane & 3) * 4);
        pre_u = a.fu[oc0 + (ptrdiff_t)(lane >> 3) * a.sc + (lane & 7)];
        pre_v = a.fv[oc0 + (ptrdiff_t)(lane >> 3) * a.sc + (lane & 7)];
    }

    for (int mbx = 0; mbx < a.mb_w; mbx++) {
        // The lane id is laundered once per macroblock: otherwise every lane-derived address and index of the body is hoisted
        // out of this loop, and, being live across all of it, spilled to scratch at the top and reloaded at its use (measured:
        // ~160 scratch stores per macroblock).  Recomputing them from the lane id costs a few VALU operations each.
        int lane = lane_id;
#define LAUNDER() asm volatile("" : "+v"(lane))
        LAUNDER();
        const int mb = mby * a.mb_w + mbx;
        // ---- wait for the row above: left-top, top and top-right neighbours finished ----
        if (!RD && mby > 0) {
            const int need = min(mbx + 2, a.mb_w);
            int spins = 0;
            // Poll with relaxed loads: an acquire load invalidates this CU's vector L1 on every poll, for every wave
            // resident on it (measured: +20 % frames/s).  One acquire fence once the count has been seen.
            for (;;) {
                int v = __builtin_amdgcn_readfirstlane(__hip_atomic_load(prog + mby - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                if ((v & 0xffff) >= need) break;
                if (spins < 4) __builtin_amdgcn_s_sleep(16); else __builtin_amdgcn_s_sleep(100);
                int ab = (spins & 15) == 15 ? __builtin_amdgcn_readfirstlane(__hip_atomic_load(a.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : 0;
                if (ab || ++spins > a.spin_limit) {
                    if (lane == 0) { __hip_atomic_store(a.abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); if (!ab) atomicAdd(a.abort_total, 1); }
                    return;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        PROF(0);
        const ptrdiff_t oy = (ptrdiff_t)16 * mby * a.sy + 16 * mbx, oc = (ptrdiff_t)8 * mby * a.sc + 8 * mbx;
        // ---- x264_macroblock_cache_load: pixels ----
        if (mbx > 0) {      // copy_column8: the column to the left is the previous reconstruction's last column
            if (lane < 16) s.fd[FDY + lane * FD - 1] = s.fd[FDY + lane * FD + 15];
            else if (lane < 24) s.fd[FDU + (lane - 16) * FD - 1] = s.fd[FDU + (lane - 16) * FD + 7];
            else if (lane < 32) s.fd[FDV + (lane - 24) * FD - 1] = s.fd[FDV + (lane - 24) * FD + 7];
        }
        {   // source pixels: fetched one macroblock ahead (they depend on nothing), parked in registers meanwhile
            const int r = lane >> 2, x = (lane & 3) * 4;
            *(u32 *)(s.fe + r * 16 + x) = pre_y;
            s.fe[256 + lane] = pre_u;
            s.fe[320 + lane] = pre_v;
        }
        if (mby > 0) {      // the row above, still unfiltered: x = -1 .. w*3/2-1
            if (lane < 25) s.fd[FDY - FD - 1 + lane] = a.dy[oy - a.sy - 1 + lane];
            else if (lane >= 32 && lane < 45) s.fd[FDU - FD - 1 + (lane - 32)] = a.du[oc - a.sc - 1 + (lane - 32)];
            else if (lane >= 48 && lane < 61) s.fd[FDV - FD - 1 + (lane - 48)] = a.dv[oc - a.sc - 1 + (lane - 48)];
        }
        if (mbx + 1 < a.mb_w) {     // issued after the loads above so that waiting for those leaves these in flight
            const int r = lane >> 2, x = (lane & 3) * 4, cx = lane & 7, cy = lane >> 3;
            pre_y = *(const u32 *)(a.fy + oy + 16 + (ptrdiff_t)r * a.sy + x);
            pre_u = a.fu[oc + 8 + (ptrdiff_t)cy * a.sc + cx];
            pre_v = a.fv[oc + 8 + (ptrdiff_t)cy * a.sc + cx];
        }
        WAVE_SYNC();
        PROF(1);
        LAUNDER();
        // ---- neighbour availability and types ----
        int nb = 0, type_top = -1, type_topleft = -1, type_topright = -1;
#define UNI(x_) __builtin_amdgcn_readfirstlane((int)(x_))      /* a wave-uniform load: keep the value in a scalar register */
        if (mby > 0) { nb |= NB_TOP; type_top = UNI(a.mb_type[mb - a.mb_w]); }
        if (mbx > 0) nb |= NB_LEFT;
        if (mbx < a.mb_w - 1 && mby > 0) { nb |= NB_TOPRIGHT; type_topright = UNI(a.mb_type[mb - a.mb_w + 1]); }
        if (mbx > 0 && mby > 0) { nb |= NB_TOPLEFT; type_topleft = UNI(a.mb_type[mb - a.mb_w - 1]); }
        int cbp_top = -1, cpm_top = 0, t8_top = 0;
        if constexpr (RD) {
            // ---- x264_ratecontrol_qp + x264_adaptive_quant (R/encoder/analyse.c:2162-2164, ratecontrol.c:257-265) ----
            int qp = a.qp;
            if (rd.aq) {
                const float off = __builtin_bit_cast(float, UNI(__builtin_bit_cast(int, rd.aq_offset[cb + mb])));
                qp = clip3((int)((double)(rd.f_qpm + off) + .5), rd.qp_min, rd.qp_max);
                if (iabs(qp - last_qp) == 1) qp = last_qp;
            }
            if (qp != Q.qp) {
                Q.qp = qp; Q.qpc = d_chroma_qp[clip3(qp + rd.chroma_qp_offset, 0, 51)];
                Q.lambda = d_lambda_tab[qp]; Q.lambda2 = d_lambda2_tab[qp]; Q.skip_thresh = (d_lambda2_tab[Q.qpc] + 32) >> 6;
                cost_g = rd.cost_mv_all + (size_t)qp * (2 * a.cost_center + 1) + a.cost_center;
                WAVE_SYNC();
                load_qp_tables(lane);
                WAVE_SYNC();
            }
            // ---- what the entropy coder reads of the neighbours (R/common/macroblock.c:896-1010,1129-1160) ----
            if constexpr (SUB8) {   // with the carry the macroblock's own entries (12 + x + 8 y) stay as the last macroblock left them, like s.nnz
                const bool own = rd.mb_carry && lane >= 12 && lane < 40 && ((lane - 12) & 7) < 4;
                if (lane < 48 && !own) { sr.cmvd[lane][0] = 0; sr.cmvd[lane][1] = 0; }
            } else
            if (lane < 48) { sr.cmvd[lane][0] = 0; sr.cmvd[lane][1] = 0; }
            WAVE_SYNC();
            if (nb & NB_TOP) {
                const int top = mb - a.mb_w;
                const u8 *nz = (a.nnz + 27 * cb) + (size_t)top * 27;
                cbp_top = UNI((a.cbp + cb)[top]); t8_top = UNI((a.t8 + cb)[top]);
                { const int ct = UNI((a.chroma_mode + cb)[top]); cpm_top = type_top == T_I_PCM ? 0 : sw_fix8c(ct); }
                if (lane < 4) sr.nz_t[lane] = nz[lane == 0 ? 10 : lane == 1 ? 11 : lane == 2 ? 14 : 15];
                else if (lane < 8) sr.nz_tc[(lane - 4) >> 1][lane & 1] = nz[16 + 4 * ((lane - 4) >> 1) + 2 + (lane & 1)];
                else if (lane < 12) {
                    const i16 *mvd = rd.mvd + ((cb + top) * 16 + 12 + (lane - 8)) * 2;
                    sr.cmvd[4 + lane - 8][0] = mvd[0]; sr.cmvd[4 + lane - 8][1] = mvd[1];
                }
            } else if (lane < 4) sr.nz_t[lane] = 0x80;
            else if (lane < 8) sr.nz_tc[(lane - 4) >> 1][lane & 1] = 0x80;
            if (nb & NB_LEFT) {
                if (lane >= 16 && lane < 20) sr.nz_l[lane - 16] = sr.left_nz[lane - 16];
                else if (lane >= 20 && lane < 24) sr.nz_lc[(lane - 20) >> 1][lane & 1] = sr.left_nz[4 + lane - 20];
                else if (lane >= 24 && lane < 28) { sr.cmvd[11 + 8 * (lane - 24)][0] = sr.left_mvd[lane - 24][0]; sr.cmvd[11 + 8 * (lane - 24)][1] = sr.left_mvd[lane - 24][1]; }
            } else if (lane >= 16 && lane < 20) sr.nz_l[lane - 16] = 0x80;
            else if (lane >= 20 && lane < 24) sr.nz_lc[(lane - 20) >> 1][lane & 1] = 0x80;
            WAVE_SYNC();
        }

        int type = T_I_16x16, mvx = 0, mvy = 0, ref = 0, skip_mc = 0, pred16 = 0, predc = 0, part = D_16x16;
        int sub_t_mb = D_L0_8x8;                    // lanes 0..3: h->mb.i_sub_partition[] (D_L0_4x4 0, 8x4 1, 4x8 2, 8x8 3)
        int satd_i16 = MX_COST_MAX, satd_chroma = MX_COST_MAX, pskx = 0, psky = 0;
        int satd_i8 = MX_COST_MAX, satd_i4 = MX_COST_MAX, i8_cbp = 0, i4_cbp = 0, t8 = 0, fi_open = 0, stat_alt = -1;
        if (a.flags_intra & 3) {
            // intra4x4_pred_mode cache (R/common/macroblock.c:907-980): -1 where there is no neighbour; the frame array holds
            // I_PRED_4x4_DC for every macroblock that is not I_4x4 / I_8x8
            if (lane < 48) s.i4c[lane] = -1;
            WAVE_SYNC();
            if ((nb & NB_TOP) && lane < 4)
                s.i4c[4 + lane] = a.i4mode[(size_t)(mb - a.mb_w) * 16 + (lane == 0 ? 10 : lane == 1 ? 11 : lane == 2 ? 14 : 15)];
            if ((nb & NB_LEFT) && lane >= 8 && lane < 12) s.i4c[11 + 8 * (lane - 8)] = s.left_i4[lane - 8];
            WAVE_SYNC();
        }
        int stat_intra = 0, stat_inter = 0, analysed = 0;
        // x264_mb_analyse_init (R/encoder/analyse.c:235-252): h->mb.b_trellis while analysing, i_skip_intra
        const int mbrd = RD ? rd.mbrd : 0;
        typename std::conditional<PT, SwTqPsy, SwTq>::type tq = {RD && rd.trellis > 1 && mbrd, &sr};
        // psy-trellis, --trellis 2: with the RD levels both source transforms are the macroblock's own from its first trial on (x264_mb_cache_fenc_satd);
        // below them nobody writes the arrays -- zeros, except in a B slice at subme 6, whose I and P slices ARE at the RD levels: it reads what the last
        // macroblock they analysed left.  --trellis 1: sw_psy_after_analysis, once the analysis is over.
        if constexpr (PT) sw_tq_set_psy(tq, rd.psy_trellis, rd.trellis > 1 && !mbrd ? (BS ? SW_PSY_KEPT : SW_PSY_ZERO) : SW_PSY_OWN, sw_psy_carry(rd, bz));
        int skip_intra = a.lossless ? 0 : mbrd ? 2 : (RD ? (!rd.trellis && !a.nr) : 1);
        (void)skip_intra;

        // x264_mb_analyse_intra_chroma, R/encoder/analyse.c:539-610
        auto analyse_chroma = [&]() {
            if (satd_chroma < MX_COST_MAX) return;
            int n;
            const u32 list = sw_modes8c(nb, n);
            for (int i = 0; i < n; i++) {
                const int m = (int)((list >> (4 * i)) & 15);
                sw_pred8c(s, m, lane, a.lossless);
                int c = sw_cmp_chroma(s, satd, lane) + Q.lambda * sw_ue_size(sw_fix8c(m));
                if constexpr (RF) { if (lane == 0) sf.cdir[i] = c; }
                if (c < satd_chroma) { satd_chroma = c; predc = m; }
            }
        };
        // a->b_fast_intra (R/encoder/analyse.c:345-362), evaluated only when its value matters.  Its last term counts
        // the intra macroblocks BEFORE this one in raster order, some of which (to the right in the rows above) may
        // not be coded yet: bound the count from what the rows above have published, and wait only while the
        // bounds leave the answer open (the rows above never wait for this one, so this terminates).
        // wait = 0: answer 0 / 1, or 2 when the bounds do not decide it yet; wait = 1: poll until they do
        auto fast_intra_now = [&](int wait) -> int {
            if ((!is_p && !BS) || mb <= 4) return 0;
            if (IS_INTRA_T(left_type) || IS_INTRA_T(type_top) || IS_INTRA_T(type_topleft) || IS_INTRA_T(type_topright)) return 0;
            if ((!BS || is_p) && a.l0_type && IS_INTRA_T(UNI(a.l0_type[mb]))) return 0;      // only in a P slice (analyse.c:357)
            if constexpr (RD) return mb < 3 * intra_before ? 0 : 1;        // raster order: every earlier macroblock is done
            for (int spins = 0;; spins++) {
                int known = row_intra, pending = 0;
                for (int r0 = 0; r0 < mby; r0 += 64) {
                    const int r = r0 + lane;
                    const int v = r < mby ? __hip_atomic_load(prog + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
                    known += wave_sum(r < mby ? v >> 16 : 0);
                    pending += wave_sum(r < mby ? a.mb_w - (v & 0xffff) : 0);
                }
                if (mb < 3 * known) return 0;
                if (mb >= 3 * (known + pending)) return 1;
                if (!wait) return 2;
                __builtin_amdgcn_s_sleep(100);
                if (spins > a.spin_limit) { if (lane == 0) { __hip_atomic_store(a.abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); atomicAdd(a.abort_total, 1); } return 0; }
            }
        };
        // x264_mb_analyse_intra, R/encoder/analyse.c:612-843
        auto analyse_intra = [&](int satd_inter) {
            LAUNDER();
            {
                int n;
                const u32 list = sw_modes16(nb, n);
                for (int i = 0; i < n; i++) {
                    const int m = (int)((list >> (4 * i)) & 15);
                    sw_pred16(s, m, lane, a.lossless);
                    int c = sw_cmp_luma16(s, satd, lane) + Q.lambda * sw_ue_size(sw_fix16(m));
                    if constexpr (RF) { if (lane == 0) sf.i16dir[m] = c; }
                    if (c < satd_i16) { satd_i16 = c; pred16 = m; }
                }
            }
            if constexpr (BS) satd_i16 += Q.lambda * 9;                  // i_mb_b_cost_table[I_16x16], analyse.c:659-661
            if (!(a.flags_intra & 3)) return;
            if (satd_i16 > 2 * satd_inter) {
                // b_fast_intra would end the analysis here.  If the raster-order count behind it is not decidable yet, go on
                // as if it were 0: the extra analysis only matters if 8x8 / 4x4 then beat the inter cost, which the caller
                // checks (and only then waits for the exact answer); the statistics term is settled after the frame.
                const int fi = fast_intra_now(0);
                if (fi == 1) return;
                fi_open = fi == 2;
            }
            if (a.flags_intra & 2) {                                   // X264_ANALYSE_I8x8
                const int thresh = mbrd ? MX_COST_MAX : min(satd_inter, satd_i16);
                int cost = BS ? Q.lambda * 9 : 0, idx, acbp = 0;            // i_mb_b_cost_table[I_8x8], :676-677
                for (idx = 0;; idx++) {
                    const int bx = 8 * (idx & 1), by = 8 * (idx >> 1), pm = sw_pred_i4mode(s, 4 * idx), nb8 = sw_nb8(idx, nb);
                    int n;
                    const unsigned long long list = sw_modes4(nb8, n);
                    sw_pred8_filter_all(s.edge8, s.fd + FDY + by * FD + bx, nb8, lane);
                    WAVE_SYNC();
                    sw_pred8_table(s, lane);
                    WAVE_SYNC();
                    u32 kb = 0xffffffffu;
#pragma unroll
                    for (int pass = 0; pass < 2; pass++) {
                        const int g = (lane >> 3) + 8 * pass, r = lane & 7;
                        u32 key = 0xffffffffu;
                        if (g < n) {
                            const int mode = (int)((list >> (4 * g)) & 15);
                            const u32 o0 = s.p8lut[(mode * 8 + r) * 2], o1 = s.p8lut[(mode * 8 + r) * 2 + 1];
                            const u32 f0 = *(const u32 *)(s.fe + (by + r) * 16 + bx), f1 = *(const u32 *)(s.fe + (by + r) * 16 + bx + 4);
                            int d[8];
#pragma unroll
                            for (int x = 0; x < 4; x++) {
                                d[x] = (int)((f0 >> (8 * x)) & 255) - (int)s.pt8[(o0 >> (8 * x)) & 255];
                                d[4 + x] = (int)((f1 >> (8 * x)) & 255) - (int)s.pt8[(o1 >> (8 * x)) & 255];
                            }
                            if (a.lossless && mode < 2) {
#pragma unroll
                                for (int x = 0; x < 8; x++) d[x] = (int)s.fe[(by + r) * 16 + bx + x] - sw_ll_px(s, 0, mode, bx + x, by + r);
                            }
                            int c;
                            if (satd) c = (sw_sa8d_rows_d(d, lane) + 2) >> 2;
                            else {
                                int sd = 0;
#pragma unroll
                                for (int x = 0; x < 8; x++) sd += iabs(d[x]);
                                c = half_sum8(sd);
                            }
                            key = ((u32)(c + Q.lambda * (pm == mb_fix4(mode) ? 1 : 4)) << 4) | (u32)g;
                            if constexpr (RF) { if (r == 0) sf.i8dir[mode][idx] = (int)(key >> 4); }
                        }
                        // the reference's in-order strict '<' over the modes = the smallest (cost, slot) key
#pragma unroll
                        for (int k = 0; k < 8; k++) { const u32 t = (u32)__builtin_amdgcn_readlane((int)key, 8 * k); kb = t < kb ? t : kb; }
                    }
                    const int best = (int)(kb >> 4), bmode = (int)((list >> (4 * (kb & 15))) & 15);
                    cost += best;
                    if (lane == 0) s.pred8[idx] = (signed char)bmode;
                    if (idx == 3 || cost > thresh) break;
                    {
                        int v = s.pt8[(s.p8lut[(bmode * 8 + (lane >> 3)) * 2 + ((lane >> 2) & 1)] >> (8 * (lane & 3))) & 255];
                        if (a.lossless && bmode < 2) v = sw_ll_px(s, 0, bmode, bx + (lane & 7), by + (lane >> 3));
                        WAVE_SYNC();
                        s.fd[FDY + (by + (lane >> 3)) * FD + bx + (lane & 7)] = (u8)v;
                        if (lane < 4) s.i4c[mb_scan8_luma(4 * idx) + (lane & 1) + 8 * (lane >> 1)] = (signed char)bmode;
                        WAVE_SYNC();
                    }
                    sw_encode_i8x8(s, a, Q, tq, idx, acbp, lane);
                }
                if (idx == 3) {
                    satd_i8 = cost; i8_cbp = acbp;
                    if constexpr (RD) { if (skip_intra == 2) for (int k = lane; k < 256; k += 64) sr.i8_dct[k] = s.lv_y8[k]; }
                    *(u32 *)(s.i8_fdec + lane * 4) = *(const u32 *)(s.fd + FDY + (lane >> 2) * FD + (lane & 3) * 4);
                    if (lane < 16) s.i8_nnz[lane] = s.nnz[lane];
                    WAVE_SYNC();
                } else {
                    satd_i8 = MX_COST_MAX;
                    cost = (cost * (idx == 0 ? 1024 : idx == 1 ? 512 : 341)) >> 8;
                }
                if (min(cost, satd_i16) > satd_inter * (5 + !!mbrd) / 4) return;
            }
            if (a.flags_intra & 1) {                                   // X264_ANALYSE_I4x4
                int thresh = min(min(satd_inter, satd_i16), satd_i8);
                if (mbrd) thresh = thresh * (10 - fast_intra_now(0)) / 8;
                int cost = Q.lambda * (BS ? 24 + 9 : 24), idx, acbp = 0;    // + i_mb_b_cost_table[I_4x4] in a B slice, :770-771
                for (idx = 0;; idx++) {
                    int bx, by, n;
                    sw_blk_xy(idx, bx, by);
                    const int pm = sw_pred_i4mode(s, idx), nb4 = sw_nb4(idx, nb);
                    const unsigned long long list = sw_modes4(nb4, n);
                    u8 *dst = s.fd + FDY + by * FD + bx;
                    if ((nb4 & (NB_TOPRIGHT | NB_TOP)) == NB_TOP && lane < 4) dst[4 - FD + lane] = dst[3 - FD];    // emulate missing topright samples
                    WAVE_SYNC();
                    sw_pred4_table(s, dst, lane);
                    WAVE_SYNC();
                    u32 key = 0xffffffffu;
                    {
                        const int g = lane >> 2, r = lane & 3;
                        if (g < n) {
                            const int mode = (int)((list >> (4 * g)) & 15);
                            const u32 off = s.p4lut[mode * 4 + r], fw = *(const u32 *)(s.fe + (by + r) * 16 + bx);
                            int d0 = (int)(fw & 255) - (int)s.pt4[off & 255], d1 = (int)((fw >> 8) & 255) - (int)s.pt4[(off >> 8) & 255];
                            int d2 = (int)((fw >> 16) & 255) - (int)s.pt4[(off >> 16) & 255], d3 = (int)(fw >> 24) - (int)s.pt4[off >> 24];
                            if (a.lossless && mode < 2) {
                                d0 = (int)(fw & 255) - sw_ll_px(s, 0, mode, bx, by + r); d1 = (int)((fw >> 8) & 255) - sw_ll_px(s, 0, mode, bx + 1, by + r);
                                d2 = (int)((fw >> 16) & 255) - sw_ll_px(s, 0, mode, bx + 2, by + r); d3 = (int)(fw >> 24) - sw_ll_px(s, 0, mode, bx + 3, by + r);
                            }
                            const int c = sw_cost4x4_rows(d0, d1, d2, d3, satd, lane);
                            key = ((u32)(c + Q.lambda * (pm == mb_fix4(mode) ? 1 : 4)) << 4) | (u32)g;
                        }
                    }
                    u32 kb = (u32)__builtin_amdgcn_readlane((int)key, 0);
#pragma unroll
                    for (int k = 1; k < 9; k++) { const u32 t = (u32)__builtin_amdgcn_readlane((int)key, 4 * k); kb = t < kb ? t : kb; }
                    const int best = (int)(kb >> 4), bmode = (int)((list >> (4 * (kb & 15))) & 15);
                    cost += best;
                    if (lane == 0) s.pred4[idx] = (signed char)bmode;
                    if (cost > thresh || idx == 15) break;
                    if (lane < 16) dst[(lane >> 2) * FD + (lane & 3)] = a.lossless && bmode < 2 ? (u8)sw_ll_px(s, 0, bmode, bx + (lane & 3), by + (lane >> 2))
                                                                         : s.pt4[(s.p4lut[bmode * 4 + (lane >> 2)] >> (8 * (lane & 3))) & 255];
                    if (lane == 0) s.i4c[mb_scan8_luma(idx)] = (signed char)bmode;
                    WAVE_SYNC();
                    sw_encode_i4x4(s, a, Q, tq, idx, acbp, lane);
                }
                if (idx == 15) {
                    satd_i4 = cost; i4_cbp = acbp;
                    if constexpr (RD) { if (skip_intra == 2) for (int k = lane; k < 256; k += 64) sr.i4_dct[k] = s.lv_y[k]; }
                    *(u32 *)(s.i4_fdec + lane * 4) = *(const u32 *)(s.fd + FDY + (lane >> 2) * FD + (lane & 3) * 4);
                    if (lane < 16) s.i4_nnz[lane] = s.nnz[lane];
                    WAVE_SYNC();
                } else
                    satd_i4 = MX_COST_MAX;
            }
        };

        // ---- x264_macroblock_encode (R/encoder/macroblock.c:475-790) of the macroblock as type / part / t8 / the intra modes / s.mv4 /
        // s.ref8 describe it now.  The final encode, and with the RD levels every trial encode of x264_rd_cost_mb (final_pass = 0).
        int cbp_luma = 0, cbp_chroma = 0;
        bool encoded = false;               // (RD) the final encode has run inside the candidate loop
        auto encode_pskip = [&]() {         // x264_macroblock_encode_pskip, macroblock.c:378-402
            cbp_luma = 0; cbp_chroma = 0;
            if (lane < 32) s.nnz[lane] = 0;
            mvx = pskx; mvy = psky; ref = 0;
            if (lane < 16) { s.mv4[lane][0] = (i16)pskx; s.mv4[lane][1] = (i16)psky; }
            if (lane < 4) s.ref8[lane] = 0;
            WAVE_SYNC();
            if (!skip_mc) {
                const int vx = clip3(mvx, 4 * (-16 * mbx - 24), 4 * (16 * (a.mb_w - mbx - 1) + 24));
                const int vy = clip3(mvy, 4 * (-16 * mby - 24), 4 * (16 * (a.mb_h - mby - 1) + 24));
                sw_mc16(s, refs, a, 0, vx, vy, oy, oc, by_, bc_, lane, true);
                WAVE_SYNC();
            }
        };
        auto psy_after_analysis = [&]() {   // analyse.c:2770-2771, with t8 = h->mb.b_transform_8x8 as the analysis left it
            if constexpr (PT) { if (rd.trellis == 1) sw_psy_after_analysis(s, tq, t8, lane); }
        };
        auto encode_mb = [&](int final_pass) {
            if (type == T_P_SKIP) { encode_pskip(); return; }
            cbp_luma = 0; cbp_chroma = 0;
            if (lane < 32) s.nnz[lane] = 0;
            WAVE_SYNC();
            if (BS && type == T_B_SKIP) return;              // x264_macroblock_encode_skip: the prediction (made by the caller) is the reconstruction
            if (final_pass && IS_INTRA_T(type)) psy_after_analysis();
            if (type == T_I_16x16) {
                t8 = 0;
                analyse_chroma();
                sw_pred16(s, pred16, lane, a.lossless);
                cbp_luma = sw_encode_i16x16(s, a, Q, tq, lane, BS);
                sw_pred8c(s, predc, lane, a.lossless);
                cbp_chroma = sw_encode_chroma(s, a, Q, tq, 0, lane);
            } else if (type == T_I_8x8 || type == T_I_4x4) {
                // x264_analyse_update_cache: the winner's modes into the cache; then macroblock.c:527-590.  With i_skip_intra the
                // analysis already encoded all blocks but the last: take its state and finish; without it (trellis 1, --nr,
                // lossless) every block is predicted and coded again.
                const bool i8 = type == T_I_8x8;
                if (lane < 16) s.i4c[mb_scan8_luma(lane)] = i8 ? s.pred8[lane >> 2] : s.pred4[lane];
                analyse_chroma();
                if (skip_intra) {
                    *(u32 *)(s.fd + FDY + (lane >> 2) * FD + (lane & 3) * 4) = *(const u32 *)((i8 ? s.i8_fdec : s.i4_fdec) + lane * 4);
                    if (lane < 16) s.nnz[lane] = i8 ? s.i8_nnz[lane] : s.i4_nnz[lane];
                    cbp_luma = i8 ? i8_cbp : i4_cbp;
                    if constexpr (RD) {                  // "In RD mode, restore the now-overwritten DCT data", macroblock.c:543
                        if (skip_intra == 2) for (int k = lane; k < 256; k += 64) { if (i8) s.lv_y8[k] = sr.i8_dct[k]; else s.lv_y[k] = sr.i4_dct[k]; }
                    }
                }
                WAVE_SYNC();
                if (i8) {
                    t8 = 1;
                    for (int idx = skip_intra ? 3 : 0; idx < 4; idx++) {
                        const int bx = 8 * (idx & 1), by = 8 * (idx >> 1);
                        const int mode = __builtin_amdgcn_readfirstlane((int)s.pred8[idx]), nb8 = sw_nb8(idx, nb);
                        // x264_pred_i4x4_neighbors (R/common/macroblock.h:40-54)
                        const int need = mode == 0 || mode == 10 ? NB_TOP : mode == 1 || mode == 8 || mode == 9 ? NB_LEFT : mode == 2 ? NB_LEFT | NB_TOP
                                       : mode == 3 || mode == 7 ? NB_TOP | NB_TOPRIGHT : mode == 11 ? 0 : NB_LEFT | NB_TOPLEFT | NB_TOP;
                        if (lane == 0) pred8_filter(s.edge8, s.fd + FDY + by * FD + bx, FD, nb8, need);
                        WAVE_SYNC();
                        const int v = a.lossless && mode < 2 ? sw_ll_px(s, 0, mode, bx + (lane & 7), by + (lane >> 3)) : pred8_px(mode, s.edge8, lane & 7, lane >> 3);
                        WAVE_SYNC();
                        s.fd[FDY + (by + (lane >> 3)) * FD + bx + (lane & 7)] = (u8)v;
                        WAVE_SYNC();
                        sw_encode_i8x8(s, a, Q, tq, idx, cbp_luma, lane);
                    }
                } else {
                    t8 = 0;
                    for (int idx = skip_intra ? 15 : 0; idx < 16; idx++) {
                        int bx, by;
                        sw_blk_xy(idx, bx, by);
                        u8 *dst = s.fd + FDY + by * FD + bx;
                        const int mode = __builtin_amdgcn_readfirstlane((int)s.pred4[idx]);
                        if ((sw_nb4(idx, nb) & (NB_TOPRIGHT | NB_TOP)) == NB_TOP && lane < 4) dst[4 - FD + lane] = dst[3 - FD];
                        WAVE_SYNC();
                        if (lane < 13) pred4_edges(s.e4, dst, FD, lane);
                        WAVE_SYNC();
                        if (lane < 16) dst[(lane >> 2) * FD + (lane & 3)] = (u8)(a.lossless && mode < 2 ? sw_ll_px(s, 0, mode, bx + (lane & 3), by + (lane >> 2))
                                                                                                       : pred4_px(mode, s.e4, lane & 3, lane >> 2));
                        WAVE_SYNC();
                        sw_encode_i4x4(s, a, Q, tq, idx, cbp_luma, lane);
                    }
                }
                sw_pred8c(s, predc, lane, a.lossless);
                cbp_chroma = sw_encode_chroma(s, a, Q, tq, 0, lane);
            } else {
                if constexpr (!BS) sw_mc_parts(s, refs, a, oy, oc, by_, bc_, lane, RF, mbx, mby);    // (B slice: the caller has run the bi-predictive motion compensation)
                WAVE_SYNC();
                // x264_mb_transform_8x8_allowed: a P_8x8 macroblock only with four 8x8 sub-partitions
                if (!mbrd && a.transform8x8 && !a.lossless && (type != T_P_8x8 || __ballot(lane < 4 && sub_t_mb != D_L0_8x8) == 0)) {
                    // x264_mb_analyse_transform (R/encoder/analyse.c:2109-2126): SA8D against SATD of the 16x16 prediction error
                    int raw = 0;
                    if (lane < 32) {
                        const int blk = lane >> 3, r = lane & 7;
                        raw = sw_sa8d_rows(s.fe + ((blk >> 1) * 8 + r) * 16 + (blk & 1) * 8, s.fd + FDY + ((blk >> 1) * 8 + r) * FD + (blk & 1) * 8, lane);
                    }
                    const int c8 = (__builtin_amdgcn_readlane(raw, 0) + __builtin_amdgcn_readlane(raw, 8) + __builtin_amdgcn_readlane(raw, 16)
                                    + __builtin_amdgcn_readlane(raw, 24) + 2) >> 2;
                    const int c4 = sw_cmp_luma16(s, 1, lane);
                    t8 = c8 < c4;
                }
                if (final_pass) psy_after_analysis();
                const int nr_on = a.nr && final_pass;        // h->mb.b_noise_reduction is off while analysing (analyse.c:237,2769)
                if (nr_on) { if (t8) nr_n8 += 4; else nr_n4 += 16; }
                if (LL && t8) {      // zigzag sub_8x8 of the four blocks (macroblock.c:604-615): only x264_mb_analyse_transform_rd turns the 8x8 transform on here
                    for (int idx = 0; idx < 4; idx++) sw_ll_i8x8(s, idx, cbp_luma, lane);
                } else
                cbp_luma = t8 ? sw_encode_inter_luma8(s, a, Q, tq, lane, &nr_acc8, nr_on) : sw_encode_inter_luma(s, a, Q, tq, lane, &nr_acc4, nr_on);   // never a conditional pointer: that pins the counter in scratch memory
                cbp_chroma = sw_encode_chroma(s, a, Q, tq, 1, lane);
                if (type == T_P_L0 && part == D_16x16 && !(cbp_luma | cbp_chroma) && mvx == pskx && mvy == psky && ref == 0) type = T_P_SKIP;
                if (BS && type == T_B_DIRECT && !(cbp_luma | cbp_chroma)) type = T_B_SKIP;       // macroblock.c:784-788
            }
        };

        // ---- the RD levels: x264_mb_cache_fenc_satd, ssd_mb, x264_macroblock_size_cabac, x264_rd_cost_mb ----
        int fenc_satd_sum = 0, fenc_sa8d_sum = 0;
        auto cache_fenc_satd = [&]() {     // R/encoder/analyse.c:509-537 (the 16x16 sums; sub-partition RD is not built)
            // :515-516.  Only a B slice below the RD levels ever reads what this leaves (above): subme 6, whose I and P slices run this
            if constexpr (PT && !BS) { if (rd.trellis == 2 && a.subme == 6) sw_psy_before_trials(s, tq, a.transform8x8, lane); }
            if (!rd.psy_rd) return;
            int v4 = 0, v8 = 0;
            if (lane < 16) {
                const u8 *fe = s.fe + (lane >> 2) * 64 + (lane & 3) * 4;
                int sad = 0;
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int i = 0; i < 4; i++) sad += fe[j * 16 + i];
                v4 = satd_4x4(sr.zero16, 0, fe, 16) - (sad >> 1);
            } else if (lane < 20) {
                const int b = lane - 16;
                const u8 *fe = s.fe + (b >> 1) * 128 + (b & 1) * 8;
                int sad = 0;
                for (int j = 0; j < 8; j++)
#pragma unroll
                    for (int i = 0; i < 8; i++) sad += fe[j * 16 + i];
                v8 = ((sa8d_8x8_raw(sr.zero16, 0, fe, 16) + 2) >> 2) - (sad >> 2);
            }
            fenc_satd_sum = wave_sum(v4); fenc_sa8d_sum = wave_sum(v8);
            if constexpr (RF) {         // h->mb.pic.fenc_satd[y][x] / fenc_sa8d[y][x]: the partial RD costs sum them over their blocks (sum_satd / sum_sa8d, rdo.c:66-91)
                if (lane < 16) sr.fenc_satd[lane] = v4; else if (lane < 20) sr.fenc_sa8d[lane - 16] = v8;
                WAVE_SYNC();
            }
        };
        auto ssd_mb = [&]() -> int {       // ssd_mb / ssd_plane, R/encoder/rdo.c:106-137
            int acc = 0;
            {
                const int r = lane >> 2, x = (lane & 3) * 4, cx = lane & 7, cy = lane >> 3;
#pragma unroll
                for (int i = 0; i < 4; i++) { const int d = (int)s.fe[r * 16 + x + i] - (int)s.fd[FDY + r * FD + x + i]; acc += d * d; }
                const int du = (int)s.fe[256 + cy * 8 + cx] - (int)s.fd[FDU + cy * FD + cx], dv = (int)s.fe[320 + cy * 8 + cx] - (int)s.fd[FDV + cy * FD + cx];
                acc += du * du + dv * dv;
            }
            int ssd = wave_sum(acc);
            if (rd.psy_rd) {
                unsigned long long h = 0;
                if (lane < 4) h = hadamard_ac_8x8(s.fd + FDY + (lane >> 1) * 8 * FD + (lane & 1) * 8, FD);
                const u32 lo = (u32)h, hi = (u32)(h >> 32);
                unsigned long long sum = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) sum += ((unsigned long long)(u32)__builtin_amdgcn_readlane((int)hi, k) << 32) + (u32)__builtin_amdgcn_readlane((int)lo, k);
                const int s4 = (int)((u32)sum >> 1), s8 = (int)(sum >> 34);
                const int satd = (iabs(s4 - fenc_satd_sum) + iabs(s8 - fenc_sa8d_sum)) >> 1;
                ssd += (satd * rd.psy_rd * Q.lambda + 128) >> 8;
            }
            return ssd;
        };
        // what the entropy coder reads of this macroblock: the interior of the motion cache from s.mv4 / s.ref8 (all lanes) ...
        auto syn_prepare = [&]() {
            if (is_p && lane < 16) {
                const int k = 12 + (lane & 3) + 8 * (lane >> 2);
                sr.cref[k] = s.ref8[(lane >> 3) * 2 + ((lane & 3) >> 1)]; sr.cmv[k][0] = s.mv4[lane][0]; sr.cmv[k][1] = s.mv4[lane][1];
            }
            if (lane < 4) sr.sub[lane] = (signed char)sub_t_mb;
            WAVE_SYNC();
        };
        // ... and the record the writer walks (scalars: wave-uniform registers)
        auto make_syn = [&]() -> MbSynDev {
            MbSynDev y;
            y.slice_type = a.slice_type; y.type = type; y.partition = part; y.i16mode = pred16; y.chroma_mode = predc;
            y.cbp_luma = cbp_luma; y.cbp_chroma = cbp_chroma; y.t8 = t8; y.qp = Q.qp; y.n_ref = a.n_refs; y.pps_t8 = a.transform8x8;
            y.t8_allowed = a.transform8x8 && (type == T_P_L0 || (type == T_P_8x8 && __ballot(lane < 4 && sub_t_mb != D_L0_8x8) == 0));
            if constexpr (BS) y.t8_allowed = a.transform8x8 && type >= T_B_DIRECT && type <= T_B_8x8;
            // h->mb.type[] holds x264_mb_type_fix'ed types (I_8x8 is stored as I_4x4, R/common/macroblock.c:1209,1226)
            y.type_left = left_type == T_I_8x8 ? T_I_4x4 : left_type; y.type_top = type_top == T_I_8x8 ? T_I_4x4 : type_top; y.cbp_left = left_cbp; y.cbp_top = cbp_top; y.cpm_left = left_cpm; y.cpm_top = cpm_top;
            y.nb_t8 = (left_type >= 0 && left_t8) + (type_top >= 0 && t8_top);
            y.last_qp = last_qp; y.last_dqp = last_dqp; y.prev_coded = prev_coded;
            y.sub = sr.sub; y.i4c = s.i4c; y.cref = sr.cref; y.cmv = sr.cmv; y.cmvd = sr.cmvd;
            y.n_ref1 = 0; y.cref1 = nullptr; y.cskip = nullptr; y.cmv1 = nullptr; y.cmvd1 = nullptr;
            if constexpr (BS) { y.n_ref1 = 1; y.sub = sb.sub; y.cref1 = sb.cref1; y.cskip = sb.cskip; y.cmv1 = sb.cmv1; y.cmvd1 = sb.cmvd1; }
            y.nnz = s.nnz; y.nz_l = sr.nz_l; y.nz_t = sr.nz_t; y.nz_lc = sr.nz_lc; y.nz_tc = sr.nz_tc;
            y.lv4 = (i16 (*)[16])s.lv_y; y.lv8 = (i16 (*)[64])s.lv_y8; y.lv_dc = s.lv_dc; y.lv_cdc = (i16 (*)[4])s.lv_cdc; y.lv_cac = (i16 (*)[16])s.lv_cac;
            return y;
        };
        // x264_macroblock_size_cabac of an RD trial (rdo.c:139-171), priced against a copy of the live contexts: the coefficient arrays summarised
        // by ballots of the whole wave first, then lane 0 walks the syntax (cabac_price.h)
        auto price_mb = [&]() -> int {
            syn_prepare();
            for (int k = lane; k < 460; k += 64) sr.cabac_tmp[k] = sr.cabac[k];
            const MbSynDev y0 = make_syn();
            const CpMasks km = cp_masks([&](int q) -> cp_u64 { return __ballot(cp_mask_lane(y0, q, lane)); });
            WAVE_SYNC();
            if (lane == 0) {
                DCabac tcb = {0, 0x1FE, -1, 0, nullptr, 0};
                MbSynDev y = y0;
                cp_macroblock(tcb, sr.cabac_tmp, y, km);
                sr.tmp_i[0] = tcb.f8;
            }
            WAVE_SYNC();
            return UNI(sr.tmp_i[0]);
        };
        (void)cache_fenc_satd; (void)ssd_mb; (void)price_mb;
        // a->i_satd_pcm, analyse.c:246
        const int satd_pcm = RD && !rd.psy_rd && mbrd ? (int)(((unsigned long long)(386 * 8) * (u32)Q.lambda2 + 128) >> 8) : MX_COST_MAX;

        if constexpr (BS) {
#include "slice_b_flow.h"
        } else
        if (!RD && !is_p) {
          {
            analyse_intra(MX_COST_MAX);
            type = T_I_16x16;
            int i_cost = satd_i16;
            if (satd_i4 < i_cost) { i_cost = satd_i4; type = T_I_4x4; }
            if (satd_i8 < i_cost) { i_cost = satd_i8; type = T_I_8x8; }
          }
        } else {
            // (The raster variant sends an I slice's macroblocks down this path too, its motion parts skipped: the candidate loop at the
            // end -- and with it the encoder, the distortion and the bit counter -- then exists ONCE in the kernel.  Two call sites of
            // the encoder made the compiler keep it as a function, and every variable it shares with the rest in scratch memory.)
            // ---- motion neighbours: what cache_load puts around the block (R/common/macroblock.c:1040-1128) ----
            int ra = left_ref, ax = left_mvx, ay = left_mvy;                 // A
            int rb = -2, bx = 0, byv = 0, rc = -2, cx = 0, cy = 0;            // B, C (or D)
            if (is_p && (nb & NB_TOP)) { const int o = mb - a.mb_w; rb = UNI(a.ref[o * 4 + 2]); bx = UNI(a.mv[(o * 16 + 12) * 2]); byv = UNI(a.mv[(o * 16 + 12) * 2 + 1]); }
            if (!is_p) {}
            else if (nb & NB_TOPRIGHT) { const int o = mb - a.mb_w + 1; rc = UNI(a.ref[o * 4 + 2]); cx = UNI(a.mv[(o * 16 + 12) * 2]); cy = UNI(a.mv[(o * 16 + 12) * 2 + 1]); }
            else if (nb & NB_TOPLEFT) { const int o = mb - a.mb_w - 1; rc = UNI(a.ref[o * 4 + 3]); cx = UNI(a.mv[(o * 16 + 15) * 2]); cy = UNI(a.mv[(o * 16 + 15) * 2 + 1]); }
            // The motion cache (h->mb.cache.ref[0] / mv[0], x264_scan8 layout) and the partition analysis' candidate records live in
            // the register file as lane-indexed arrays: entry k = lane k of a VGPR, read with v_readlane (uniform index), written
            // by the lane itself or with v_writelane -- no LDS round trip, no barrier.
            int cref_v = -2, cmvx_v = 0, cmvy_v = 0, pme_v = 0;
            int sub_mx = 0, sub_my = 0, sub_cost = 0, sub_px = 0, sub_py = 0, sub_t = D_L0_8x8;      // sub-8x8 records (lanes 0..31) and chosen type (lanes 0..3)
            int sub_cst = MX_COST_MAX;          // (SUB8) lane 4 i + t: a->l0.i_cost4x4[i] / i_cost8x4[i] / i_cost4x8[i] (t = D_L0_4x4, 8x4, 4x8), COST_MAX where not searched
            (void)sub_cst;
            if (is_p && (RD || (a.flags_inter & 0x10))) {
                // the full motion cache for x264_mb_predict_mv on partitions: -2 = not available, neighbours as cache_load leaves them
                if ((nb & NB_TOP) && lane >= 4 && lane < 8) {
                    const int o = mb - a.mb_w, k = lane - 4;
                    cref_v = a.ref[o * 4 + 2 + (k >> 1)]; cmvx_v = a.mv[(o * 16 + 12 + k) * 2]; cmvy_v = a.mv[(o * 16 + 12 + k) * 2 + 1];
                }
                if ((nb & NB_TOPLEFT) && lane == 3) {
                    const int o = mb - a.mb_w - 1;
                    cref_v = a.ref[o * 4 + 3]; cmvx_v = a.mv[(o * 16 + 15) * 2]; cmvy_v = a.mv[(o * 16 + 15) * 2 + 1];
                }
                if ((nb & NB_TOPRIGHT) && lane == 8) {
                    const int o = mb - a.mb_w + 1;
                    cref_v = a.ref[o * 4 + 2]; cmvx_v = a.mv[(o * 16 + 12) * 2]; cmvy_v = a.mv[(o * 16 + 12) * 2 + 1];
                }
                if ((nb & NB_LEFT) && lane >= 11 && lane < 36 && ((lane - 11) & 7) == 0) {
                    const int i = (lane - 11) >> 3;
                    cref_v = s.left_r8[i >> 1]; cmvx_v = s.left_mv4[i][0]; cmvy_v = s.left_mv4[i][1];
                }
            }
            if constexpr (RD) { if (is_p && lane == 30) { cref_v = st0r; cmvx_v = st0x; cmvy_v = st0y; } }      // the entry cache_load does not rewrite
            if constexpr (RD) {     // the neighbours' part of the motion cache, for the entropy coder's x264_mb_predict_mv / ref contexts
                if (is_p) {
                    if (lane < 48) { sr.cref[lane] = (signed char)cref_v; sr.cmv[lane][0] = (i16)cmvx_v; sr.cmv[lane][1] = (i16)cmvy_v; }
                    WAVE_SYNC();
                }
            }
            // x264_mb_predict_mv_16x16, :90-128, and below x264_mb_predict_mv on the cache held in registers: the P flow keeps its own copies of
            // mb_vocab.h's mb_predict_mv_abc / mb_predict_mv (the shared statements, which these restate) -- routed through them, the RD
            // instantiation spills (3 VGPR spills, 8 bytes of scratch where it has none)
            auto predict16 = [&](int i_ref, int &px, int &py) {
                const int cnt = (ra == i_ref) + (rb == i_ref) + (rc == i_ref);
                if (cnt > 1) { px = mb_median(ax, bx, cx); py = mb_median(ay, byv, cy); }
                else if (cnt == 1) { if (ra == i_ref) { px = ax; py = ay; } else if (rb == i_ref) { px = bx; py = byv; } else { px = cx; py = cy; } }
                else if (rb == -2 && rc == -2 && ra != -2) { px = ax; py = ay; }
                else { px = mb_median(ax, bx, cx); py = mb_median(ay, byv, cy); }
            };
            // x264_mb_predict_mv_pskip, :131-149
            if (ra == -2 || rb == -2 || !(ra | ax | ay) || !(rb | bx | byv)) { pskx = 0; psky = 0; }
            else predict16(0, pskx, psky);

            int b_skip = 0, try_pskip = 0;
            if (is_p && a.fast_pskip) {
                if (a.subme >= 3) try_pskip = 1;
                else if (left_type == T_P_SKIP || type_top == T_P_SKIP || type_topleft == T_P_SKIP || type_topright == T_P_SKIP) {
                    b_skip = sw_probe_pskip(s, refs, a, Q, pskx, psky, mbx, mby, oy, oc, by_, bc_, lane);
                    skip_mc = b_skip;
                }
            }
            if (b_skip) type = T_P_SKIP;
            else {
                // ---- x264_mb_analyse_inter_p16x16, R/encoder/analyse.c:1077-1143 ----
                const MeLimits L = me_limits(mbx, mby, a.mb_w, a.mb_h, a.mv_range);
                MxCtx c;
                c.fe = (MX_LDS(u32))s.fe; c.fe_u = (MX_LDS(u8))(s.fe + 256); c.fe_v = (MX_LDS(u8))(s.fe + 320); c.sy = a.sy; c.sc = a.sc; c.lane = lane; c.set_block(16, 16, 0, 0);
                c.cost_g = (MX_GLB(i16))cost_g;           // (the current macroblock's QP: with adaptive quantisation not the slice's)
                c.cost_l = (MX_LDS(i16))s.costl; c.has_cost_l = true; c.patch = (MX_LDS(u8))s.patch; c.has_patch = true; c.patch_on = false;
                int thresh = 0x7fffffff, best = 0x7fffffff, bmvpx = 0, bmvpy = 0;
                bool early_skip = false;
                for (int r = 0; r < (is_p ? a.n_refs : 0); r++) {
                    int mvpx, mvpy;
                    predict16(r, mvpx, mvpy);
                    // x264_mb_predict_mv_ref16x16, R/common/macroblock.c:376-437
                    int n_mvc = 0;
                    {
                        const i16 *mvr = a.mvr + (size_t)r * nmb * 2;
                        const int top = mb - a.mb_w;
                        WAVE_SYNC();                                   // the previous reference's candidates have been read
                        // every lane stores the same values: the list is wave-uniform
#define SETC(vx_, vy_) do { s.mvc[n_mvc][0] = (i16)(vx_); s.mvc[n_mvc][1] = (i16)(vy_); n_mvc++; } while (0)
                        if (r == 0 && a.lowres0) {       // the lookahead's vector, twice (R/common/macroblock.c:393-398); 0x7fff in the chain's first component: none
                            const i16 *lw = a.lowres0 + 2 * cb;      // (re-derived from the argument where it is used: nothing to keep live across the macroblock)
                            if (UNI(lw[0]) != 0x7fff) SETC((u16)(UNI(lw[2 * mb]) << 1), (u16)(UNI(lw[2 * mb + 1]) << 1));
                        }
                        if ((nb & NB_LEFT) && left_type != T_P_SKIP) SETC(s.left_mvr[r][0], s.left_mvr[r][1]);
                        if (nb & NB_TOP) {
                            if (type_top != T_P_SKIP) SETC(mvr[2 * top], mvr[2 * top + 1]);
                            if ((nb & NB_TOPLEFT) && type_topleft != T_P_SKIP) SETC(mvr[2 * (top - 1)], mvr[2 * (top - 1) + 1]);
                            if (mbx < a.mb_w - 1 && type_topright != T_P_SKIP) SETC(mvr[2 * (top + 1)], mvr[2 * (top + 1) + 1]);
                        }
                        if (a.l0_n_ref0 > 0)
                            for (int k = 0; k < 3; k++) {
                                const int dx = k == 1, dy = k == 2;
                                if ((dx && mbx >= a.mb_w - 1) || (dy && mby >= a.mb_h - 1)) continue;
                                const int o = mb + dx + dy * a.mb_w, ref_col = a.l0_ref[o * 4];
                                if (ref_col >= 0) {
                                    const int scale = refs.poc_delta[r] * refs.l0_inv_ref_poc[ref_col];
                                    SETC((a.l0_mv[o * 32] * scale + 128) >> 8, (a.l0_mv[o * 32 + 1] * scale + 128) >> 8);
                                }
                            }
#undef SETC
                        WAVE_SYNC();
                    }
#pragma unroll
                    for (int k = 0; k < 4; k++) c.pl[k] = (MX_GLB(u8))(refs.y[r][k] + by_ + oy);
                    c.cu = (MX_GLB(u8))(refs.u[r] + bc_ + oc); c.cv = (MX_GLB(u8))(refs.v[r] + bc_ + oc);
                    c.mvpx = mvpx; c.mvpy = mvpy;
                    thresh -= (Q.lambda * refs.ref_bits[r]);
                    int smx, smy, cost_mv;
                    LAUNDER(); c.lane = lane;
                    int cost = me_search_ref16(c, L, mo, &s.mvc[0][0], n_mvc, &thresh, smx, smy, cost_mv);   // with one reference the threshold never bites (it starts at COST_MAX); a conditional
                                                                                        // pointer would pin it in scratch memory
                    if (r == 0 && try_pskip && cost - cost_mv < 300 * Q.lambda && iabs(smx - pskx) + iabs(smy - psky) <= 1) {
                        if (sw_probe_pskip(s, refs, a, Q, pskx, psky, mbx, mby, oy, oc, by_, bc_, lane)) { early_skip = true; break; }
                    }
                    cost += (Q.lambda * refs.ref_bits[r]);
                    thresh += (Q.lambda * refs.ref_bits[r]);
                    if (cost < best) { best = cost; mvx = smx; mvy = smy; ref = r; bmvpx = mvpx; bmvpy = mvpy; }
                    if (lane == 0) {
                        a.mvr[((size_t)r * nmb + mb) * 2] = (i16)smx; a.mvr[((size_t)r * nmb + mb) * 2 + 1] = (i16)smy;
                        s.left_mvr[r][0] = (i16)smx; s.left_mvr[r][1] = (i16)smy;
                        s.l0mvc[r][0][0] = (i16)smx; s.l0mvc[r][0][1] = (i16)smy;          // a->l0.mvc[i_ref][0]
                    }
                }
                if (early_skip) { type = T_P_SKIP; skip_mc = 1; }
                else {
                    type = T_P_L0;
                    // point the search context at a block of reference r (LOAD_HPELS, analyse.c:1065-1072)
                    auto aim = [&](int r, int w, int h, int bx, int by) {
#pragma unroll
                        for (int k = 0; k < 4; k++) c.pl[k] = (MX_GLB(u8))(refs.y[r][k] + by_ + oy + (ptrdiff_t)by * a.sy + bx);
                        c.cu = (MX_GLB(u8))(refs.u[r] + bc_ + oc + (ptrdiff_t)(by >> 1) * a.sc + (bx >> 1)); c.cv = (MX_GLB(u8))(refs.v[r] + bc_ + oc + (ptrdiff_t)(by >> 1) * a.sc + (bx >> 1));
                        c.set_block(w, h, bx, by);
                    };
                    // candidate records of the partition analysis (x264_me_t's mv / cost / cost_mv / i_ref / i_ref_cost / mvp):
                    // slots 0-3 me8x8, 4-5 me16x8, 6-7 me8x16.  Wave-uniform values, parked in LDS because they are indexed.
                    auto pme_put = [&](int slot, int vx, int vy, int cost, int cost_mv, int r, int ref_cost, int px, int py) {
                        const int f = lane - slot * 8;                          // this lane's field of that record, if 0..7
                        pme_v = f == 0 ? vx : f == 1 ? vy : f == 2 ? cost : f == 3 ? cost_mv : f == 4 ? r : f == 5 ? ref_cost : f == 6 ? px : f == 7 ? py : pme_v;
                    };
                    auto pme = [&](int slot, int f) -> int { return __builtin_amdgcn_readlane(pme_v, slot * 8 + f); };
                    // x264_macroblock_cache_ref / _mv on a run of 4x4 blocks of the motion cache
                    auto cache_set = [&](int x, int y, int w, int h, int r, int vx, int vy, int set_mv) {
                        const int k = lane - 12, i = k & 7, j = k >> 3;          // cache entry 12 + i + 8 j = 4x4 block (i, j)
                        if (k >= 0 && i < 4 && j < 4 && i >= x && i < x + w && j >= y && j < y + h) {
                            cref_v = r;
                            if (set_mv) { cmvx_v = vx; cmvy_v = vy; }
                        }
                    };
                    // x264_mb_predict_mv (R/common/macroblock.c:28-88) from the cache; cur_part = h->mb.i_partition
                    auto predict_blk = [&](int cur_part, int idx, int width, int &px, int &py) {
                        const int i8 = mb_scan8_luma(idx), i_ref = __builtin_amdgcn_readlane(cref_v, i8);
                        int ra = __builtin_amdgcn_readlane(cref_v, i8 - 1), rb = __builtin_amdgcn_readlane(cref_v, i8 - 8), rc = __builtin_amdgcn_readlane(cref_v, i8 - 8 + width), kc = i8 - 8 + width;
                        if ((idx & 3) == 3 || (width == 2 && (idx & 3) == 2) || rc == -2) { kc = i8 - 8 - 1; rc = __builtin_amdgcn_readlane(cref_v, kc); }
                        const int ax = __builtin_amdgcn_readlane(cmvx_v, i8 - 1), ay = __builtin_amdgcn_readlane(cmvy_v, i8 - 1), bx = __builtin_amdgcn_readlane(cmvx_v, i8 - 8), byv = __builtin_amdgcn_readlane(cmvy_v, i8 - 8);
                        const int cx = __builtin_amdgcn_readlane(cmvx_v, kc), cy = __builtin_amdgcn_readlane(cmvy_v, kc);
                        if (cur_part == D_16x8) {
                            if (idx == 0 && rb == i_ref) { px = bx; py = byv; return; }
                            if (idx != 0 && ra == i_ref) { px = ax; py = ay; return; }
                        } else if (cur_part == D_8x16) {
                            if (idx == 0 && ra == i_ref) { px = ax; py = ay; return; }
                            if (idx != 0 && rc == i_ref) { px = cx; py = cy; return; }
                        }
                        const int cnt = (ra == i_ref) + (rb == i_ref) + (rc == i_ref);
                        if (cnt > 1) { px = mb_median(ax, bx, cx); py = mb_median(ay, byv, cy); }
                        else if (cnt == 1) { if (ra == i_ref) { px = ax; py = ay; } else if (rb == i_ref) { px = bx; py = byv; } else { px = cx; py = cy; } }
                        else if (rb == -2 && rc == -2 && ra != -2) { px = ax; py = ay; }
                        else { px = mb_median(ax, bx, cx); py = mb_median(ay, byv, cy); }
                    };
                    int i_cost = best;
                    int c8x8 = MX_COST_MAX, c16x8 = MX_COST_MAX, c8x16 = MX_COST_MAX;   // a->l0.i_cost8x8 / i_cost16x8 / i_cost8x16
                    auto search_partitions = [&]() {
                    part = D_16x16;
                    if (a.flags_inter & 0x10) {
                        // ---- X264_ANALYSE_PSUB16x16: p8x8, then p16x8 / p8x16 (R/encoder/analyse.c:2222-2265) ----
                        cache_set(0, 0, 4, 4, ref, 0, 0, 0);
                        int cost8x8;
                        if (a.mixed_refs) {                          // x264_mb_analyse_inter_p8x8_mixed_ref, :1146-1219
                            int maxref = a.n_refs - 1;
                            const int tt = type_top == T_I_8x8 ? 0 : type_top, tl = left_type == T_I_8x8 ? 0 : left_type;   // as cache_save stores them
                            if (maxref > 0 && ref == 0 && tt && tl) {
                                maxref = 0;
                                maxref = max(maxref, __builtin_amdgcn_readlane(cref_v, 3)); maxref = max(maxref, __builtin_amdgcn_readlane(cref_v, 4)); maxref = max(maxref, __builtin_amdgcn_readlane(cref_v, 6));
                                maxref = max(maxref, __builtin_amdgcn_readlane(cref_v, 8)); maxref = max(maxref, __builtin_amdgcn_readlane(cref_v, 11)); maxref = max(maxref, __builtin_amdgcn_readlane(cref_v, 27));
                            }
                            bool multi = false;                      // every reference's search of a block at once (me_search_refs8)
                            if constexpr (RD && !BS) multi = maxref > 0 && mo.method == 1 && mo.subme >= 3;
                            for (int i = 0; i < 4; i++) {
                                int bcost = 0x7fffffff, bvx = 0, bvy = 0, bcm = 0, br = 0, bpx = 0, bpy = 0;
                                const int bx8 = 8 * (i & 1), by8 = 8 * (i >> 1);
                                for (int r0 = 0; multi && r0 <= maxref; r0 += 4) {      // four references (slots of 16 lanes) per pass
                                    const int nsl = min(maxref - r0 + 1, 4), slot = lane >> 4, j = lane & 15;
                                    // every reference's predictor first: x264_mb_predict_mv with only the block's cached reference changed.
                                    // A spare slot repeats the pass's first reference.
                                    int lpx = 0, lpy = 0;
                                    for (int t = 0; t < nsl; t++) {
                                        cache_set(2 * (i & 1), 2 * (i >> 1), 2, 2, r0 + t, 0, 0, 0);
                                        int px, py;
                                        predict_blk(13, 4 * i, 2, px, py);
                                        if (slot == t || (t == 0 && slot >= nsl)) { lpx = px; lpy = py; }
                                    }
                                    const bool live = slot < nsl;
                                    const int r = r0 + (live ? slot : 0);
                                    // lane j < 6 of a slot: plane j of its reference at the block (four half-pel planes, U, V)
                                    const u8 *pb = j < 4 ? refs.y[r][j & 3] : j == 4 ? refs.u[r] : refs.v[r];
                                    const uint64_t plv = j < 4 ? (uint64_t)(uintptr_t)(pb + by_ + oy + (ptrdiff_t)by8 * a.sy + bx8)
                                                               : (uint64_t)(uintptr_t)(pb + bc_ + oc + (ptrdiff_t)(by8 >> 1) * a.sc + (bx8 >> 1));
                                    c.set_block(8, 8, bx8, by8);
                                    int vx, vy, cm;
                                    LAUNDER(); c.lane = lane;
                                    const int cost = me_search_refs8(c, plv, L, mo, (MX_LDS(i16))&s.l0mvc[r][0][0], i + 1, live, lpx, lpy, vx, vy, cm);
                                    for (int t = 0; t < nsl; t++) {                  // the winner in reference order, strict '<'
                                        const int rt = r0 + t, ct = __builtin_amdgcn_readlane(cost, 16 * t) + (Q.lambda * refs.ref_bits[rt]);
                                        const int tvx = __builtin_amdgcn_readlane(vx, 16 * t), tvy = __builtin_amdgcn_readlane(vy, 16 * t);
                                        if (lane == 0) { s.l0mvc[rt][i + 1][0] = (i16)tvx; s.l0mvc[rt][i + 1][1] = (i16)tvy; }
                                        if (ct < bcost) {
                                            bcost = ct; bvx = tvx; bvy = tvy; bcm = __builtin_amdgcn_readlane(cm, 16 * t); br = rt;
                                            bpx = __builtin_amdgcn_readlane(lpx, 16 * t); bpy = __builtin_amdgcn_readlane(lpy, 16 * t);
                                        }
                                    }
                                    WAVE_SYNC();
                                }
                                for (int r = 0; !multi && r <= maxref; r++) {
                                    cache_set(2 * (i & 1), 2 * (i >> 1), 2, 2, r, 0, 0, 0);
                                    int px, py, vx, vy, cm;
                                    predict_blk(13, 4 * i, 2, px, py);
                                    aim(r, 8, 8, 8 * (i & 1), 8 * (i >> 1));
                                    c.mvpx = px; c.mvpy = py;
                                    LAUNDER(); c.lane = lane;
                                    int cost = me_search_ref16(c, L, mo, &s.l0mvc[r][0][0], i + 1, nullptr, vx, vy, cm) + (Q.lambda * refs.ref_bits[r]);
                                    if (lane == 0) { s.l0mvc[r][i + 1][0] = (i16)vx; s.l0mvc[r][i + 1][1] = (i16)vy; }
                                    WAVE_SYNC();
                                    if (cost < bcost) { bcost = cost; bvx = vx; bvy = vy; bcm = cm; br = r; bpx = px; bpy = py; }
                                }
                                cache_set(2 * (i & 1), 2 * (i >> 1), 2, 2, br, bvx, bvy, 1);
                                pme_put(i, bvx, bvy, bcost + Q.lambda, bcm, br, (Q.lambda * refs.ref_bits[br]), bpx, bpy);      // + lambda * i_sub_mb_p_cost_table[D_L0_8x8]
                            }
                            cost8x8 = pme(0, 2) + pme(1, 2) + pme(2, 2) + pme(3, 2);
                            if (!a.cabac && !(pme(0, 4) | pme(1, 4) | pme(2, 4) | pme(3, 4))) cost8x8 -= (Q.lambda * refs.ref_bits[0]) * 4;
                        } else {                                     // x264_mb_analyse_inter_p8x8, :1221-1272
                            const int r = ref, ref_cost = a.cabac || r ? (Q.lambda * refs.ref_bits[r]) : 0;
                            if (lane == 0) { s.l0mvc[r][0][0] = (i16)mvx; s.l0mvc[r][0][1] = (i16)mvy; }
                            WAVE_SYNC();
                            for (int i = 0; i < 4; i++) {
                                int px, py, vx, vy, cm;
                                predict_blk(13, 4 * i, 2, px, py);
                                aim(r, 8, 8, 8 * (i & 1), 8 * (i >> 1));
                                c.mvpx = px; c.mvpy = py;
                                LAUNDER(); c.lane = lane;
                                const int cost = me_search_ref16(c, L, mo, &s.l0mvc[r][0][0], i + 1, nullptr, vx, vy, cm);
                                cache_set(2 * (i & 1), 2 * (i >> 1), 2, 2, r, vx, vy, 1);
                                if (lane == 0) { s.l0mvc[r][i + 1][0] = (i16)vx; s.l0mvc[r][i + 1][1] = (i16)vy; }
                                pme_put(i, vx, vy, cost + ref_cost + Q.lambda, cm, r, ref_cost, px, py);
                            }
                            cost8x8 = pme(0, 2) + pme(1, 2) + pme(2, 2) + pme(3, 2);
                            if (a.cabac) cost8x8 -= ref_cost;
                        }
                        if (cost8x8 < best) { type = T_P_8x8; part = D_8x8; i_cost = cost8x8; }
                        if ((a.flags_inter & 0x20) && type == T_P_8x8) {
                            // ---- X264_ANALYSE_PSUB8x8 (R/encoder/analyse.c:2252-2277): p4x4, and only if that beats the 8x8 block, p8x4 and p4x8
                            // (:1407-1519).  Records (mv, cost, mvp) of me4x4[i][k] / me8x4[i][k] / me4x8[i][k] sit in lanes 4i+k / 16+2i+k / 24+2i+k.
                            MeOpts mo_sub = mo;
                            mo_sub.chroma_me = 0;                        // b_chroma_me && i_pixel <= PIXEL_8x8, me.c:654
                            for (int i = 0; i < 4; i++) {
                                const int r = pme(i, 4), x0 = 2 * (i & 1), y0 = 2 * (i >> 1);
                                int c8 = 0, subt = D_L0_8x8;
                                for (int t = 0; t < 3; t++) {
                                    const int sw = t == 1 ? 2 : 1, sh = t == 2 ? 2 : 1, sn = t == 0 ? 4 : 2, rec0 = t == 0 ? 4 * i : t == 1 ? 16 + 2 * i : 24 + 2 * i;
                                    const int cvx = t == 0 ? pme(i, 0) : __builtin_amdgcn_readlane(sub_mx, 4 * i), cvy = t == 0 ? pme(i, 1) : __builtin_amdgcn_readlane(sub_my, 4 * i);
                                    int sum = 0;
                                    for (int k = 0; k < sn; k++) {
                                        const int x4 = x0 + (t == 0 ? (k & 1) : t == 2 ? k : 0), y4 = y0 + (t == 0 ? (k >> 1) : t == 1 ? k : 0);
                                        const int idx = 4 * i + (y4 - y0) * 2 + (x4 - x0);
                                        int px, py, vx, vy, cm;
                                        predict_blk(13, idx, sw, px, py);
                                        aim(r, 4 * sw, 4 * sh, 4 * x4, 4 * y4);
                                        c.mvpx = px; c.mvpy = py;
                                        WAVE_SYNC();
                                        if (lane < 2) s.mvc[0][lane] = (i16)(lane ? cvy : cvx);
                                        WAVE_SYNC();
                                        LAUNDER(); c.lane = lane;
                                        const int cost = me_search_ref16(c, L, mo_sub, &s.mvc[0][0], k == 0 ? 1 : 0, nullptr, vx, vy, cm);
                                        if (lane == rec0 + k) { sub_mx = vx; sub_my = vy; sub_cost = cost; sub_px = px; sub_py = py; }
                                        cache_set(x4, y4, sw, sh, r, vx, vy, 1);
                                        sum += cost;
                                    }
                                    int cst = sum + (Q.lambda * refs.ref_bits[r]) + Q.lambda * (t == 0 ? 5 : 3);          // i_sub_mb_p_cost_table
                                    if (a.chroma_me && a.subme >= 5) cst += sw_sub_chroma(s, refs, a, r, i, t, rec0, sub_mx, sub_my, satd, oc, bc_, lane);
                                    if constexpr (SUB8) { if (lane == 4 * i + t) sub_cst = cst; }
                                    if (t == 0) {
                                        if (!(cst < pme(i, 2))) break;
                                        c8 = cst; subt = D_L0_4x4;
                                    } else if (cst < c8) { c8 = cst; subt = t; }
                                }
                                if (subt != D_L0_8x8) i_cost += c8 - pme(i, 2);
                                // x264_mb_cache_mv_p8x8
                                if (subt == D_L0_8x8) cache_set(x0, y0, 2, 2, r, pme(i, 0), pme(i, 1), 1);
                                else {
                                    const int sw = subt == D_L0_8x4 ? 2 : 1, sh = subt == D_L0_4x8 ? 2 : 1, sn = subt == D_L0_4x4 ? 4 : 2, rec0 = subt == D_L0_4x4 ? 4 * i : subt == D_L0_8x4 ? 16 + 2 * i : 24 + 2 * i;
                                    for (int k = 0; k < sn; k++)
                                        cache_set(x0 + (subt == D_L0_4x4 ? (k & 1) : subt == D_L0_4x8 ? k : 0), y0 + (subt == D_L0_4x4 ? (k >> 1) : subt == D_L0_8x4 ? k : 0), sw, sh, r,
                                                  __builtin_amdgcn_readlane(sub_mx, rec0 + k), __builtin_amdgcn_readlane(sub_my, rec0 + k), 1);
                                }
                                if (lane == i) sub_t = subt;
                            }
                            cost8x8 = i_cost;
                        }
                        const int thresh16x8 = pme(1, 3) + pme(2, 3);
                        if (cost8x8 < best + thresh16x8)
                            for (int dir = 0; dir < 2; dir++) {      // 0: x264_mb_analyse_inter_p16x8 (:1274), 1: _p8x16 (:1324)
                                int sum = 0;
                                for (int i = 0; i < 2; i++) {
                                    const int ra = dir ? pme(i, 4) : pme(2 * i, 4), rb = dir ? pme(i + 2, 4) : pme(2 * i + 1, 4), nr = ra == rb ? 1 : 2;
                                    int bcost = 0x7fffffff, bvx = 0, bvy = 0, bcm = 0, br = 0, bpx = 0, bpy = 0;
                                    for (int j = 0; j < nr; j++) {
                                        const int r = j ? rb : ra, k1 = dir ? i + 1 : 2 * i + 1, k2 = dir ? i + 3 : 2 * i + 2;
                                        WAVE_SYNC();
                                        if (lane < 6) {
                                            const int k = lane >> 1 == 0 ? 0 : lane >> 1 == 1 ? k1 : k2;
                                            s.mvc[lane >> 1][lane & 1] = s.l0mvc[r][k][lane & 1];
                                        }
                                        if (dir) cache_set(2 * i, 0, 2, 4, r, 0, 0, 0); else cache_set(0, 2 * i, 4, 2, r, 0, 0, 0);
                                        int px, py, vx, vy, cm;
                                        predict_blk(dir ? D_8x16 : D_16x8, dir ? 4 * i : 8 * i, dir ? 2 : 4, px, py);
                                        aim(r, dir ? 8 : 16, dir ? 16 : 8, dir ? 8 * i : 0, dir ? 0 : 8 * i);
                                        c.mvpx = px; c.mvpy = py;
                                        LAUNDER(); c.lane = lane;
                                        const int cost = me_search_ref16(c, L, mo, &s.mvc[0][0], 3, nullptr, vx, vy, cm) + (Q.lambda * refs.ref_bits[r]);
                                        if (cost < bcost) { bcost = cost; bvx = vx; bvy = vy; bcm = cm; br = r; bpx = px; bpy = py; }
                                    }
                                    if (dir) cache_set(2 * i, 0, 2, 4, br, bvx, bvy, 1); else cache_set(0, 2 * i, 4, 2, br, bvx, bvy, 1);
                                    pme_put(4 + 2 * dir + i, bvx, bvy, bcost, bcm, br, (Q.lambda * refs.ref_bits[br]), bpx, bpy);
                                    sum += bcost;
                                }
                                if (dir) c8x16 = sum; else c16x8 = sum;
                                if (sum < i_cost) { i_cost = sum; type = T_P_L0; part = dir ? D_8x16 : D_16x8; }
                            }
                        c8x8 = cost8x8;
                    }
                    };
                    // x264_me_refine_qpel on the winning partition (analyse.c:2289-2352); the reference cost leaves every block's sum (me.c:639-640)
                    auto refine_winner = [&]() {
                    if (part == D_16x16) {
                        aim(ref, 16, 16, 0, 0);
                        c.mvpx = bmvpx; c.mvpy = bmvpy;
                        best -= (Q.lambda * refs.ref_bits[ref]);
                        LAUNDER(); c.lane = lane;
                        best = me_refine_qpel16(c, L, mo, best, mvx, mvy);
                        i_cost = best;
                        if (lane < 16) { s.mv4[lane][0] = (i16)mvx; s.mv4[lane][1] = (i16)mvy; }
                        if (lane < 4) s.ref8[lane] = (signed char)ref;
                    } else {
                        i_cost = 0;
                        const int nblk = part == D_8x8 ? 4 : 2, slot0 = part == D_8x8 ? 0 : part == D_16x8 ? 4 : 6;
                        for (int i = 0; i < nblk; i++) {
                            // an 8x8 block of a P_8x8 macroblock refines its sub-partitions (analyse.c:2317-2352): no reference cost in their
                            // sums and no chroma (me.c:639, :654)
                            const int subt = part == D_8x8 ? __builtin_amdgcn_readlane(sub_t, i) : D_L0_8x8, nj = subt == D_L0_8x8 ? 1 : subt == D_L0_4x4 ? 4 : 2;
                            for (int k = 0; k < nj; k++) {
                                int bx = part == D_8x8 ? 8 * (i & 1) : part == D_8x16 ? 8 * i : 0, by = part == D_8x8 ? 8 * (i >> 1) : part == D_16x8 ? 8 * i : 0;
                                int w = part == D_16x8 ? 16 : 8, h = part == D_8x16 ? 16 : 8;
                                const int r = pme(slot0 + i, 4);
                                int vx = pme(slot0 + i, 0), vy = pme(slot0 + i, 1), cin = pme(slot0 + i, 2) - pme(slot0 + i, 5);
                                MeOpts mo_r = mo;
                                c.mvpx = pme(slot0 + i, 6); c.mvpy = pme(slot0 + i, 7);
                                if (subt != D_L0_8x8) {
                                    const int rec = (subt == D_L0_4x4 ? 4 * i : subt == D_L0_8x4 ? 16 + 2 * i : 24 + 2 * i) + k;
                                    bx += 4 * (subt == D_L0_4x4 ? (k & 1) : subt == D_L0_4x8 ? k : 0); by += 4 * (subt == D_L0_4x4 ? (k >> 1) : subt == D_L0_8x4 ? k : 0);
                                    w = subt == D_L0_8x4 ? 8 : 4; h = subt == D_L0_4x8 ? 8 : 4;
                                    vx = __builtin_amdgcn_readlane(sub_mx, rec); vy = __builtin_amdgcn_readlane(sub_my, rec); cin = __builtin_amdgcn_readlane(sub_cost, rec);
                                    c.mvpx = __builtin_amdgcn_readlane(sub_px, rec); c.mvpy = __builtin_amdgcn_readlane(sub_py, rec);
                                    mo_r.chroma_me = 0;
                                }
                                aim(r, w, h, bx, by);
                                LAUNDER(); c.lane = lane;
                                i_cost += me_refine_qpel16(c, L, mo_r, cin, vx, vy);
                                WAVE_SYNC();
                                if (lane < 16) {
                                    const int x4 = (lane & 3) * 4, y4 = (lane >> 2) * 4;
                                    if (x4 >= bx && x4 < bx + w && y4 >= by && y4 < by + h) { s.mv4[lane][0] = (i16)vx; s.mv4[lane][1] = (i16)vy; }
                                }
                                if (lane < 4) {
                                    const int x8 = (lane & 1) * 8, y8 = (lane >> 1) * 8;
                                    if (x8 >= (bx & ~7) && x8 < (bx & ~7) + (w < 8 ? 8 : w) && y8 >= (by & ~7) && y8 < (by & ~7) + (h < 8 ? 8 : h)) s.ref8[lane] = (signed char)r;
                                }
                            }
                        }
                    }
                    };
                    if constexpr (!RD) {
                    search_partitions();
                    refine_winner();
                    WAVE_SYNC();
                    if (part == D_8x8) sub_t_mb = sub_t;
                    PROF(2);
                    LAUNDER();
                    if (a.chroma_me) {
                        analyse_chroma();
                        analyse_intra(i_cost - satd_chroma);
                        satd_i16 += satd_chroma; satd_i8 += satd_chroma; satd_i4 += satd_chroma;
                    } else
                        analyse_intra(i_cost);
                    if (fi_open) {
                        if (min(satd_i8, satd_i4) < i_cost) {        // the answer decides the macroblock type: it must be exact
                            if (fast_intra_now(1)) satd_i8 = satd_i4 = MX_COST_MAX;
                            fi_open = 0;
                        } else
                            stat_alt = satd_i16;                     // i_intra_cost if b_fast_intra turns out to be 1
                    }
                    // analyse.c:2372-2400: best intra type (16x16, then 8x8, then 4x4 on strict improvement) against inter
                    int itype = T_I_16x16, icost = satd_i16;
                    if (satd_i8 < icost) { icost = satd_i8; itype = T_I_8x8; }
                    if (satd_i4 < icost) { icost = satd_i4; itype = T_I_4x4; }
                    if (icost < i_cost) { i_cost = icost; type = itype; }
                    stat_intra = icost; analysed = 1;
                    stat_inter = i_cost;
                    } else {
                        // ---- the raster variant's P macroblock (analyse.c:2228-2405): the rest of the analysis, the RD candidates of
                        // x264_mb_analyse_p_rd / x264_mb_analyse_transform_rd / x264_intra_rd, and the final encode, through ONE copy of
                        // x264_rd_cost_mb: step 0 the early 16x16 trial (:1134-1143), 1 the analysis, 2-5 p_rd, 6 the transform, 7-9 intra, 10 final.
                        int me16x = mvx, me16y = mvy;                    // (the RD refinement moves the 16x16 vector)
                        const int me16r = ref;
                        int i8_cbp_rd = 0;                               // a->i_cbp_i8x8_luma (x264_intra_rd, analyse.c:869)
                        // the RD refinement's state (slice_refine.h): what is being refined, the best cost so far, and the candidate generator of
                        // x264_me_refine_qpel_rd
                        int rf_kind = 0, rf_i = 0, rf_n = 0, rf_old16 = 0, rf_best16 = 0, rf_thr = 0;
                        u32 rf_list = 0;
                        unsigned long long rf_best = 0;
                        int rf_sub = 0, rf_k = 0;       // (SUB8) the sub-partitions of step 5 are chosen; the sub-block the refinement is at
                        (void)rf_sub; (void)rf_k;
                        int q_st = 0, q_j = 0, q_it = 0, q_dir = -2, q_odir = 0, q_tag = 0, q_after_pm = 0;
                        int q_bmx = 0, q_bmy = 0, q_omx = 0, q_omy = 0, q_pmx = 0, q_pmy = 0, q_m0x = 0, q_m0y = 0, q_mvpx = 0, q_mvpy = 0, q_cx = 0, q_cy = 0;
                        int q_pix = 0, q_bx = 0, q_by = 0, q_w = 16, q_h = 16, q_slot = -1, q_ref = 0, q_i4 = 0, q_satds = 0;
                        u32 q_bsatd = 0;
                        (void)rf_kind; (void)rf_i; (void)rf_n; (void)rf_old16; (void)rf_best16; (void)rf_thr; (void)rf_list; (void)rf_best; (void)i8_cbp_rd;
                        (void)q_st; (void)q_j; (void)q_it; (void)q_dir; (void)q_odir; (void)q_tag; (void)q_after_pm; (void)q_bmx; (void)q_bmy; (void)q_omx; (void)q_omy;
                        (void)q_pmx; (void)q_pmy; (void)q_m0x; (void)q_m0y; (void)q_mvpx; (void)q_mvpy; (void)q_cx; (void)q_cy; (void)q_pix; (void)q_bx; (void)q_by;
                        (void)q_w; (void)q_h; (void)q_slot; (void)q_ref; (void)q_i4; (void)q_satds; (void)q_bsatd;
                        int rd16 = MX_COST_MAX, satd_inter = 0, satd_intra = 0, final_type = T_P_L0, final_part = 16, rd_thresh = 0, rd_isat = 0;
                        bool rd_skip = false;
                        // x264_analyse_update_cache for a P candidate (analyse.c:2803-2846): type / part -> s.mv4 / s.ref8 (and the 16x16 scalars)
                        auto update_cache_p = [&]() {
                            if (type == T_P_SKIP) return;                        // encode_pskip sets the skip vector itself
                            const int bx4 = lane & 3, by4 = (lane >> 2) & 3, bx8 = lane & 1, by8 = (lane >> 1) & 1;
                            const int slot = part == D_16x8 ? 4 + (by4 >> 1) : part == D_8x16 ? 6 + (bx4 >> 1) : (by4 >> 1) * 2 + (bx4 >> 1);
                            const int slot8 = part == D_16x8 ? 4 + by8 : part == D_8x16 ? 6 + bx8 : by8 * 2 + bx8;
                            int vx = __shfl(pme_v, slot * 8 + 0, 64), vy = __shfl(pme_v, slot * 8 + 1, 64), vr = __shfl(pme_v, slot8 * 8 + 4, 64);
                            if (part == D_16x16) { vx = me16x; vy = me16y; vr = me16r; }
                            if constexpr (SUB8) {
                                // x264_mb_cache_mv_p8x8: an 8x8 block with sub-partitions takes its vectors from the records of its type (sub_t)
                                if (part == D_8x8 && (a.flags_inter & 0x20)) {
                                    const int i8 = (by4 >> 1) * 2 + (bx4 >> 1), st = __shfl(sub_t, i8, 64);
                                    const int rec = st == D_L0_4x4 ? 4 * i8 + (by4 & 1) * 2 + (bx4 & 1) : st == D_L0_8x4 ? 16 + 2 * i8 + (by4 & 1) : 24 + 2 * i8 + (bx4 & 1);
                                    const int sx = __shfl(sub_mx, rec, 64), sy = __shfl(sub_my, rec, 64);
                                    if (st != D_L0_8x8) { vx = sx; vy = sy; }
                                }
                            }
                            if (lane < 16) { s.mv4[lane][0] = (i16)vx; s.mv4[lane][1] = (i16)vy; }
                            if (lane < 4) s.ref8[lane] = (signed char)vr;
                            {   // the motion cache's copy of block 12 (raster block 10, 8x8 block 3) follows the candidate
                                const int nx = __shfl(vx, 10, 64), ny = __shfl(vy, 10, 64), nr = __shfl(vr, 3, 64);
                                if (lane == 30) { cref_v = nr; cmvx_v = nx; cmvy_v = ny; }
                            }
                            mvx = me16x; mvy = me16y; ref = me16r;
                            WAVE_SYNC();
                        };
#pragma nounroll
                        for (int step = 0; step < (RF ? 13 : 11); step++) {      // RF: 10 decides, 11 refines (once per full-macroblock candidate), 12 is the final encode
                            bool fin = false;
                            if (step == 0) {
                                if (!mbrd) continue;
                                cache_fenc_satd();
                                if (!is_p || !(me16r == 0 && me16x == pskx && me16y == psky)) continue;
                                type = T_P_L0; part = D_16x16;
                            } else if (step == 1) {
                                if (rd_skip) { step = 9; continue; }
                                int intra_thresh = MX_COST_MAX;              // an I slice: x264_mb_analyse_intra(h, &analysis, COST_MAX), analyse.c:2175
                                if (is_p) {
                                    type = T_P_L0;
                                    search_partitions();
                                    if (!mbrd) refine_winner();
                                    WAVE_SYNC();
                                    if (part == D_8x8) sub_t_mb = sub_t;
                                    PROF(2);
                                    LAUNDER();
                                    final_type = type; final_part = part;
                                    intra_thresh = i_cost;
                                    if (a.chroma_me) { analyse_chroma(); intra_thresh = i_cost - satd_chroma; }
                                }
                                analyse_intra(intra_thresh);
                                if (is_p && a.chroma_me) { satd_i16 += satd_chroma; satd_i8 += satd_chroma; satd_i4 += satd_chroma; }
                                satd_inter = i_cost; satd_intra = min(min(satd_i16, satd_i8), satd_i4);
                                if (!mbrd) { step = 9; continue; }
                                rd_isat = min(satd_inter, satd_intra); rd_thresh = rd_isat * 5 / 4;
                                type = T_P_L0;
                                if (!is_p) step = 6;                         // an I slice: straight to x264_intra_rd (:2177)
                                continue;
                            } else if (step == 2) {
                                if (!(rd16 == MX_COST_MAX && best <= rd_isat * 3 / 2)) continue;
                                part = D_16x16;
                            } else if (step == 3) {
                                if (!(c16x8 <= rd_thresh)) { c16x8 = MX_COST_MAX; continue; }
                                part = D_16x8;
                            } else if (step == 4) {
                                if (!(c8x16 <= rd_thresh)) { c8x16 = MX_COST_MAX; continue; }
                                part = D_8x16;
                            } else if (step == 5) {
                                if (!(c8x8 <= rd_thresh)) { c8x8 = MX_COST_MAX; continue; }
                                type = T_P_8x8; part = D_8x8;
                                if constexpr (SUB8) {
                                    // X264_ANALYSE_PSUB8x8 (analyse.c:1966-1996): every 8x8 block's sub-partition by x264_rd_cost_part first -- in
                                    // slice_refine.h (rf_kind 4), where the one copy of the partial encode is; it comes back here with rf_sub set
                                    if ((a.flags_inter & 0x20) && !rf_sub) { rf_kind = 4; rf_i = 0; q_st = 0; step = 10; continue; }
                                }
                            } else if (step == 6) {
                                final_type = T_P_L0; final_part = 16; i_cost = rd16;
                                if (c16x8 < i_cost) { i_cost = c16x8; final_part = 14; }
                                if (c8x16 < i_cost) { i_cost = c8x16; final_part = 15; }
                                if (c8x8 < i_cost) { i_cost = c8x8; final_part = 13; final_type = T_P_8x8; }
                                type = final_type; part = final_part;
                                if (!(i_cost < MX_COST_MAX) || !a.transform8x8) continue;        // x264_mb_analyse_transform_rd, :2127-2150
                                if constexpr (SUB8) {                    // x264_mb_transform_8x8_allowed: not with a sub-partition below 8x8
                                    if (type == T_P_8x8) { sub_t_mb = sub_t; if (__ballot(lane < 4 && sub_t != D_L0_8x8) != 0) continue; }
                                }
                                t8 = !t8;
                            } else if (step == 7) {                                                // x264_intra_rd, :845-874 (threshold COST_MAX in an I slice)
                                if (!(satd_i16 <= (is_p ? satd_inter * 5 / 4 : MX_COST_MAX))) { satd_i16 = MX_COST_MAX; continue; }
                                type = T_I_16x16;
                            } else if (step == 8) {
                                if (!(satd_i4 <= (is_p ? satd_inter * 5 / 4 : MX_COST_MAX) && satd_i4 < MX_COST_MAX)) { satd_i4 = MX_COST_MAX; continue; }
                                type = T_I_4x4;
                            } else if (step == 9) {
                                if (!(satd_i8 <= (is_p ? satd_inter * 5 / 4 : MX_COST_MAX) && satd_i8 < MX_COST_MAX)) { satd_i8 = MX_COST_MAX; continue; }
                                type = T_I_8x8;
                            } else if (!RF || step == 10) {
                                fin = !RF;
                                if (!is_p) {                                 // analyse.c:2179-2184: 16x16, then 4x4, then 8x8, then PCM on strict improvement
                                    type = T_I_16x16;
                                    int ic = satd_i16;
                                    if (satd_i4 < ic) { ic = satd_i4; type = T_I_4x4; }
                                    if (satd_i8 < ic) { ic = satd_i8; type = T_I_8x8; }
                                    if (satd_pcm < ic) type = T_I_PCM;
                                } else if (rd_skip) type = T_P_SKIP;
                                else {
                                    // analyse.c:2391-2404: best intra type (16x16, then 8x8, then 4x4, then PCM on strict improvement) against inter
                                    int itype = T_I_16x16, icost = satd_i16;
                                    if (satd_i8 < icost) { icost = satd_i8; itype = T_I_8x8; }
                                    if (satd_i4 < icost) { icost = satd_i4; itype = T_I_4x4; }
                                    if (satd_pcm < icost) { icost = satd_pcm; itype = T_I_PCM; }
                                    type = final_type; part = final_part;
                                    if (icost < i_cost) { i_cost = icost; type = itype; }
                                    if (icost == MX_COST_MAX) icost = i_cost * satd_intra / satd_inter + 1;
                                    stat_intra = icost; analysed = 1;
                                    stat_inter = i_cost;
                                }
                                if constexpr (RF) {
                                    // analyse.c:2184-2185 (I), :2406-2464 (P): with a->i_mbrd >= 2 the winner's intra modes / vectors are refined by RD
                                    rf_kind = 9;
                                    if (mbrd >= 2 && type != T_I_PCM && !rd_skip) {
                                        if (IS_INTRA_T(type)) {
                                            skip_intra = 0;                  // x264_intra_rd_refine's first statement
                                            rf_kind = 2;
                                            if (type == T_I_16x16) {
                                                rf_kind = 1; rf_list = sw_modes16(nb, rf_n); rf_i = 0; rf_old16 = rf_best16 = pred16;
                                                rf_thr = UNI(sf.i16dir[pred16]) * 9 / 8; rf_best = (unsigned long long)(u32)satd_i16;
                                            }
                                        } else { rf_kind = 3; rf_i = 0; q_st = -1; }
                                    }
                                    continue;
                                } else {
                                    tq.on = rd.trellis != 0;                                      // :2768-2773
                                    if (rd.trellis == 1 || a.nr) skip_intra = 0;
                                }
                            } else if (step == 11) {
                                if constexpr (RF) {
#include "slice_refine.h"
                                }
                            } else {
                                fin = true;
                                tq.on = rd.trellis != 0;                                          // :2768-2773
                                if (rd.trellis == 1 || a.nr) skip_intra = 0;
                            }
                            // x264_analyse_update_cache (:2763 for the final type), then the encoder: the trial of x264_rd_cost_mb
                            // (R/encoder/rdo.c:139-171) or the real thing
                            if ((!fin || mbrd) && !IS_INTRA_T(type)) update_cache_p();
                            const int t8_bak = t8;
                            PROF(6);
                            if (!(fin && type == T_I_PCM)) encode_mb(fin ? 1 : 0);
                            else psy_after_analysis();               // I_PCM is not a skip: the arrays are refreshed, nothing is quantised
                            if (fin) { encoded = true; break; }
                            PROF(0);
                            // distortion, and the syntax priced against a copy of the live contexts.  Like the reference this leaves `type`
                            // as the encode left it (P_SKIP when nothing was left to code on the skip vector).
                            int c = ssd_mb();
                            if (type == T_P_SKIP) c += (Q.lambda2 + 128) >> 8;
                            else {
                                const int f8 = price_mb();
                                c += (int)(((unsigned long long)(u32)f8 * (u32)Q.lambda2 + 32768) >> 16);
                            }
                            t8 = t8_bak;
                            PROF(7);
                            if (step == 0) { rd16 = c; if (type == T_P_SKIP) rd_skip = true; }
                            else if (step == 2) rd16 = c;
                            else if (step == 3) c16x8 = c;
                            else if (step == 4) c8x16 = c;
                            else if (step == 5) c8x8 = c;
                            else if (step == 6) {
                                if (i_cost >= c) {
                                    if (i_cost > 0) satd_inter = (int)((long long)satd_inter * c / i_cost);
                                    if (satd_inter == 0) satd_inter = 1;
                                    i_cost = c;
                                } else
                                    t8 = !t8;
                            } else if (step == 7) satd_i16 = c;
                            else if (step == 8) satd_i4 = c;
                            else if (step == 9) { satd_i8 = c; i8_cbp_rd = cbp_luma; }
                            else if constexpr (RF) {                     // step 11: the full-macroblock candidate the refinement asked for
                                if (rf_kind == 1) { if ((unsigned long long)(u32)c < rf_best) { rf_best = (unsigned long long)(u32)c; rf_best16 = pred16; } }
                                else {
                                    type = T_P_L0;                       // x264_rd_cost_part( .., PIXEL_16x16 ) restores h->mb.i_type (rdo.c:209-213)
                                    if ((unsigned long long)(u32)c < rf_best) { rf_best = (unsigned long long)(u32)c; q_bmx = q_cx; q_bmy = q_cy; if (q_tag != -3) q_dir = q_tag; }
                                }
                                step = 10;                               // back into the refinement
                            }
                        }
                    }
                }
            }
            if constexpr (RD) {     // what the next macroblock finds in the cache's entry of block 12 (oracle/slice_oracle.c: stale_ref)
                if (is_p && rd.stale) {
                    if (type == T_P_SKIP) { st0r = 0; st0x = pskx; st0y = psky; }
                    else if (!IS_INTRA_T(type) && encoded) { st0r = UNI(s.ref8[3]); st0x = UNI(s.mv4[10][0]); st0y = UNI(s.mv4[10][1]); }
                    else { st0r = __builtin_amdgcn_readlane(cref_v, 30); st0x = __builtin_amdgcn_readlane(cmvx_v, 30); st0y = __builtin_amdgcn_readlane(cmvy_v, 30); }
                }
            }
        }
        (void)analysed;
        if constexpr (!RD) PROF(6);
        LAUNDER();

        // ---- x264_analyse_update_cache + x264_macroblock_encode ----
        if constexpr (!RD) encode_mb(1);
        else if (!encoded) encode_pskip();                     // the fast / early P_SKIP exits of the analysis
        const int intra = IS_INTRA_T(type);
        int mb_qp = Q.qp, cbp_store = 0;
        if constexpr (RD) {
            PROF(3);
            if (type == T_I_PCM) {          // the samples themselves are sent: the reconstruction is the source (R/encoder/cabac.c:801-818)
                *(u32 *)(s.fd + FDY + (lane >> 2) * FD + (lane & 3) * 4) = *(const u32 *)(s.fe + (lane >> 2) * 16 + (lane & 3) * 4);
                s.fd[FDU + (lane >> 3) * FD + (lane & 7)] = s.fe[256 + lane]; s.fd[FDV + (lane >> 3) * FD + (lane & 7)] = s.fe[320 + lane];
                cbp_luma = 0xf; cbp_chroma = 2; t8 = 0;
                WAVE_SYNC();
            }
            // ---- the entropy coder, where x264_slice_write has it (R/encoder/encoder.c:1192-1205) ----
            if (rd.write) {
                syn_prepare();
                const MbSynDev y0 = make_syn();
                if (lane == 0) {
                    if (mb > 0) cd_encode_terminal(cab);
                    if (IS_SKIP_T(type)) cw_mb_skip(cab, sr.cabac, left_type, type_top, 1, a.slice_type);
                    else {
                        if (is_p || BS) cw_mb_skip(cab, sr.cabac, left_type, type_top, 0, a.slice_type);
                        MbSynDev y = y0;
                        cw_macroblock(cab, sr.cabac, 0, y, s.fe, rd.i_frame + bz * rd.i_frame_stride);
                        sr.tmp_i[1] = y.qp;
                    }
                    const int pos = cd_pos(cab, payload0);
                    if (rd.mb_bits) rd.mb_bits[cb + mb] = pos;
                    sr.tmp_i[2] = (pos >> 3) + SW_MB_BYTES_MAX + 64 > rd.payload_cap;      // the next macroblock (and the flush) may not fit
                }
                WAVE_SYNC();
                if (UNI(sr.tmp_i[2])) {          // out of payload space: never write past the chain's buffer; the frame is reported aborted
                    if (lane == 0) { __hip_atomic_store(a.abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); atomicAdd(a.abort_total, 1); }
                    return;
                }
                if (!IS_SKIP_T(type)) mb_qp = UNI(sr.tmp_i[1]);
            } else if (type == T_I_16x16 && !(cbp_luma | cbp_chroma) && !UNI((int)s.nnz[24])) {
                // a slice without the writer in the loop is written after the sweep (x264hip_cavlc_write_frame, x264hip_cabac_write_frame), but the
                // side effect of either writer's mb_qp_delta belongs here: an I_16x16 macroblock without any coefficient takes the previous QP
                // (R/encoder/cavlc.c:205-211, R/encoder/cabac.c:270-276), which the next macroblock's QP rule and the loop filter read
                mb_qp = last_qp;
            }
            // x264_macroblock_cache_save's QP rules (R/common/macroblock.c:1244-1272): a macroblock without coefficients has no QP of its own
            if (SUB8 && type == T_I_PCM) {
                // the cache keeps the last trial's counts for the next macroblock (x264_macroblock_encode clears the luma DC's and returns); the 16s
                // x264_macroblock_cache_save reports go to the frame's arrays alone, below
                mb_qp = 0; last_dqp = 0; if (lane == 24) s.nnz[24] = 0; WAVE_SYNC();
            } else
            if (type == T_I_PCM) { mb_qp = 0; last_dqp = 0; if (lane < 27) s.nnz[lane] = 16; WAVE_SYNC(); }
            else {
                if (type != T_I_16x16 && cbp_luma == 0 && cbp_chroma == 0) mb_qp = last_qp;
                last_dqp = mb_qp - last_qp; last_qp = mb_qp;
            }
        }
        if (cbp_luma == 0 && type != T_I_8x8) t8 = 0;           // x264_macroblock_cache_save, R/common/macroblock.c:1273-1275
        PROF(RD ? 5 : 3);
        LAUNDER();

        // ---- x264_macroblock_cache_save: reconstruction, per-macroblock state, levels ----
        {
            const int r = lane >> 2, x = (lane & 3) * 4;
            *(u32 *)(a.dy + oy + (ptrdiff_t)r * a.sy + x) = *(const u32 *)(s.fd + FDY + r * FD + x);
            if (lane < 32) {
                const int chn = lane >> 4, l = lane & 15, cr = l >> 1, cx4 = (l & 1) * 4;
                *(u32 *)((chn ? a.dv : a.du) + oc + (ptrdiff_t)cr * a.sc + cx4) = *(const u32 *)(s.fd + (chn ? FDV : FDU) + cr * FD + cx4);
            }
        }
        if (lane < 16) {
            a.mv[((size_t)mb * 16 + lane) * 2] = (i16)(intra ? 0 : s.mv4[lane][0]);
            a.mv[((size_t)mb * 16 + lane) * 2 + 1] = (i16)(intra ? 0 : s.mv4[lane][1]);
            if ((lane & 3) == 3) { s.left_mv4[lane >> 2][0] = (i16)(intra ? 0 : s.mv4[lane][0]); s.left_mv4[lane >> 2][1] = (i16)(intra ? 0 : s.mv4[lane][1]); }
            const bool i48 = type == T_I_4x4 || type == T_I_8x8;
            a.i4mode[(size_t)mb * 16 + lane] = i48 ? s.i4c[mb_scan8_luma(lane)] : (signed char)2;
            if (lane == 5 || lane == 7 || lane == 13 || lane == 15)       // what the next macroblock sees to its left
                s.left_i4[lane == 5 ? 0 : lane == 7 ? 1 : lane == 13 ? 2 : 3] = i48 ? s.i4c[mb_scan8_luma(lane)] : (signed char)2;
        }
        if (lane < 4) {
            const signed char rv = (signed char)(is_p || BS ? (intra ? -1 : s.ref8[lane]) : -1);
            a.ref[(size_t)mb * 4 + lane] = rv;
            if (lane & 1) s.left_r8[lane >> 1] = rv;
        }
        if (lane < 27) (a.nnz + 27 * cb)[(size_t)mb * 27 + lane] = IS_SKIP_T(type) ? (u8)0 : SUB8 && type == T_I_PCM ? (u8)16 : s.nnz[lane];
        if (lane < 4) (a.sub_partition + 4 * cb)[(size_t)mb * 4 + lane] = (signed char)(type == T_P_8x8 ? sub_t_mb : BS && type == T_B_8x8 ? (int)sb.sub[lane] : 0);
        if constexpr (BS) {     // list 1 of x264_macroblock_cache_save, h->mb.skipbp, and what the next macroblock sees to its left
            if (lane < 16) {
                const i16 vx = (i16)(intra ? 0 : sb.mv4_1[lane][0]), vy = (i16)(intra ? 0 : sb.mv4_1[lane][1]);
                (rd.mv1 + 32 * cb)[((size_t)mb * 16 + lane) * 2] = vx; (rd.mv1 + 32 * cb)[((size_t)mb * 16 + lane) * 2 + 1] = vy;
                if ((lane & 3) == 3) { sb.left_mv4_1[lane >> 2][0] = vx; sb.left_mv4_1[lane >> 2][1] = vy; }
            }
            if (lane < 4) {
                const signed char rv1 = (signed char)(intra ? -1 : sb.ref8_1[lane]);
                (rd.ref1 + 4 * cb)[(size_t)mb * 4 + lane] = rv1;
                if (lane & 1) sb.left_r8_1[lane >> 1] = rv1;
            }
            if (lane == 0) {
                const int sbp = type == T_B_SKIP || type == T_B_DIRECT ? 0xf
                              : type == T_B_8x8 ? (sb.sub[0] == D_DIRECT_8x8) | (sb.sub[1] == D_DIRECT_8x8) << 1 | (sb.sub[2] == D_DIRECT_8x8) << 2 | (sb.sub[3] == D_DIRECT_8x8) << 3 : 0;
                (rd.skipbp + cb)[mb] = (u8)sbp; sb.left_skipbp = (u8)sbp;
            }
        }
        if (lane == 0) {
            const int cbp_dc = a.cabac ? (s.nnz[24] | s.nnz[25] << 1 | s.nnz[26] << 2) : 0;
            a.mb_type[mb] = (signed char)type;
            (a.partition + cb)[mb] = (signed char)(intra || IS_SKIP_T(type) || (BS && type == T_B_DIRECT) ? D_16x16 : part);
            (a.i16mode + cb)[mb] = (signed char)(type == T_I_16x16 ? pred16 : 0);
            (a.chroma_mode + cb)[mb] = (signed char)(intra ? predc : 0);
            (a.qp_out + cb)[mb] = (signed char)mb_qp;
            (a.t8 + cb)[mb] = (signed char)t8;
            (a.cbp + cb)[mb] = (i16)(IS_SKIP_T(type) ? 0 : type == T_I_PCM ? 0x72f : (cbp_dc << 8) | (cbp_chroma << 4) | cbp_luma);
            (a.cost_intra + cb)[mb] = stat_intra; (a.cost_inter + cb)[mb] = stat_inter; (a.cost_alt + cb)[mb] = stat_alt;
        }
        if (a.luma) {   // coefficient levels, masked by what the entropy coder reads (cbp, then nnz); a state without level arrays (the payload is the product) skips them
            const bool coded = !IS_SKIP_T(type) && type != T_I_PCM;
            i16 *ly = (a.luma + 256 * cb) + (size_t)mb * 256, *cac = (a.chroma_ac + 128 * cb) + (size_t)mb * 128;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int i = lane + 64 * k, blk = i >> 4;
                ly[i] = (coded && ((cbp_luma >> (blk >> 2)) & 1) && s.nnz[blk]) ? (t8 ? s.lv_y8[i] : s.lv_y[i]) : (i16)0;
            }
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int i = lane + 64 * k, blk = i >> 4;
                cac[i] = (coded && cbp_chroma == 2 && s.nnz[16 + blk]) ? s.lv_cac[i] : (i16)0;
            }
            if (lane < 16) (a.luma_dc + 16 * cb)[(size_t)mb * 16 + lane] = (coded && type == T_I_16x16 && s.nnz[24]) ? s.lv_dc[lane] : (i16)0;
            if (lane < 8) (a.chroma_dc + 8 * cb)[(size_t)mb * 8 + lane] = (coded && cbp_chroma && s.nnz[25 + (lane >> 2)]) ? s.lv_cdc[lane] : (i16)0;
        }
        if constexpr (RD) {     // what the next macroblock's entropy coding reads of this one (kept in LDS / registers), and mvd for the row below
            const int cbp_dc = s.nnz[24] | s.nnz[25] << 1 | s.nnz[26] << 2;
            cbp_store = IS_SKIP_T(type) ? 0 : type == T_I_PCM ? 0x72f : (UNI(cbp_dc) << 8) | (cbp_chroma << 4) | cbp_luma;
            const bool keep = !intra && !IS_SKIP_T(type) && !(BS && type == T_B_DIRECT);
            if (lane < 16) {
                const int k = 12 + (lane & 3) + 8 * (lane >> 2);
                i16 *mvd = rd.mvd + ((cb + mb) * 16 + lane) * 2;
                mvd[0] = keep ? sr.cmvd[k][0] : (i16)0; mvd[1] = keep ? sr.cmvd[k][1] : (i16)0;
                if ((lane & 3) == 3) { sr.left_mvd[lane >> 2][0] = mvd[0]; sr.left_mvd[lane >> 2][1] = mvd[1]; }
                if constexpr (BS) {
                    i16 *mvd1 = rd.mvd1 + ((cb + mb) * 16 + lane) * 2;
                    mvd1[0] = keep ? sb.cmvd1[k][0] : (i16)0; mvd1[1] = keep ? sb.cmvd1[k][1] : (i16)0;
                    if ((lane & 3) == 3) { sb.left_mvd1[lane >> 2][0] = mvd1[0]; sb.left_mvd1[lane >> 2][1] = mvd1[1]; }
                }
            } else if (lane < 24) {
                const int j = lane - 16;
                const int idx = j < 4 ? (j == 0 ? 5 : j == 1 ? 7 : j == 2 ? 13 : 15) : 16 + 4 * ((j - 4) >> 1) + 1 + 2 * (j & 1);
                sr.left_nz[j] = IS_SKIP_T(type) ? (u8)0 : SUB8 && type == T_I_PCM ? (u8)16 : s.nnz[idx];
            }
            left_cbp = cbp_store; left_cpm = intra && type != T_I_PCM ? sw_fix8c(predc) : 0; left_t8 = t8;
            prev_coded = type == T_I_16x16 || (cbp_store & 0x3f);
            intra_before += intra;
            WAVE_SYNC();
        }
        left_type = type;
        left_ref = is_p || BS ? (intra ? -1 : UNI(s.ref8[1])) : -1; left_mvx = intra ? 0 : UNI(s.mv4[3][0]); left_mvy = intra ? 0 : UNI(s.mv4[3][1]);
        PROF(4);
        LAUNDER();
        if constexpr (!RD) {
        // ---- publish: everything this macroblock wrote is visible before the count moves ----
        __threadfence();
        __builtin_amdgcn_wave_barrier();
        row_intra += intra;
        if (lane == 0) __hip_atomic_store(prog + mby, (mbx + 1) | (row_intra << 16), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
        PROF(5);
    }
    if (a.prof && lane < 8) {
        long long v = lane == 0 ? pacc[0] : lane == 1 ? pacc[1] : lane == 2 ? pacc[2] : lane == 3 ? pacc[3] : lane == 4 ? pacc[4] : lane == 5 ? pacc[5] : lane == 6 ? pacc[6] : pacc[7];
        a.prof[((size_t)bz * a.mb_h + mby) * 8 + lane] = v;
    }
  }   // rows
    if constexpr (RD) {     // x264_slice_write's end (R/encoder/encoder.c:1269-1273)
        if (rd.write && lane == 0) { cd_encode_flush(cab, rd.i_frame + bz * rd.i_frame_stride); rd.payload_len[bz] = (int)(cab.p - payload0); }
        if constexpr (SUB8) {       // the cache's own entries as the frame's last macroblock leaves them: the chain's next frame starts from them
            if (rd.mb_carry) {
                u8 *cp = rd.mb_carry + (size_t)bz * 160;
                if (lane < 32) cp[lane] = lane < 27 ? s.nnz[lane] : (u8)0;
                if (lane < 16) {
                    const int k = 12 + (lane & 3) + 8 * (lane >> 2);
                    ((i16 *)(cp + 32))[2 * lane] = sr.cmvd[k][0]; ((i16 *)(cp + 32))[2 * lane + 1] = sr.cmvd[k][1];
                }
            }
        }
        if constexpr (TD) if (rd.direct_score && lane == 0) { rd.direct_score[2 * bz] = dscore0; rd.direct_score[2 * bz + 1] = dscore1; }
        if constexpr (TD) {
            if (rd.stale && lane == 30) { i16 *sp = rd.stale + (size_t)bz * 8; for (int k = 0; k < 6; k++) sp[k] = sb.stale[k]; }
        } else if (!BS && rd.stale && is_p && lane == 0) {            // (an I slice never touches the motion cache)
            i16 *sp = rd.stale + (size_t)bz * 8;
            sp[0] = (i16)st0r; sp[1] = (i16)st0x; sp[2] = (i16)st0y;
        }
    }
    if (a.nr) {
        if (lane >= 1 && lane < 16 && nr_acc4) atomicAdd(a.nr_sum + (size_t)bz * 128 + lane, (u32)nr_acc4);
        if (lane >= 1 && nr_acc8) atomicAdd(a.nr_sum + (size_t)bz * 128 + 64 + lane, (u32)nr_acc8);
        if (lane == 0 && (nr_n4 | nr_n8)) { atomicAdd(a.nr_count + (size_t)bz * 2, (u32)nr_n4); atomicAdd(a.nr_count + (size_t)bz * 2 + 1, (u32)nr_n8); }
    }
#undef PROF
#undef LAUNDER
