/* x264hip_stream.h -- the bytes around slice_data(): what x264_encoder_encode puts in front of and around the payloads the sweep returns,
 * so that a host that is NOT the reference's encoder.c (x264_vs2008_amd/mux.py, a C consumer) can emit the complete Annex B stream.
 * Host C of the library, no device call inside.  A maintainer of the reference keeps encoder.c's own writers and needs none of this.
 *
 *   x264hip_validate_parameters   x264_validate_parameters (R/encoder/encoder.c:335-606), the part that reaches the stream: clamps, the level
 *                                 picked from frame size / DPB / macroblock rate (x264_validate_levels, R/encoder/set.c:538-577), mv_range,
 *                                 the psy-RD shift of the chroma QP offset; then x264_sps_init / x264_pps_init's derived values (set.c:77-212,367-431)
 *   x264hip_param2string          x264_param2string( p, 0 ) (R/common/common.c:816-909)
 *   x264hip_sps_write / _pps_write / _sei_version_write      x264_sps_write, x264_pps_write, x264_sei_version_write (set.c:215-365,433-506), as RBSP bytes
 *   x264hip_stat_* / x264hip_frame_report_*      h->stat: x264_fdec_filter_row's PSNR / SSIM measurement and x264_slice_write's counters per frame (device),
 *                                 x264_encoder_frame_end's sums and x264_encoder_close's report (host C) -- at the end of this file
 *   x264hip_slice_nal             x264_slice_header_write (encoder.c:168-299) + bs_align_1 and the CABAC bytes, or the CAVLC bits spliced on
 *                                 behind the header's last bit + bs_rbsp_trailing (encoder.c:1151-1282), through x264_nal_encode
 *
 * Pinning: x264hip_param2string against the reference's own x264_param2string (oracle/_ref); the writers cannot be compared live (R/encoder/set.c and
 * encoder.c need the configure-generated config.h: not buildable here) and are pinned end to end by the md5 of the reference CLI's whole .264 that
 * SURVEY.md 8(c) records for BASELINE's configurations (tests/test_gpu_mux.py).
 */
#ifndef X264HIP_STREAM_H
#define X264HIP_STREAM_H
#include <stdint.h>
#include "x264hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* x264_param_t's fields that reach the stream (names follow R/x264.h:152-295).  Fill like x264_param_default + the command line, then call
 * x264hip_validate_parameters once: it edits the fields as x264_encoder_open does and fills the derived ones (d_*). */
typedef struct x264hip_encoder_params {
    int width, height, fps_num, fps_den;
    int level_idc;                         /* -1: chosen like x264_validate_parameters does */
    int threads;                           /* 1 (printed in the SEI) */
    int frame_reference, keyint_max, keyint_min, scenecut_threshold, pre_scenecut;
    int bframe, bframe_adaptive, bframe_bias, bframe_pyramid;
    int deblocking_filter, deblocking_filter_alphac0, deblocking_filter_beta;
    int cabac, cabac_init_idc, interlaced, cqm_preset;
    unsigned intra, inter;                 /* param.analyse.intra / .inter */
    int transform_8x8, weighted_bipred, direct_mv_pred, chroma_qp_offset;
    int me_method, me_range, mv_range, subpel_refine, chroma_me, mixed_references, trellis, fast_pskip, dct_decimate, noise_reduction;
    float psy_rd, psy_trellis;
    int luma_deadzone[2];
    int rc_method;                         /* X264_RC_CQP 0, X264_RC_CRF 1 (ABR / VBV / 2-pass: not built) */
    int qp_constant, qp_min, qp_max, qp_step;
    float rf_constant, ip_factor, pb_factor, qcompress;
    int aq_mode;
    float aq_strength;
    const uint8_t *scaling_list[6];        /* cqm_preset != 0: the PPS's lists (4iy 4ic 4py 4pc 8iy 8py), zigzag order is applied here */
    /* derived by x264hip_validate_parameters */
    int d_valid, d_lossless, d_profile_idc, d_num_ref_frames, d_num_reorder_frames, d_log2_max_frame_num, d_log2_max_poc_lsb,
        d_mb_width, d_mb_height, d_pic_init_qp, d_log2_max_mv_length, d_psy_rd_fix8;
} x264hip_encoder_params;

void x264hip_encoder_params_default(x264hip_encoder_params *p);            /* x264_param_default's values for the fields above */
int x264hip_validate_parameters(x264hip_encoder_params *p);                /* 0, or -1 + x264hip_last_error() */
int x264hip_param2string(const x264hip_encoder_params *p, char *dst, int cap);      /* length, or -1 */
/* RBSP bytes (no NAL header, no emulation prevention: x264hip_nal_encode adds both); return the length or -1 */
int x264hip_sps_write(const x264hip_encoder_params *p, uint8_t *dst, int cap);
int x264hip_pps_write(const x264hip_encoder_params *p, uint8_t *dst, int cap);
int x264hip_sei_version_write(const x264hip_encoder_params *p, uint8_t *dst, int cap);

typedef struct x264hip_slice_header {
    int nal_type;              /* NAL_SLICE 1, NAL_SLICE_IDR 5 */
    int nal_ref_idc;           /* 3 IDR, 2 I / P, 0 disposable B */
    int slice_type;            /* 0 P, 1 B, 2 I (x264hip_slice_params.slice_type) */
    int frame_num, idr_pic_id /* -1 unless IDR */, poc, qp;
    int n_ref0, n_ref1;        /* h->i_ref0 / i_ref1 */
    int direct_spatial;        /* B: sh.b_direct_spatial_mv_pred */
    int ref_frame_num[16];     /* P: frame_num of list 0's pictures, for x264_reference_build_list's reorder check (encoder.c:961-972) */
} x264hip_slice_header;

/* One slice NAL, Annex B start code included: header + payload (CABAC: the bytes of x264hip_slice_rd.payload; CAVLC: the bits
 * x264hip_cavlc_write_frame wrote, trailing bits included -- they are re-aligned behind the header).  dst: payload_len * 3 / 2 + 64 bytes.
 * Returns the NAL's length or -1. */
int x264hip_slice_nal(const x264hip_encoder_params *p, const x264hip_slice_header *sh, const uint8_t *payload, int payload_len,
                      uint8_t *dst, int cap);

/* h->stat.frame's terms the post-encode scene cut of x264_encoder_encode reads after a P slice (R/encoder/encoder.c:1603-1644), per chain, from
 * the state the sweep left: out_dev [batch] records on the device (stream-ordered).  x264hip_scenecut_post is the decision (host C, the reference's
 * float expression): 1 = the reference gives this attempt up and codes again -- the picture as I / IDR, or the B picture before it as the P: the host
 * discards the attempt (reconstruction, payload, its place in the DPB), calls x264hip_lookahead_scenecut (x264hip.h) instead of x264hip_lookahead_end and
 * codes what x264hip_lookahead_get hands out next (x264_vs2008_amd/stream.py: StreamEncoder.step does it inside the step, for the chains concerned). */
typedef struct x264hip_frame_stat { int64_t intra_cost, inter_cost; int32_t mbs_analysed, mb_i, mb_p, mb_skip; } x264hip_frame_stat;
int x264hip_frame_stats(x264hip_frame_ctx *c, const x264hip_mb_state *st, x264hip_frame_stat *out_dev);
int x264hip_scenecut_post(const x264hip_frame_stat *s, int i_mb, int i_gop_size, int scenecut_threshold, int keyint_min, int keyint_max);

/* x264hip_slice_nal, which also returns in *rbsp_size the NAL's payload size before x264_nal_encode (slice header + slice data + trailing bits, no
 * NAL header, no emulation prevention): nal->i_payload, the i_frame_size x264_encoder_encode reports and its statistics add up (encoder.c:1335,1762). */
int x264hip_slice_nal_sized(const x264hip_encoder_params *p, const x264hip_slice_header *sh, const uint8_t *payload, int payload_len,
                            uint8_t *dst, int cap, int *rbsp_size);

/* ---- what x264 core 66 measures of every coded frame, and the report x264_encoder_close prints --------------------------------------------------
 * Device half: one pass per step over the finished pictures and the states the sweeps left.  x264_fdec_filter_row measures while it filters
 * (encoder.c:1031-1056): PSNR's squared error of the three planes over the true width x height, and SSIM of the luma plane from column 2 -- per
 * macroblock row, each call's float added into the double h->stat.frame.f_ssim.  A row's later neighbours never touch rows already measured, so the
 * finished frame gives the same numbers: measure a kept frame after x264hip_deblock_frame, a disposable B frame on its unfiltered reconstruction
 * (b_deblock &= b_hpel, encoder.c:991), and before anything overwrites the source or the reconstruction.  ssd equals the reference's as integers and
 * ssim as a double, bit for bit: the float adds are nested as x264_pixel_ssim_wxh and x264_fdec_filter_row nest them (csrc/frame_quality.hip).
 * The counters are h->stat.frame's (x264_slice_write, encoder.c:1229-1251) from the state's mb_type / partition / sub_partition / ref / ref1 / cbp /
 * t8 / qp arrays; qp_sum / (mb_w * mb_h) in float is fdec->f_qp_avg_aq (ratecontrol.c:931,1092). */
typedef struct x264hip_frame_report {
    int64_t ssd[3];                    /* h->stat.frame.i_ssd */
    double  ssim;                      /* h->stat.frame.f_ssim: the sum, not yet divided by the number of 4x4 windows */
    int32_t qp_sum;
    int32_t mb_count[19];              /* by macroblock type (R/common/macroblock.h:61-86) */
    int32_t mb_partition[17];          /* by partition / sub-partition type (:112-138) */
    int32_t mb_count_8x8dct[2];
    int32_t mb_count_ref[2][32];
    int32_t reserved;
} x264hip_frame_report;
/* One chain's frame in a launch of x264hip_frame_report_chains, in the style of x264hip_chain_sweep: the pictures and the state are the batch-wide ones,
 * the entry reads element fenc_element of the source picture, element recon_element of the reconstruction and element `chain` of the state's arrays
 * (state NULL: no counters, they are left zero).  count_refs: param.i_frame_reference > 1. */
typedef struct x264hip_chain_report {
    int chain;
    const x264hip_picture *fenc;
    int fenc_element;
    const x264hip_picture *recon;
    int recon_element;
    const x264hip_mb_state *state;
    int slice_type;                    /* 0 P, 1 B (list 1's references are counted too), 2 I */
    int psnr, ssim, count_refs;
} x264hip_chain_report;
/* out_dev: n records in entry order (device, stream-ordered).  staging_host (pinned) and table_dev: n * x264hip_chain_report_bytes() each; scratch_dev:
 * n * x264hip_frame_report_scratch_bytes(c) (the calls' partial results); all left alone until the stream has passed the call.  Two launches on the
 * context's stream however many entries and pictures, no synchronisation, no allocation.  Refused: a width whose two rows of block sums exceed 64 KB of LDS. */
int x264hip_frame_report_chains(x264hip_frame_ctx *c, const x264hip_chain_report *entries, int n, void *staging_host, void *table_dev, void *scratch_dev,
                                x264hip_frame_report *out_dev);
size_t x264hip_chain_report_bytes(void);
size_t x264hip_frame_report_scratch_bytes(const x264hip_frame_ctx *c);
/* Lock step: every element of the batch from one source picture, one reconstruction and one state; out_dev [batch] records in element order.
 * flags: X264HIP_REPORT_*.  staging_host: batch * x264hip_frame_report_frame_staging_bytes(); table_dev and scratch_dev as above with n = batch. */
#define X264HIP_REPORT_PSNR 1
#define X264HIP_REPORT_SSIM 2
#define X264HIP_REPORT_REFS 4          /* param.i_frame_reference > 1 */
int x264hip_frame_report_frame(x264hip_frame_ctx *c, const x264hip_picture *fenc, const x264hip_picture *recon, const x264hip_mb_state *state,
                               int slice_type, int flags, void *staging_host, void *table_dev, void *scratch_dev, x264hip_frame_report *out_dev);
size_t x264hip_frame_report_frame_staging_bytes(void);

/* Host half (no device call inside): h->stat of x264_encoder_frame_end (encoder.c:1760-1835) in the reference's types -- double sums, int64_t counts,
 * the float x264_psnr -- and x264_encoder_close's report (encoder.c:1899-2080).  psnr / ssim: param.analyse.b_psnr / b_ssim; both are forced off when
 * the parameters are lossless, as x264_validate_parameters does (encoder.c:410-411).  p: validated parameters (x264hip_validate_parameters). */
typedef struct x264hip_stat x264hip_stat;
typedef struct x264hip_stat_frame {
    int slice_type;                    /* 0 P, 1 B, 2 I */
    int frame_size;                    /* h->out.i_frame_size: x264hip_slice_nal_sized's rbsp_size */
    int nal_ref_idc, poc;              /* printed in the per-frame line */
    int frames_since_ref;              /* P: fdec->i_frame - fref0[0]->i_frame - 1, the B frames before this P in display order */
    int direct_spatial;                /* B: sh.b_direct_spatial_mv_pred */
} x264hip_stat_frame;
x264hip_stat *x264hip_stat_new(const x264hip_encoder_params *p, int psnr, int ssim);
void x264hip_stat_delete(x264hip_stat *s);
/* One coded frame (not a given-up attempt of the post-encode scene cut: x264_encoder_frame_end never sees those).  Writes the X264_LOG_DEBUG line
 * "x264 [debug]: frame=%4d QP=%.2f NAL=%d Slice:%c Poc:%-3d I:%-4d P:%-4d SKIP:%-4d size=%d bytes PSNR Y:... SSIM Y:...\n" into line (may be NULL);
 * returns its length, or -1. */
int x264hip_stat_frame_end(x264hip_stat *s, const x264hip_stat_frame *f, const x264hip_frame_report *r, char *line, int cap);
/* x264_encoder_close's lines in order, each as x264_log's default handler prints it ("x264 [info]: ...\n"); returns the length, or -1 if cap is too small. */
int x264hip_stat_summary(const x264hip_stat *s, char *dst, int cap);
int x264hip_stat_frames(const x264hip_stat *s);        /* frames accumulated so far */

#ifdef __cplusplus
}
#endif
#endif
