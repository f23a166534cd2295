// stream_stats.hip -- h->stat: x264_encoder_frame_end's sums (R/encoder/encoder.c:1760-1835) and x264_encoder_close's report (:1899-2080) in host C, in the
// reference's types and with its format strings; every line as x264_log's default handler prints it (R/common/common.c:600-623).  No device call: the
// per-frame numbers come in as an x264hip_frame_report (csrc/frame_quality.hip).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "internal.h"
#include "mb_vocab.h"
#include "../../include/x264hip_stream.h"

using x264hip::set_error;

enum { ST_P = 0, ST_B = 1, ST_I = 2 };                 // SLICE_TYPE_P / _B / _I (R/common/common.h:128-134)
#define NALU_OVERHEAD 5                                // encoder.c:43: startcode + NAL type costs 5 bytes per frame
#define X264_BFRAME_MAX 16

struct x264hip_stat {
    int width, height, fps_num, fps_den, bframe, transform_8x8, direct_auto, i_mb_count;
    int b_psnr, b_ssim, i_frame;
    int     i_slice_count[3];
    int64_t i_slice_size[3];
    double  f_slice_qp[3];
    int     i_consecutive_bframes[X264_BFRAME_MAX + 1];
    int64_t i_ssd_global[3];
    double  f_psnr_average[3], f_psnr_mean_y[3], f_psnr_mean_u[3], f_psnr_mean_v[3], f_ssim_mean_y[3];
    int64_t i_mb_count_type[3][19];
    int64_t i_mb_partition[2][17];
    int64_t i_mb_count_8x8dct[2];
    int64_t i_mb_count_ref[2][2][32];
    int     i_direct_frames[2];
};

// encoder.c:57-64
static float x264_psnr(int64_t i_sqe, int64_t i_size)
{
    double f_mse = (double)i_sqe / ((double)65025.0 * (double)i_size);
    if (f_mse <= 0.0000000001) return 100;             /* Max 100dB */
    return (float)(-10.0 * log(f_mse) / log(10.0));
}

extern "C" x264hip_stat *x264hip_stat_new(const x264hip_encoder_params *p, int psnr, int ssim)
{
    if (!p || !p->d_valid) { set_error("stat_new: parameters not validated"); return nullptr; }
    x264hip_stat *s = (x264hip_stat *)calloc(1, sizeof(*s));
    if (!s) { set_error("stat_new: out of memory"); return nullptr; }
    s->width = p->width; s->height = p->height; s->fps_num = p->fps_num; s->fps_den = p->fps_den;
    s->bframe = p->bframe < X264_BFRAME_MAX ? p->bframe : X264_BFRAME_MAX;
    s->transform_8x8 = p->transform_8x8;
    s->direct_auto = p->direct_mv_pred == 3;           // X264_DIRECT_PRED_AUTO
    s->i_mb_count = p->d_mb_width * p->d_mb_height;
    s->b_psnr = psnr && !p->d_lossless; s->b_ssim = ssim && !p->d_lossless;        // encoder.c:410-411
    return s;
}
extern "C" void x264hip_stat_delete(x264hip_stat *s) { free(s); }
extern "C" int x264hip_stat_frames(const x264hip_stat *s) { return s ? s->i_frame : -1; }

extern "C" int x264hip_stat_frame_end(x264hip_stat *s, const x264hip_stat_frame *f, const x264hip_frame_report *r, char *line, int cap)
{
    if (!s || !f || !r || f->slice_type < 0 || f->slice_type > 2) { set_error("stat_frame_end: bad argument"); return -1; }
    const int t = f->slice_type;
    const int *mbs = r->mb_count;
    // x264_ratecontrol_end (ratecontrol.c:1085-1092): rc->qpa_aq is a float sum of integer QPs (exact), divided by the int macroblock count
    const int i_mb_count_skip = mbs[T_P_SKIP] + mbs[T_B_SKIP], i_mb_count_i = mbs[T_I_16x16] + mbs[T_I_8x8] + mbs[T_I_4x4];
    int i_mb_count_p = mbs[T_P_L0] + mbs[T_P_8x8];
    for (int i = T_B_DIRECT; i < T_B_8x8; i++) i_mb_count_p += mbs[i];
    float f_qp_avg_aq = (float)r->qp_sum;
    f_qp_avg_aq /= s->i_mb_count;

    s->i_slice_count[t]++;
    s->i_slice_size[t] += f->frame_size + NALU_OVERHEAD;
    s->f_slice_qp[t] += f_qp_avg_aq;
    for (int i = 0; i < 19; i++) s->i_mb_count_type[t][i] += r->mb_count[i];
    if (t != ST_I)                                     // (the reference adds an I slice's partition counts, all zero, behind the array's end)
        for (int i = 0; i < 17; i++) s->i_mb_partition[t][i] += r->mb_partition[i];
    for (int i = 0; i < 2; i++) s->i_mb_count_8x8dct[i] += r->mb_count_8x8dct[i];
    if (t != ST_I)
        for (int l = 0; l < 2; l++)
            for (int i = 0; i < 32; i++) s->i_mb_count_ref[t][l][i] += r->mb_count_ref[l][i];
    if (t == ST_P) {
        if (f->frames_since_ref < 0 || f->frames_since_ref > X264_BFRAME_MAX) { set_error("stat_frame_end: %d B frames before a P frame", f->frames_since_ref); return -1; }
        s->i_consecutive_bframes[f->frames_since_ref]++;
    }
    if (t == ST_B) s->i_direct_frames[!!f->direct_spatial]++;

    char msg[80];
    msg[0] = '\0';
    if (s->b_psnr) {
        const int64_t ssd[3] = {r->ssd[0], r->ssd[1], r->ssd[2]};
        s->i_ssd_global[t] += ssd[0] + ssd[1] + ssd[2];
        s->f_psnr_average[t] += x264_psnr(ssd[0] + ssd[1] + ssd[2], 3 * s->width * s->height / 2);
        s->f_psnr_mean_y[t] += x264_psnr(ssd[0], s->width * s->height);
        s->f_psnr_mean_u[t] += x264_psnr(ssd[1], s->width * s->height / 4);
        s->f_psnr_mean_v[t] += x264_psnr(ssd[2], s->width * s->height / 4);
        snprintf(msg, 80, " PSNR Y:%5.2f U:%5.2f V:%5.2f", x264_psnr(ssd[0], s->width * s->height), x264_psnr(ssd[1], s->width * s->height / 4),
                 x264_psnr(ssd[2], s->width * s->height / 4));
    }
    if (s->b_ssim) {
        double ssim_y = r->ssim / (((s->width - 6) >> 2) * ((s->height - 6) >> 2));
        s->f_ssim_mean_y[t] += ssim_y;
        snprintf(msg + strlen(msg), 80 - strlen(msg), " SSIM Y:%.5f", ssim_y);
    }
    msg[79] = '\0';
    int n = 0;
    if (line && cap > 0) {
        n = snprintf(line, (size_t)cap, "x264 [debug]: frame=%4d QP=%.2f NAL=%d Slice:%c Poc:%-3d I:%-4d P:%-4d SKIP:%-4d size=%d bytes%s\n", s->i_frame,
                     f_qp_avg_aq, f->nal_ref_idc, t == ST_I ? 'I' : (t == ST_P ? 'P' : 'B'), f->poc, i_mb_count_i, i_mb_count_p, i_mb_count_skip,
                     f->frame_size, msg);
        if (n >= cap) { set_error("stat_frame_end: the line needs %d bytes", n + 1); n = -1; }
    }
    s->i_frame++;                                      // (h->i_frame: x264_reference_update counts a frame when the next one begins, encoder.c:1062-1064)
    return n;
}

// x264_print_intra, encoder.c:1864-1873
static void print_intra(const int64_t *i_mb_count, double i_count, int b_print_pcm, char *intra)
{
    intra += sprintf(intra, "I16..4%s: %4.1f%% %4.1f%% %4.1f%%", b_print_pcm ? "..PCM" : "", i_mb_count[T_I_16x16] / i_count, i_mb_count[T_I_8x8] / i_count,
                     i_mb_count[T_I_4x4] / i_count);
    if (b_print_pcm) sprintf(intra, " %4.1f%%", i_mb_count[T_I_PCM] / i_count);
}

namespace {
struct Out {                                           // x264_log( h, X264_LOG_INFO, ... ) into the caller's buffer
    char *dst; int cap, n; bool over;
    void info(const char *fmt, ...) __attribute__((format(printf, 2, 3)))
    {
        char buf[1200];
        va_list ap;
        va_start(ap, fmt);
        int m = snprintf(buf, sizeof buf, "x264 [info]: ");
        m += vsnprintf(buf + m, sizeof buf - (size_t)m, fmt, ap);
        va_end(ap);
        if (m >= (int)sizeof buf || n + m >= cap) { over = true; return; }
        memcpy(dst + n, buf, (size_t)m + 1);
        n += m;
    }
};
}

extern "C" int x264hip_stat_summary(const x264hip_stat *s, char *dst, int cap)
{
    if (!s || !dst || cap <= 0) { set_error("stat_summary: bad argument"); return -1; }
    static const uint8_t partition_pixel[17] = {6, 4, 5, 3, 6, 4, 5, 3, 6, 4, 5, 3, 3, 3, 1, 2, 0};      // x264_mb_partition_pixel_table
    enum { PIXEL_16x16 = 0, PIXEL_16x8, PIXEL_8x16, PIXEL_8x8, PIXEL_8x4, PIXEL_4x8, PIXEL_4x4 };
    Out o = {dst, cap, 0, false};
    dst[0] = '\0';
    const int64_t i_yuv_size = 3 * s->width * s->height / 2;
    int64_t i_mb_count_size[2][7] = {{0}};
    char buf[1000];
    const int b_print_pcm = s->i_mb_count_type[ST_I][T_I_PCM] || s->i_mb_count_type[ST_P][T_I_PCM] || s->i_mb_count_type[ST_B][T_I_PCM];

    /* Slices used and PSNR */
    static const int slice_order[3] = {ST_I, ST_P, ST_B};
    static const char *slice_name[3] = {"P", "B", "I"};
    for (int i = 0; i < 3; i++) {
        const int i_slice = slice_order[i];
        if (s->i_slice_count[i_slice] > 0) {
            const int i_count = s->i_slice_count[i_slice];
            if (s->b_psnr)
                o.info("slice %s:%-5d Avg QP:%5.2f  size:%6.0f  PSNR Mean Y:%5.2f U:%5.2f V:%5.2f Avg:%5.2f Global:%5.2f\n", slice_name[i_slice], i_count,
                       s->f_slice_qp[i_slice] / i_count, (double)s->i_slice_size[i_slice] / i_count, s->f_psnr_mean_y[i_slice] / i_count,
                       s->f_psnr_mean_u[i_slice] / i_count, s->f_psnr_mean_v[i_slice] / i_count, s->f_psnr_average[i_slice] / i_count,
                       x264_psnr(s->i_ssd_global[i_slice], i_count * i_yuv_size));
            else
                o.info("slice %s:%-5d Avg QP:%5.2f  size:%6.0f\n", slice_name[i_slice], i_count, s->f_slice_qp[i_slice] / i_count,
                       (double)s->i_slice_size[i_slice] / i_count);
        }
    }
    if (s->bframe && s->i_slice_count[ST_P]) {
        char *p = buf;
        int den = 0;
        // weight by number of frames (including the P-frame) that are in a sequence of N B-frames
        for (int i = 0; i <= s->bframe; i++) den += (i + 1) * s->i_consecutive_bframes[i];
        for (int i = 0; i <= s->bframe; i++) p += sprintf(p, " %4.1f%%", 100. * (i + 1) * s->i_consecutive_bframes[i] / den);
        o.info("consecutive B-frames:%s\n", buf);
    }
    for (int i_type = 0; i_type < 2; i_type++)
        for (int i = 0; i < 17; i++) {
            if (i == D_DIRECT_8x8) continue;           /* direct is counted as its own type */
            i_mb_count_size[i_type][partition_pixel[i]] += s->i_mb_partition[i_type][i];
        }

    /* MB types used */
    if (s->i_slice_count[ST_I] > 0) {
        double i_count = s->i_slice_count[ST_I] * s->i_mb_count / 100.0;
        print_intra(s->i_mb_count_type[ST_I], i_count, b_print_pcm, buf);
        o.info("mb I  %s\n", buf);
    }
    if (s->i_slice_count[ST_P] > 0) {
        const int64_t *i_mb_count = s->i_mb_count_type[ST_P];
        double i_count = s->i_slice_count[ST_P] * s->i_mb_count / 100.0;
        const int64_t *i_mb_size = i_mb_count_size[ST_P];
        print_intra(i_mb_count, i_count, b_print_pcm, buf);
        o.info("mb P  %s  P16..4: %4.1f%% %4.1f%% %4.1f%% %4.1f%% %4.1f%%    skip:%4.1f%%\n", buf, i_mb_size[PIXEL_16x16] / (i_count * 4),
               (i_mb_size[PIXEL_16x8] + i_mb_size[PIXEL_8x16]) / (i_count * 4), i_mb_size[PIXEL_8x8] / (i_count * 4),
               (i_mb_size[PIXEL_8x4] + i_mb_size[PIXEL_4x8]) / (i_count * 4), i_mb_size[PIXEL_4x4] / (i_count * 4), i_mb_count[T_P_SKIP] / i_count);
    }
    if (s->i_slice_count[ST_B] > 0) {
        int64_t i_mb_count[19];
        memcpy(i_mb_count, s->i_mb_count_type[ST_B], sizeof i_mb_count);
        double i_count = s->i_slice_count[ST_B] * s->i_mb_count / 100.0;
        double i_mb_list_count;
        const int64_t *i_mb_size = i_mb_count_size[ST_B];
        int64_t list_count[3] = {0};                   /* 0 == L0, 1 == L1, 2 == BI */
        print_intra(i_mb_count, i_count, b_print_pcm, buf);
        for (int i = 0; i < 17; i++)                   // (X264_PARTTYPE_MAX of them, as the reference walks x264_mb_type_list_table)
            for (int j = 0; j < 2; j++) {
                // x264_mb_type_list_table[i][list][j]: P_L0 and P_SKIP use list 0, B_L0_L0 .. B_BI_BI by B_USES, the rest none
                const int l0 = i == T_P_L0 || i == T_P_SKIP ? 1 : i >= T_B_L0_L0 && i <= T_B_BI_BI ? B_USES(i, 0, j) : 0;
                const int l1 = i >= T_B_L0_L0 && i <= T_B_BI_BI ? B_USES(i, 1, j) : 0;
                if (l0 || l1) list_count[l1 + l0 * l1] += s->i_mb_count_type[ST_B][i] * 2;
            }
        list_count[0] += s->i_mb_partition[ST_B][D_L0_8x8];
        list_count[1] += s->i_mb_partition[ST_B][D_L1_8x8];
        list_count[2] += s->i_mb_partition[ST_B][D_BI_8x8];
        i_mb_count[T_B_DIRECT] += (s->i_mb_partition[ST_B][D_DIRECT_8x8] + 2) / 4;
        i_mb_list_count = (list_count[0] + list_count[1] + list_count[2]) / 100.0;
        o.info("mb B  %s  B16..8: %4.1f%% %4.1f%% %4.1f%%  direct:%4.1f%%  skip:%4.1f%%  L0:%4.1f%% L1:%4.1f%% BI:%4.1f%%\n", buf,
               i_mb_size[PIXEL_16x16] / (i_count * 4), (i_mb_size[PIXEL_16x8] + i_mb_size[PIXEL_8x16]) / (i_count * 4), i_mb_size[PIXEL_8x8] / (i_count * 4),
               i_mb_count[T_B_DIRECT] / i_count, i_mb_count[T_B_SKIP] / i_count, list_count[0] / i_mb_list_count, list_count[1] / i_mb_list_count,
               list_count[2] / i_mb_list_count);
    }

    /* x264_ratecontrol_summary prints nothing for constant QP and CRF (ratecontrol.c:1027-1038) */

    if (s->i_slice_count[ST_I] + s->i_slice_count[ST_P] + s->i_slice_count[ST_B] > 0) {
        const int i_count = s->i_slice_count[ST_I] + s->i_slice_count[ST_P] + s->i_slice_count[ST_B];
        float fps = (float)s->fps_num / s->fps_den;
#define SUM3(p) (p[ST_I] + p[ST_P] + p[ST_B])
#define SUM3b(p, o_) (p[ST_I][o_] + p[ST_P][o_] + p[ST_B][o_])
        float f_bitrate = fps * SUM3(s->i_slice_size) / i_count / 125;
        if (s->transform_8x8) {
            int64_t i_i8x8 = SUM3b(s->i_mb_count_type, T_I_8x8);
            int64_t i_intra = i_i8x8 + SUM3b(s->i_mb_count_type, T_I_4x4) + SUM3b(s->i_mb_count_type, T_I_16x16);
            o.info("8x8 transform  intra:%.1f%%  inter:%.1f%%\n", 100. * i_i8x8 / i_intra, 100. * s->i_mb_count_8x8dct[1] / s->i_mb_count_8x8dct[0]);
        }
        if (s->direct_auto && s->i_slice_count[ST_B])
            o.info("direct mvs  spatial:%.1f%%  temporal:%.1f%%\n", s->i_direct_frames[1] * 100. / s->i_slice_count[ST_B],
                   s->i_direct_frames[0] * 100. / s->i_slice_count[ST_B]);
        for (int i_list = 0; i_list < 2; i_list++)
            for (int i_slice = 0; i_slice < 2; i_slice++) {
                char *p = buf;
                int64_t i_den = 0;
                int i_max = 0;
                for (int i = 0; i < 32; i++)
                    if (s->i_mb_count_ref[i_slice][i_list][i]) { i_den += s->i_mb_count_ref[i_slice][i_list][i]; i_max = i; }
                if (i_max == 0) continue;
                for (int i = 0; i <= i_max; i++) p += sprintf(p, " %4.1f%%", 100. * s->i_mb_count_ref[i_slice][i_list][i] / i_den);
                o.info("ref %c L%d %s\n", "PB"[i_slice], i_list, buf);
            }
        if (s->b_ssim) o.info("SSIM Mean Y:%.7f\n", SUM3(s->f_ssim_mean_y) / i_count);
        if (s->b_psnr)
            o.info("PSNR Mean Y:%6.3f U:%6.3f V:%6.3f Avg:%6.3f Global:%6.3f kb/s:%.2f\n", SUM3(s->f_psnr_mean_y) / i_count, SUM3(s->f_psnr_mean_u) / i_count,
                   SUM3(s->f_psnr_mean_v) / i_count, SUM3(s->f_psnr_average) / i_count, x264_psnr(SUM3(s->i_ssd_global), i_count * i_yuv_size), f_bitrate);
        else
            o.info("kb/s:%.1f\n", f_bitrate);
#undef SUM3
#undef SUM3b
    }
    if (o.over) { set_error("stat_summary: the report does not fit %d bytes", cap); return -1; }
    return o.n;
}
