// engine_metrics.hip — car_ms_ssim, car_f1, car_rmse, car_pixels_to_u8: the scoring step of evaluations/{hed,lineart}_ssim.py, canny_f1score.py,
// depth_rmse.py and autoregressive/test/metric.py, and the save_image quantiser in front of it (autoregressive/test/test_t2i.py:233-234), as metrics.hip
// launches.  (one of the translation units behind include/controlar_hip.h; shared declarations: engine_internal.h)
#include "engine_internal.h"
#include "metrics_params.h"

extern "C" {
void car_launch_ms_ssim_scale(const MsScaleP* p, long planes, hipStream_t st);
void car_launch_ms_ssim_fold(const MsFoldP* p, int B, hipStream_t st);
void car_launch_f1(const void* pred, int dt_p, int rule_p, float val_p, const void* tgt, int dt_t, int rule_t, float val_t, int B, long HW,
                   long chunk, int chunks, unsigned long long* part, long long* counts, double* f1, hipStream_t st);
void car_launch_rmse(const float* pred, const void* label, int dt_l, int B, long HW, long chunk, int chunks, int use_max, float* pmax, double* psum,
                     double* out, hipStream_t st);
void car_launch_pixels_to_u8(const float* x, int B, long HW, unsigned char* out_hwc, float* fout, hipStream_t st);
}

static const int kMaxBatch = 65535;              // images ride on grid.y
static const int kMsMinSide = 16 * (MS_K - 1) + 16;   // 176: the smallest side with side / 16 > 10

static bool metric_dtype_ok(int dt) { return dt == CAR_DT_F32 || dt == CAR_DT_U8; }

// an image of HW elements in at most 1024 chunks of at least 8192 elements: a block reduces one chunk
static void chunking(long HW, long* chunk, int* chunks) {
    long ch = 8192;
    while ((HW + ch - 1) / ch > 1024) ch *= 2;
    *chunk = ch; *chunks = (int)((HW + ch - 1) / ch);
}

extern "C" int car_ms_ssim(car_ctx* c, const void* pred, int32_t pred_dtype, const void* target, int32_t target_dtype, int32_t B, int32_t C, int32_t H,
                           int32_t W, double pred_scale, double target_scale, double* out, double* scales_out, void* stream_) {
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!pred || !target || !out) FAIL(c, "car_ms_ssim: pred, target and out must not be NULL");
    if (!metric_dtype_ok(pred_dtype) || !metric_dtype_ok(target_dtype)) FAIL(c, "car_ms_ssim: inputs are fp32 (0) or uint8 (4), got dtypes %d and %d", pred_dtype, target_dtype);
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) FAIL(c, "car_ms_ssim: sizes must be positive (got B %d, C %d, %d x %d)", B, C, H, W);
    if (H < kMsMinSide || W < kMsMinSide)
        FAIL(c, "car_ms_ssim: five scales with an 11 x 11 window need both sides to be at least %d (side / 16 > 10), got %d x %d", kMsMinSide, H, W);
    const long planes = (long)B * C;
    int hs[MS_SCALES], ws[MS_SCALES], tx[MS_SCALES], ty[MS_SCALES];
    size_t part_elems = 0, pool_elems = 0;
    MsFoldP f; memset(&f, 0, sizeof(f));
    for (int s = 0; s < MS_SCALES; ++s) {
        hs[s] = H >> s; ws[s] = W >> s;
        tx[s] = (ws[s] - (MS_K - 1) + MS_T - 1) / MS_T; ty[s] = (hs[s] - (MS_K - 1) + MS_T - 1) / MS_T;
        f.off[s] = (long)part_elems; f.ntile[s] = tx[s] * ty[s];
        f.count[s] = (double)C * (hs[s] - (MS_K - 1)) * (ws[s] - (MS_K - 1));
        part_elems += (size_t)planes * f.ntile[s] * 2;
        if (s) pool_elems += rup((size_t)planes * hs[s] * ws[s], 4) * 2;
    }
    if (B > kMaxBatch || (double)planes * f.ntile[0] > 2147483647.0)
        FAIL(c, "car_ms_ssim: the batch is too large for one call (B %d, C %d, %d x %d: at most %d images and 2^31 - 1 tiles)", B, C, H, W, kMaxBatch);
    NEED(c, c->metrics_ws, part_elems * sizeof(double) + pool_elems * sizeof(float));
    double* part = (double*)c->metrics_ws.p;
    float* pool = (float*)(part + part_elems);
    // the 1-D Gaussian, sigma 1.5, normalised to sum 1
    double g[MS_K], gs = 0;
    for (int i = 0; i < MS_K; ++i) { const double d = (i - (MS_K - 1) / 2) / 1.5; g[i] = exp(-d * d / 2); gs += g[i]; }
    for (int i = 0; i < MS_K; ++i) g[i] /= gs;
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    MsScaleP p; memset(&p, 0, sizeof(p));
    memcpy(p.g, g, sizeof(g));
    p.p = pred; p.t = target; p.dt_p = pred_dtype; p.dt_t = target_dtype; p.scale_p = pred_scale; p.scale_t = target_scale;
    for (int s = 0; s < MS_SCALES; ++s) {
        p.H = hs[s]; p.W = ws[s]; p.tiles_x = tx[s]; p.tiles_y = ty[s]; p.part = part + f.off[s];
        if (s + 1 < MS_SCALES) {
            p.Hn = hs[s + 1]; p.Wn = ws[s + 1];
            p.next_p = pool; p.next_t = pool + rup((size_t)planes * p.Hn * p.Wn, 4);
            pool = p.next_t + rup((size_t)planes * p.Hn * p.Wn, 4);
        } else { p.next_p = p.next_t = nullptr; p.Hn = p.Wn = 0; }
        car_launch_ms_ssim_scale(&p, planes, st);
        // the next scale reads the pooled images: already clipped, fp32
        p.p = p.next_p; p.t = p.next_t; p.dt_p = p.dt_t = CAR_DT_F32; p.scale_p = p.scale_t = 1.0;
    }
    static const double betas[MS_SCALES] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    memcpy(f.beta, betas, sizeof(betas));
    f.part = part; f.C = C; f.out = out; f.table = scales_out;
    car_launch_ms_ssim_fold(&f, B, st);
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int car_f1(car_ctx* c, const void* pred, int32_t pred_dtype, int32_t pred_rule, float pred_value, const void* target, int32_t target_dtype,
                      int32_t target_rule, float target_value, int32_t B, int32_t H, int32_t W, int64_t* counts_out, double* f1_out, void* stream_) {
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!pred || !target) FAIL(c, "car_f1: pred and target must not be NULL");
    if (!counts_out && !f1_out) FAIL(c, "car_f1: no output requested (counts_out and f1_out are both NULL)");
    if (!metric_dtype_ok(pred_dtype) || !metric_dtype_ok(target_dtype)) FAIL(c, "car_f1: inputs are fp32 (0) or uint8 (4), got dtypes %d and %d", pred_dtype, target_dtype);
    if ((pred_rule != MT_RULE_EQ && pred_rule != MT_RULE_GT) || (target_rule != MT_RULE_EQ && target_rule != MT_RULE_GT))
        FAIL(c, "car_f1: a rule is 0 (v == value) or 1 (v > value), got %d and %d", pred_rule, target_rule);
    if (B <= 0 || H <= 0 || W <= 0 || B > kMaxBatch) FAIL(c, "car_f1: sizes must be positive and B at most %d (got B %d, %d x %d)", kMaxBatch, B, H, W);
    const long HW = (long)H * W;
    long chunk; int chunks; chunking(HW, &chunk, &chunks);
    NEED(c, c->metrics_ws, (size_t)B * chunks * 3 * sizeof(unsigned long long));
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    car_launch_f1(pred, pred_dtype, pred_rule, pred_value, target, target_dtype, target_rule, target_value, B, HW, chunk, chunks,
                  (unsigned long long*)c->metrics_ws.p, (long long*)counts_out, f1_out, st);
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int car_rmse(car_ctx* c, const float* pred, const void* label, int32_t label_dtype, int32_t B, int32_t H, int32_t W, int32_t scale_to_max,
                        double* out, void* stream_) {
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!pred || !label || !out) FAIL(c, "car_rmse: pred, label and out must not be NULL");
    if (!metric_dtype_ok(label_dtype)) FAIL(c, "car_rmse: the label is fp32 (0) or uint8 (4), got dtype %d", label_dtype);
    if (scale_to_max != 0 && scale_to_max != 1) FAIL(c, "car_rmse: scale_to_max must be 0 (pred as it is) or 1 (pred * 255 / max(pred) per image), got %d", scale_to_max);
    if (B <= 0 || H <= 0 || W <= 0 || B > kMaxBatch) FAIL(c, "car_rmse: sizes must be positive and B at most %d (got B %d, %d x %d)", kMaxBatch, B, H, W);
    const long HW = (long)H * W;
    long chunk; int chunks; chunking(HW, &chunk, &chunks);
    const size_t n = (size_t)B * chunks;
    NEED(c, c->metrics_ws, n * sizeof(double) + n * sizeof(float));
    double* psum = (double*)c->metrics_ws.p;
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    car_launch_rmse(pred, label, label_dtype, B, HW, chunk, chunks, scale_to_max, (float*)(psum + n), psum, out, st);
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int car_pixels_to_u8(car_ctx* c, const float* x_nchw, int32_t B, int32_t H, int32_t W, uint8_t* out_hwc, float* float_out, void* stream_) {
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!x_nchw) FAIL(c, "car_pixels_to_u8: the image pointer is NULL");
    if (!out_hwc && !float_out) FAIL(c, "car_pixels_to_u8: no output requested (out_hwc and float_out are both NULL)");
    if (B <= 0 || H <= 0 || W <= 0 || B > kMaxBatch) FAIL(c, "car_pixels_to_u8: sizes must be positive and B at most %d (got B %d, %d x %d)", kMaxBatch, B, H, W);
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    car_launch_pixels_to_u8(x_nchw, B, (long)H * W, out_hwc, float_out, st);
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}
