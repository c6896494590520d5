// engine_resize.hip — car_resize: Pillow's 8-bit Image.resize (modes L and RGB; sample_t2i_MR.py:37-49, dataset/augmentation.py:8-26, sample_t2i.py:135,
// demo/model.py:127,221, condition/utils.py:28-38) as one or two resample.hip launches, and car_debug_resample_coeffs, the host-only view of the tables.
// (one of the translation units behind include/controlar_hip.h; shared declarations: engine_internal.h)
#include "engine_internal.h"
#include "resample_tab.h"

extern "C" void car_launch_resample_h_lds(const ResampleP* p, int rb, int row_stride, hipStream_t st);

static const int kMaxSide = 1 << 16;             // per side, input and output
static const long long kMaxTable = 1LL << 24;    // taps of one axis table (out_size * ksize)

// why an axis cannot be resampled, or nullptr.  in0 / in1 are the box edges along it.
static const char* axis_refusal(int in_size, double in0, double in1, int out_size, int filter) {
    if (in_size <= 0 || out_size <= 0) return "sizes must be positive";
    if (in_size > kMaxSide || out_size > kMaxSide) return "a side is larger than 65536";
    if (!(in0 < in1)) return "the box is empty";
    if (!(in0 >= 0 && in1 <= (double)in_size)) return "the box lies outside the image";
    if (filter == RS_NEAREST) return "the NEAREST filter (0) is not implemented: Pillow takes another code path for it";
    if (!rs_filter_ok(filter)) return "unknown filter (1 LANCZOS, 2 BILINEAR, 3 BICUBIC, 4 BOX, 5 HAMMING)";
    if (rs_ksize(in0, in1, out_size, filter) * out_size > kMaxTable) return "the coefficient table would exceed 2^24 taps";
    return nullptr;
}

extern "C" int car_debug_resample_coeffs(int32_t in_size, double in0, double in1, int32_t out_size, int32_t filter,
                                         int32_t* ksize_out, int32_t* kk, int32_t* bounds, int64_t max_kk) {
    if (!ksize_out || !kk || !bounds || axis_refusal(in_size, in0, in1, out_size, filter)) return -1;
    if (rs_ksize(in0, in1, out_size, filter) * out_size > max_kk) return -1;
    std::vector<int32_t> k, b;
    *ksize_out = rs_coeffs(in_size, in0, in1, out_size, filter, k, b);
    memcpy(kk, k.data(), k.size() * sizeof(int32_t));
    memcpy(bounds, b.data(), b.size() * sizeof(int32_t));
    return 0;
}

// The table of one axis, rebuilt and uploaded on `st` only when its key changed.
static int get_axis(car_ctx* c, ResampleAxis& a, int in_size, double in0, double in1, int out_size, int filter, hipStream_t st) {
    if (a.filter == filter && a.in_size == in_size && a.out_size == out_size && a.in0 == in0 && a.in1 == in1) return 0;
    if (!c->ev_rs) HIPCHK(c, hipEventCreateWithFlags(&c->ev_rs, hipEventDisableTiming));
    else HIPCHK(c, hipEventSynchronize(c->ev_rs));          // the previous upload has read the host copies
    a.filter = -1;
    a.ksize = rs_coeffs(in_size, in0, in1, out_size, filter, a.kk, a.bounds);
    a.lo = in_size; a.hi = 0;
    for (int i = 0; i < out_size; ++i) {
        const int x0 = a.bounds[(size_t)2 * i], n = a.bounds[(size_t)2 * i + 1];
        if (n > 0) { a.lo = std::min(a.lo, x0); a.hi = std::max(a.hi, x0 + n); }
    }
    if (a.hi <= a.lo) { a.lo = 0; a.hi = 1; }               // no output index reads anything (cannot happen for a box inside the image)
    NEED(c, a.d_kk, a.kk.size() * 4); NEED(c, a.d_bounds, a.bounds.size() * 4);
    HIPCHK(c, hipMemcpyAsync(a.d_kk.p, a.kk.data(), a.kk.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(a.d_bounds.p, a.bounds.data(), a.bounds.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(c->ev_rs, st));
    a.in_size = in_size; a.out_size = out_size; a.in0 = in0; a.in1 = in1; a.filter = filter;
    return 0;
}

extern "C" int car_resize(car_ctx* c, const uint8_t* img_hwc, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, int32_t filter,
                          const float* box, uint8_t* out_hwc, void* control_out, float* float_out, int32_t norm, void* stream_) {
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!img_hwc) FAIL(c, "car_resize: the image pointer is NULL");
    if (B <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) FAIL(c, "car_resize: sizes must be positive (got B %d, %d x %d -> %d x %d)", B, H, W, Ho, Wo);
    if (!out_hwc && !control_out && !float_out) FAIL(c, "car_resize: no output requested (out_hwc, control_out and float_out are all NULL)");
    if (C == 4) FAIL(c, "car_resize: C = 4 is not supported (no RGBA mode): reduce the image to three channels first (HWC3), then pass C = 3");
    if (C != 1 && C != 3) FAIL(c, "car_resize: C must be 1 (L) or 3 (RGB), got %d", C);
    if (float_out && norm != 0 && norm != 1) FAIL(c, "car_resize: norm must be 0 (raw) or 1 ((x/255 - 0.5)/0.5), got %d", norm);
    const double x0 = box ? (double)box[0] : 0.0, y0 = box ? (double)box[1] : 0.0, x1 = box ? (double)box[2] : (double)W, y1 = box ? (double)box[3] : (double)H;
    const char* why = axis_refusal(W, x0, x1, Wo, filter);
    if (!why) why = axis_refusal(H, y0, y1, Ho, filter);
    if (why) FAIL(c, "car_resize: %s (image %d x %d, box (%g, %g, %g, %g), output %d x %d, filter %d)", why, H, W, x0, y0, x1, y1, Ho, Wo, filter);
    // Pillow's rule: an axis whose size stays and whose box spans it is not touched at all
    const bool need_h = Wo != W || x0 != 0.0 || x1 != (double)W, need_v = Ho != H || y0 != 0.0 || y1 != (double)H;
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    ResampleAxis &ah = c->rs_axis[0], &av = c->rs_axis[1];
    if (need_h && get_axis(c, ah, W, x0, x1, Wo, filter, st)) return -1;
    if (need_v && get_axis(c, av, H, y0, y1, Ho, filter, st)) return -1;
    // the horizontal pass only makes the source rows the vertical pass reads
    const int row_lo = need_v ? av.lo : 0, nrows = need_v ? av.hi - av.lo : H;
    const int tmp_pitch = (int)rup((size_t)Wo * C, 4);
    if (need_h && need_v) NEED(c, c->resize_ws, (size_t)B * nrows * tmp_pitch);
    fence_in(c, caller);
    ResampleP p; memset(&p, 0, sizeof(p));
    p.B = B; p.C = C; p.Wo = Wo; p.norm = norm;
    p.src = img_hwc; p.src_pitch = W * C; p.src_img = (long)H * W * C; p.src_y0 = 0;
    auto finish = [&](int pass) {          // the pass that writes the caller's tensors
        p.final = 1; p.rows = Ho; p.row_bytes = Wo * C; p.nq = (p.row_bytes + 3) / 4;
        p.out = out_hwc; p.control = control_out; p.fout = float_out;
        car_launch_resample(c->mode, pass, &p, st);
    };
    if (need_h) {
        p.kk = (const int*)ah.d_kk.p; p.bounds = (const int*)ah.d_bounds.p; p.ksize = ah.ksize;
        if (!need_v) finish(0);
        else {
            p.final = 0; p.src_y0 = row_lo; p.rows = nrows; p.row_bytes = Wo * C; p.nq = tmp_pitch / 4;
            p.tmp = (unsigned char*)c->resize_ws.p; p.tmp_pitch = tmp_pitch; p.tmp_img = (long)nrows * tmp_pitch;
            // The LDS-staged form takes the pass when the source span of every 64-pixel tile fits: rb rows of row_stride bytes plus the result tile within
            // 48 KiB.  Large downscale factors of wide images do not (a span beyond ~16 K pixels): they keep the byte-gather form.  Both give the same bits.
            const std::vector<int32_t>& hb = ah.bounds;
            int max_span = 0; bool ok = CAR_KNOB("CAR_RESIZE_NO_LDS") == nullptr;
            for (int X0 = 0; X0 < Wo && ok; X0 += 64) {
                const int xl = std::min(X0 + 63, Wo - 1), s0 = hb[(size_t)2 * X0], s1 = hb[(size_t)2 * xl] + hb[(size_t)2 * xl + 1];
                for (int x = X0; x <= xl; ++x)          // the kernel relies on monotone bounds and on at least one tap per pixel
                    if (hb[(size_t)2 * x] < s0 || hb[(size_t)2 * x] + hb[(size_t)2 * x + 1] > s1 || hb[(size_t)2 * x + 1] <= 0) ok = false;
                max_span = std::max(max_span, s1 - s0);
            }
            const size_t row_stride = rup((size_t)max_span * C + 6, 4), lds_budget = 48 << 10;
            const int rb = (int)std::min<size_t>(16, lds_budget / (row_stride + (size_t)64 * C));
            if (ok && rb >= 1) car_launch_resample_h_lds(&p, rb, (int)row_stride, st);
            else car_launch_resample(c->mode, 0, &p, st);
            p.src = p.tmp; p.src_pitch = tmp_pitch; p.src_img = p.tmp_img;
        }
    }
    if (need_v) {
        p.kk = (const int*)av.d_kk.p; p.bounds = (const int*)av.d_bounds.p; p.ksize = av.ksize;
        p.src_y0 = need_h ? row_lo : 0;
        p.src_aligned = (((uintptr_t)p.src | (uintptr_t)p.src_pitch | (uintptr_t)p.src_img) & 3) == 0;
        finish(1);
    }
    if (!need_h && !need_v) finish(2);
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}
