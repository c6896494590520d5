// engine_lineart.hip — car_lineart: the LineArt control extractor (condition/lineart.py:26-86; callers sample_t2i.py:110-113,129-132,
// sample_t2i_MR.py, autoregressive/test/test_t2i.py:177) as a chain of lineart.hip launches, and the loader of its weight images ("lineart.*").
// (one of the translation units behind include/controlar_hip.h; shared declarations: engine_internal.h)
#include "engine_internal.h"

extern "C" {
int car_launch_la_to_nhwc(int mode, const float* img, void* out, int B, long HW, hipStream_t st);
int car_launch_la_conv(int mode, const LaConvP* p, int nimg, hipStream_t st);
int car_launch_la_fold(const float* part, const int* cnt, float* stats, int tiles_img, int N, int nimg, float eps, hipStream_t st);
int car_launch_la_norm(int mode, const float* raw, const float* stats, const void* skip, void* out, long n_img, long raw_img, long act_img,
                       int N, int relu, int nimg, hipStream_t st);
int car_launch_la_out7(int mode, const void* in, const void* w, const float* bias, float* out, void* control, int H, int W, long act_img, int nimg, hipStream_t st);
}

#define LACHK(ctx, x) do { const int _e = (x); if (_e != 0) FAIL(ctx, "car_lineart: %s failed: %s (%s:%d)", #x, hipGetErrorString((hipError_t)_e), __FILE__, __LINE__); } while (0)

// the 24 tensors of LineArt(n_residual_blocks = 3).state_dict(), under the "lineart." prefix of the C ABI
void lineart_tensor_names(const car_ctx*, std::vector<std::string>& v) {
    std::vector<std::string> mods = {"model0.1", "model1.0", "model1.3"};
    for (int r = 0; r < 3; ++r) for (const char* s : {".conv_block.1", ".conv_block.5"}) mods.push_back("model2." + std::to_string(r) + s);
    for (const char* s : {"model3.0", "model3.3", "model4.1"}) mods.push_back(s);
    for (auto& m : mods) { v.push_back("lineart." + m + ".weight"); v.push_back("lineart." + m + ".bias"); }
}

// Conv weights become implicit-GEMM images [Cout][taps*Cin] (k = tap*Cin + ci, K padded to the 32-wide k step) in the context's element type; a
// ConvTranspose2d weight [Cin,Cout,3,3] becomes its four output-parity phase images (weight_pack.h pack_convT_phases).  Biases stay fp32 (only model4's is
// applied: a bias in front of an InstanceNorm cancels).
int lineart_load_tensor(car_ctx* c, const LoadedTensor& t) {
    const std::string key = t.name.substr(8);
    const std::vector<int64_t>& shp = t.shape;
    std::vector<std::string> names;
    lineart_tensor_names(c, names);
    if (!has_name(names, t.name)) FAIL(c, "%s: not a tensor of the LineArt generator (n_residual_blocks = 3)", t.cname);
    if (ends_with(t.name, ".bias")) {
        if (t.ndim() != 1) FAIL(c, "%s: unexpected shape", t.cname);
        return upload(c, t.name, t.h, shp, true);
    }
    if (t.ndim() != 4 || shp[2] != shp[3]) FAIL(c, "%s: unexpected shape", t.cname);
    const int ks = (int)shp[2];
    if (starts_with(key, "model3.")) {
        const int Ci = (int)shp[0], Co = (int)shp[1];
        if (ks != 3 || (key == "model3.0.weight" ? (Ci != 256 || Co != 128) : (Ci != 128 || Co != 64))) FAIL(c, "%s: unexpected shape", t.cname);
        return upload(c, t.name, pack_convT_phases(t.h.data(), Ci, Co), {9, Co, Ci});
    }
    const int Co = (int)shp[0], Ci = (int)shp[1], Kp = conv_kp(ks * ks * Ci);
    int eCo = 256, eCi = 256, eks = 3;
    if (key == "model0.1.weight") { eCo = 64; eCi = 3; eks = 7; } else if (key == "model1.0.weight") { eCo = 128; eCi = 64; }
    else if (key == "model1.3.weight") { eCo = 256; eCi = 128; } else if (key == "model4.1.weight") { eCo = 1; eCi = 64; eks = 7; }
    if (Co != eCo || Ci != eCi || ks != eks) FAIL(c, "%s: expected [%d,%d,%d,%d]", t.cname, eCo, eCi, eks, eks);
    return upload(c, t.name, pack_conv(t.h.data(), Co, Ci, ks, ks, Kp), {Co, Kp});
}

namespace {
struct LaWs {                       // one chunk of images; every buffer is [nimg][per-image stride]
    char* in3; float* raw; char* act[3]; float* part; int* cnt; float* stats;
    long act_img, raw_img, in3_img; int tiles_max;
};

// conv (one launch, or the four parity phases of a transposed conv) -> fold -> normalise.  `skip` may be null.
int conv_in_block(car_ctx* c, const LaWs& ws, int nimg, const void* in, long in_img, int Hi, int Wi, int Cin, const std::string& wname, int N,
                  int kind /*0: 7x7 reflect, 1: 3x3 stride 2 zero pad, 2: 3x3 reflect, 3: transposed*/, int relu, const void* skip, void* out, int* Ho_, int* Wo_,
                  hipStream_t st) {
    const char* wp = (const char*)Wp(c, wname);
    if (!wp) FAIL(c, "car_lineart: %s is not loaded", wname.c_str());
    LaConvP p; memset(&p, 0, sizeof(p));
    p.in = in; p.raw = ws.raw; p.part = ws.part; p.cnt = ws.cnt; p.in_img = in_img; p.raw_img = ws.raw_img;
    p.Hi = Hi; p.Wi = Wi; p.Cin = Cin; p.N = N; p.stride = 1; p.os = 1;
    int Ho = Hi, Wo = Wi, tiles_img = 0;
    if (kind != 3) {
        const int ks = kind == 0 ? 7 : 3, pad = ks / 2;
        p.ntaps = ks * ks; p.K = p.ntaps * Cin; p.Kp = conv_kp(p.K); p.reflect = kind != 1;
        for (int t = 0; t < p.ntaps; ++t) { p.dy[t] = (signed char)(t / ks - pad); p.dx[t] = (signed char)(t % ks - pad); }
        if (kind == 1) { p.stride = 2; Ho = (Hi - 1) / 2 + 1; Wo = (Wi - 1) / 2 + 1; }
        p.Hg = Ho; p.Wg = Wo; p.Hout = Ho; p.Wout = Wo; p.w = wp;
        tiles_img = (Ho * Wo + 63) / 64; p.tile0 = 0; p.tiles_img = tiles_img;
        if (tiles_img > ws.tiles_max) FAIL(c, "car_lineart: internal error (partial slots)");
        LACHK(c, car_launch_la_conv(c->mode, &p, nimg, st));
    } else {
        // ConvTranspose2d(k=3, s=2, p=1, output_padding=1) as its four output-parity phases (weight_pack.h convT_phase_taps: 1, 2, 2 and 4 taps): a quarter
        // of the matrix work of convolving the zero-stuffed image.
        Ho = 2 * Hi; Wo = 2 * Wi;
        p.Hg = Hi; p.Wg = Wi; p.Hout = Ho; p.Wout = Wo; p.os = 2; p.reflect = 0;
        const int tp = (Hi * Wi + 63) / 64;
        tiles_img = 4 * tp; p.tiles_img = tiles_img;
        if (tiles_img > ws.tiles_max) FAIL(c, "car_lineart: internal error (partial slots)");
        size_t woff = 0;
        for (int ph = 0; ph < 4; ++ph) {
            p.py = ph >> 1; p.px = ph & 1;
            p.ntaps = convT_phase_taps(ph, p.dy, p.dx); p.K = p.Kp = p.ntaps * Cin;
            p.w = wp + woff * c->esz; p.tile0 = ph * tp;
            LACHK(c, car_launch_la_conv(c->mode, &p, nimg, st));
            woff += (size_t)N * p.Kp;
        }
    }
    LACHK(c, car_launch_la_fold(ws.part, ws.cnt, ws.stats, tiles_img, N, nimg, 1e-5f, st));
    LACHK(c, car_launch_la_norm(c->mode, ws.raw, ws.stats, skip, out, (long)Ho * Wo * N, ws.raw_img, ws.act_img, N, relu, nimg, st));
    *Ho_ = Ho; *Wo_ = Wo;
    return 0;
}
}  // namespace

extern "C" int car_lineart(car_ctx* c, const float* img_nchw, int32_t B, int32_t H, int32_t W, float* out, void* control_out, void* stream_) {
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!img_nchw || B <= 0 || (!out && !control_out)) FAIL(c, "car_lineart: bad arguments");
    // the reference raises below 5: two stride-2 convs leave one row, and ReflectionPad2d(1) needs two
    if (H < 5 || W < 5) FAIL(c, "car_lineart: the image must be at least 5 x 5 (got %d x %d): reflection padding of the residual blocks needs 2 rows and columns", H, W);
    if ((long)H * W > (1L << 26)) FAIL(c, "car_lineart: image too large");
    if (!Wp(c, "lineart.model0.1.weight") || !c->finalized) FAIL(c, "car_lineart: the context holds no LineArt weights (load lineart.* tensors, then car_finalize_weights)");
    const int h1 = (H - 1) / 2 + 1, w1 = (W - 1) / 2 + 1, h2 = (h1 - 1) / 2 + 1, w2 = (w1 - 1) / 2 + 1, Ho = 4 * h2, Wo = 4 * w2;
    const size_t P = (size_t)Ho * Wo, esz = c->esz;
    LaWs ws;
    ws.act_img = (long)P * 64; ws.raw_img = (long)P * 64; ws.in3_img = (long)rup((size_t)H * W * 3, 16);
    ws.tiles_max = (int)((P + 63) / 64) + 4;
    // per-image bytes; InstanceNorm partials: at most tiles_max slots x N x (mean, M2) with slots*N largest on the 64-channel full-resolution layers
    const size_t b_in3 = rup((size_t)ws.in3_img * esz, 256), b_raw = rup((size_t)ws.raw_img * 4, 256), b_act = rup((size_t)ws.act_img * esz, 256);
    const size_t part_img = ((size_t)P / 64 + 8) * 64 * 2 + 4 * 256 * 2;      // floats: covers every layer (slots * N <= P + 4 N at N = 64, 128, 256)
    const size_t b_part = rup(part_img * 4, 256), b_cnt = rup((size_t)ws.tiles_max * 4, 256), b_stats = 256 * 2 * 4;
    const size_t per_img = b_in3 + b_raw + 3 * b_act + b_part + b_cnt + b_stats;
    // chunking: large batches run as groups of images inside a bounded workspace (every step is image-local, so the grouping changes no bit)
    const size_t budget = (size_t)1536 << 20;
    int chunk = (int)std::min<size_t>((size_t)B, std::max<size_t>(1, budget / per_img));
    NEED(c, c->lineart_ws, per_img * chunk);
    char* base = (char*)c->lineart_ws.p;
    ws.in3 = base; base += b_in3 * chunk;
    ws.raw = (float*)base; base += b_raw * chunk;
    for (int i = 0; i < 3; ++i) { ws.act[i] = base; base += b_act * chunk; }
    ws.part = (float*)base; base += b_part * chunk;
    ws.cnt = (int*)base; base += b_cnt * chunk;
    ws.stats = (float*)base;
    // strides between images follow the rounded byte sizes
    ws.in3_img = (long)(b_in3 / esz); ws.raw_img = (long)(b_raw / 4); ws.act_img = (long)(b_act / esz);
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    const std::string L = "lineart.";
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        const float* src = img_nchw + (size_t)b0 * 3 * H * W;
        // model0 input: NHWC in T, one image per in3 slot
        for (int i = 0; i < nb; ++i) LACHK(c, car_launch_la_to_nhwc(c->mode, src + (size_t)i * 3 * H * W, ws.in3 + (size_t)i * ws.in3_img * esz, 1, (long)H * W, st));
        int hh = 0, ww = 0;
        if (conv_in_block(c, ws, nb, ws.in3, ws.in3_img, H, W, 3, L + "model0.1.weight", 64, 0, 1, nullptr, ws.act[0], &hh, &ww, st)) return -1;
        if (conv_in_block(c, ws, nb, ws.act[0], ws.act_img, H, W, 64, L + "model1.0.weight", 128, 1, 1, nullptr, ws.act[1], &hh, &ww, st)) return -1;
        if (conv_in_block(c, ws, nb, ws.act[1], ws.act_img, h1, w1, 128, L + "model1.3.weight", 256, 1, 1, nullptr, ws.act[0], &hh, &ww, st)) return -1;
        int x = 0;                                      // residual stream lives in act[x]
        for (int r = 0; r < 3; ++r) {
            const int t1 = (x + 1) % 3, t2 = (x + 2) % 3;
            const std::string pb = L + "model2." + std::to_string(r) + ".conv_block.";
            if (conv_in_block(c, ws, nb, ws.act[x], ws.act_img, h2, w2, 256, pb + "1.weight", 256, 2, 1, nullptr, ws.act[t1], &hh, &ww, st)) return -1;
            if (conv_in_block(c, ws, nb, ws.act[t1], ws.act_img, h2, w2, 256, pb + "5.weight", 256, 2, 0, ws.act[x], ws.act[t2], &hh, &ww, st)) return -1;
            x = t2;
        }
        const int u1 = (x + 1) % 3, u2 = (x + 2) % 3;
        if (conv_in_block(c, ws, nb, ws.act[x], ws.act_img, h2, w2, 256, L + "model3.0.weight", 128, 3, 1, nullptr, ws.act[u1], &hh, &ww, st)) return -1;
        if (conv_in_block(c, ws, nb, ws.act[u1], ws.act_img, 2 * h2, 2 * w2, 128, L + "model3.3.weight", 64, 3, 1, nullptr, ws.act[u2], &hh, &ww, st)) return -1;
        if (hh != Ho || ww != Wo) FAIL(c, "car_lineart: internal error (output size)");
        const void* w4 = Wp(c, L + "model4.1.weight"); const float* b4 = (const float*)Wp(c, L + "model4.1.bias");
        if (!w4 || !b4) FAIL(c, "car_lineart: lineart.model4.1 is not loaded");
        LACHK(c, car_launch_la_out7(c->mode, ws.act[u2], w4, b4, out ? out + (size_t)b0 * P : nullptr,
                                    control_out ? (char*)control_out + (size_t)b0 * 3 * P * esz : nullptr, Ho, Wo, ws.act_img, nb, st));
    }
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}
