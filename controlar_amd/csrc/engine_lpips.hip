// engine_lpips.hip — car_lpips (LPIPS.forward, tokenizer/tokenizer_image/lpips.py:83-96, in inference), car_psnr and car_recon_to_u8 (the scoring of
// tokenizer/tokenizer_image/reconstruction_vq_ddp.py:128-155) as chains of hed.hip / lpips.hip launches, and the loader of the LPIPS weight images ("lpips.*").
// (one of the translation units behind include/controlar_hip.h; shared declarations: engine_internal.h)
#include "engine_internal.h"
#include "lpips_params.h"

extern "C" {
int car_launch_hed_conv(int mode, const HedConvP* p, int nimg, hipStream_t st);
int car_launch_lpips_to_nhwc(int mode, const float* img, void* out, long out_img, long HW, int nimg, const float* shift, const float* scale, hipStream_t st);
int car_lpips_head_blocks(long P, int C);
int car_launch_lpips_head(int mode, const LpipsHeadP* p, int npairs, hipStream_t st);
int car_launch_lpips_fold(const LpipsFoldP* p, hipStream_t st);
int car_launch_psnr(const void* a, int u8_a, int map_a, const void* b, int u8_b, int map_b, int B, long n, long chunk, int chunks, double data_range,
                    double* psum, double* out, hipStream_t st);
int car_launch_recon_to_u8(const float* x, unsigned char* out, long n, hipStream_t st);
}

#define LPCHK(ctx, x) do { const int _e = (x); if (_e != 0) FAIL(ctx, "car_lpips: %s failed: %s (%s:%d)", #x, hipGetErrorString((hipError_t)_e), __FILE__, __LINE__); } while (0)

// torchvision's vgg16().features[0:30] as lpips.py:118-141 slices it: output channels and 3x3 convs of slice1..5, and the position of every conv in `features`
static const int kCin[5] = {3, 64, 128, 256, 512}, kCout[5] = {64, 128, 256, 512, 512}, kConvs[5] = {2, 2, 3, 3, 3};
static const int kFeat[5][3] = {{0, 2, -1}, {5, 7, -1}, {10, 12, 14}, {17, 19, 21}, {24, 26, 28}};
static const float kShift[3] = {-.030f, -.088f, -.188f}, kScale[3] = {.458f, .448f, .450f};          // ScalingLayer, lpips.py:102-103
static const size_t kBudget = (size_t)1536 << 20;      // bytes of workspace one chunk of pairs may take

static std::string conv_name(int l, int i) { return "lpips.net.slice" + std::to_string(l + 1) + "." + std::to_string(kFeat[l][i]); }
static std::string lin_name(int l) { return "lpips.lin" + std::to_string(l) + ".model.1.weight"; }

// "lpips." + a key of LPIPS().state_dict() (net.sliceS.N.weight, linL.model.1.weight, scaling_layer.shift) or of torchvision's vgg16().features
// (features.N.weight: the trunk is not in the LPIPS checkpoint, lpips.py:59,121) -> the first spelling; false: no tensor of the network.
// *layer / *conv: the slice and the conv's place in it for a trunk tensor, the layer and -1 for a lin, -1 / -1 for the scaling constants.
static bool lpips_canon(const std::string& in, std::string* out, int* layer, int* conv) {
    if (!starts_with(in, "lpips.")) return false;
    const std::string k = in.substr(6);
    *layer = *conv = -1;
    if (k == "scaling_layer.shift" || k == "scaling_layer.scale") { *out = in; return true; }
    for (int l = 0; l < 5; ++l) if (in == lin_name(l)) { *out = in; *layer = l; return true; }
    const char* sfx = ends_with(k, ".weight") ? ".weight" : ends_with(k, ".bias") ? ".bias" : nullptr;
    if (!sfx) return false;
    const std::string stem = k.substr(0, k.size() - strlen(sfx));
    for (int l = 0; l < 5; ++l) for (int i = 0; i < kConvs[l]; ++i) {
        const std::string n = std::to_string(kFeat[l][i]);
        if (stem == "features." + n || stem == "net.slice" + std::to_string(l + 1) + "." + n) { *out = conv_name(l, i) + sfx; *layer = l; *conv = i; return true; }
    }
    return false;
}
extern "C" int car_debug_lpips_canonical_name(const char* name, char* out, int32_t cap) {      // host-only helper (tests): 0 and the stored name, or -1
    std::string o; int l, i;
    if (!name || !out || cap <= 0 || !lpips_canon(name, &o, &l, &i) || (int)o.size() >= cap) return -1;
    memcpy(out, o.c_str(), o.size() + 1);
    return 0;
}

// the 31 tensors car_lpips needs; scaling_layer.shift / .scale are optional (host tables: the constants of lpips.py:102-103 otherwise)
void lpips_tensor_names(const car_ctx*, std::vector<std::string>& v) {
    for (int l = 0; l < 5; ++l) for (int i = 0; i < kConvs[l]; ++i) for (const char* s : {".weight", ".bias"}) v.push_back(conv_name(l, i) + s);
    for (int l = 0; l < 5; ++l) v.push_back(lin_name(l));
}

// conv weights become the implicit-GEMM images hed_load_tensor builds ([Cout][9*Cin], K padded to the 32-wide k step) in the context's element type;
// biases and the lin vectors stay fp32 (the head computes in fp32 in both modes)
int lpips_load_tensor(car_ctx* c, const LoadedTensor& t) {
    std::string name; int l, i;
    if (!lpips_canon(t.name, &name, &l, &i)) FAIL(c, "%s: not a tensor of the LPIPS network (lpips.net.sliceS.N / lpips.features.N, lpips.linL.model.1.weight, lpips.scaling_layer.*)", t.cname);
    const std::vector<int64_t>& shp = t.shape;
    if (l < 0) { if (t.n != 3) FAIL(c, "%s: expected [1,3,1,1]", t.cname); c->host_keep[name] = t.h; return 0; }
    const int Co = kCout[l];
    if (i < 0) {
        if (t.ndim() != 4 || shp[0] != 1 || shp[1] != Co || shp[2] != 1 || shp[3] != 1) FAIL(c, "%s: expected [1,%d,1,1]", t.cname, Co);
        return upload(c, name, t.h, {Co}, true);
    }
    if (ends_with(name, ".bias")) { if (t.ndim() != 1 || shp[0] != Co) FAIL(c, "%s: expected [%d]", t.cname, Co); return upload(c, name, t.h, shp, true); }
    const int Ci = i == 0 ? kCin[l] : Co, Kp = conv_kp(9 * Ci);
    if (t.ndim() != 4 || shp[0] != Co || shp[1] != Ci || shp[2] != 3 || shp[3] != 3) FAIL(c, "%s: expected [%d,%d,3,3]", t.cname, Co, Ci);
    return upload(c, name, pack_conv(t.h.data(), Co, Ci, 3, 3, Kp), {Co, Kp});
}

// per-pair workspace bytes: both images' NHWC input and two rotating activation buffers (the largest map is 64 channels at full resolution), the head partials
struct LpipsPlan { size_t b_in3, b_act, per_pair; int nblk[5]; int chunk; };
static LpipsPlan lpips_plan(size_t esz, int H, int W) {
    LpipsPlan q; const size_t P = (size_t)H * W;
    q.b_in3 = rup(P * 3 * esz, 256); q.b_act = rup(P * 64 * esz, 256);
    size_t parts = 0;
    for (int l = 0; l < 5; ++l) { q.nblk[l] = car_lpips_head_blocks((long)(H >> l) * (W >> l), kCout[l]); parts += (size_t)q.nblk[l] * sizeof(double); }
    q.per_pair = 2 * (q.b_in3 + 2 * q.b_act) + rup(parts, 256);
    // a chunk holds whole pairs; its 2 * chunk images ride on grid.z of the convolutions
    q.chunk = (int)std::min<size_t>(32767, std::max<size_t>(1, kBudget / q.per_pair));
    return q;
}
extern "C" int car_debug_lpips_chunk_pairs(int32_t mode, int32_t H, int32_t W) {      // host-only helper (tests): pairs per chunk, or -1
    if ((mode != CAR_F32 && mode != CAR_BF16) || H < 16 || W < 16 || (long)H * W > (1L << 26)) return -1;
    return lpips_plan(mode == CAR_F32 ? 4 : 2, H, W).chunk;
}

extern "C" int car_lpips(car_ctx* c, const float* a_nchw, const float* b_nchw, int32_t B, int32_t H, int32_t W, double* out, double* layers_out, void* stream_) {
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!a_nchw || !b_nchw || !out || B <= 0) FAIL(c, "car_lpips: bad arguments");
    if (H < 16 || W < 16) FAIL(c, "car_lpips: the images must be at least 16 x 16 (got %d x %d): four 2x2 max-pools leave no pixel below that", H, W);
    if ((long)H * W > (1L << 26)) FAIL(c, "car_lpips: image too large");
    if (!Wp(c, lin_name(0)) || !c->finalized) FAIL(c, "car_lpips: the context holds no LPIPS weights (load lpips.* tensors, then car_finalize_weights)");
    const size_t P = (size_t)H * W, esz = c->esz;
    const LpipsPlan q = lpips_plan(esz, H, W);
    // chunking: large batches run as groups of pairs inside a bounded workspace (every step is pair-local, so the grouping changes no bit)
    const int chunk = std::min(q.chunk, (int)B);
    NEED(c, c->lpips_ws, q.per_pair * chunk);
    char* base = (char*)c->lpips_ws.p;
    char* in3 = base; base += 2 * q.b_in3 * chunk;
    char* act[2]; for (int i = 0; i < 2; ++i) { act[i] = base; base += 2 * q.b_act * chunk; }
    double* part[5]; for (int l = 0; l < 5; ++l) { part[l] = (double*)base; base += (size_t)q.nblk[l] * sizeof(double) * chunk; }
    const long in3_img = (long)(q.b_in3 / esz), act_img = (long)(q.b_act / esz);
    const float *shift = kShift, *scale = kScale;
    { auto s = c->host_keep.find("lpips.scaling_layer.shift"); if (s != c->host_keep.end()) shift = s->second.data();
      s = c->host_keep.find("lpips.scaling_layer.scale"); if (s != c->host_keep.end()) scale = s->second.data(); }
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        // image 2i of the chunk is `a` of pair b0 + i, image 2i + 1 its `b`: both go through the trunk in the same launches
        LPCHK(c, car_launch_lpips_to_nhwc(c->mode, a_nchw + (size_t)b0 * 3 * P, in3, 2 * in3_img, (long)P, nb, shift, scale, st));
        LPCHK(c, car_launch_lpips_to_nhwc(c->mode, b_nchw + (size_t)b0 * 3 * P, in3 + (size_t)in3_img * esz, 2 * in3_img, (long)P, nb, shift, scale, st));
        LpipsFoldP f; memset(&f, 0, sizeof(f));
        const void* cur = in3; long cur_img = in3_img; int x = 0;
        for (int l = 0; l < 5; ++l) {
            const int Hl = H >> l, Wl = W >> l;
            for (int i = 0; i < kConvs[l]; ++i) {
                const std::string cv = conv_name(l, i);
                HedConvP p; memset(&p, 0, sizeof(p));
                p.in = cur; p.in_img = cur_img; p.out = act[x]; p.out_img = act_img;
                p.w = Wp(c, cv + ".weight"); p.bias = (const float*)Wp(c, cv + ".bias");
                if (!p.w || !p.bias) FAIL(c, "car_lpips: %s is not loaded", cv.c_str());
                p.Cin = i == 0 ? kCin[l] : kCout[l]; p.N = kCout[l]; p.K = 9 * p.Cin; p.Kp = conv_kp(p.K);
                p.pool = (i == 0 && l > 0) ? 1 : 0;
                p.H = Hl; p.W = Wl; p.Hi = p.pool ? H >> (l - 1) : Hl; p.Wi = p.pool ? W >> (l - 1) : Wl;
                LPCHK(c, car_launch_hed_conv(c->mode, &p, 2 * nb, st));
                cur = act[x]; cur_img = act_img; x ^= 1;
            }
            // the tap of slice l is the buffer just written: its head runs here, before the next slice's second conv overwrites it
            LpipsHeadP h; memset(&h, 0, sizeof(h));
            h.act = cur; h.img = act_img; h.lin = (const float*)Wp(c, lin_name(l)); h.part = part[l]; h.nblk = q.nblk[l]; h.P = (long)Hl * Wl; h.C = kCout[l];
            if (!h.lin) FAIL(c, "car_lpips: %s is not loaded", lin_name(l).c_str());
            LPCHK(c, car_launch_lpips_head(c->mode, &h, nb, st));
            f.part[l] = part[l]; f.nblk[l] = q.nblk[l]; f.count[l] = (double)Hl * Wl;
        }
        f.out = out + b0; f.layers = layers_out ? layers_out + (size_t)b0 * LP_LAYERS : nullptr; f.npairs = nb;
        LPCHK(c, car_launch_lpips_fold(&f, st));
    }
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}

static bool psnr_dtype_ok(int dt) { return dt == CAR_DT_F32 || dt == CAR_DT_U8; }
static bool psnr_map_ok(int m) { return m == LP_MAP_RAW || m == LP_MAP_DIV255 || m == LP_MAP_HALF; }

extern "C" int car_psnr(car_ctx* c, const void* a, int32_t a_dtype, int32_t a_map, const void* b, int32_t b_dtype, int32_t b_map, int32_t B, int64_t n,
                        double data_range, double* out, void* stream_) {
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!a || !b || !out) FAIL(c, "car_psnr: a, b and out must not be NULL");
    if (!psnr_dtype_ok(a_dtype) || !psnr_dtype_ok(b_dtype)) FAIL(c, "car_psnr: inputs are fp32 (0) or uint8 (4), got dtypes %d and %d", a_dtype, b_dtype);
    if (!psnr_map_ok(a_map) || !psnr_map_ok(b_map)) FAIL(c, "car_psnr: a map is 0 (v), 1 (v / 255) or 2 ((v + 1) / 2), got %d and %d", a_map, b_map);
    if (B <= 0 || n <= 0 || B > 65535) FAIL(c, "car_psnr: sizes must be positive and B at most 65535 (got B %d, %lld elements per image)", B, (long long)n);
    if (!(data_range > 0.0)) FAIL(c, "car_psnr: data_range must be positive (got %g)", data_range);
    // an image of n elements in at most 1024 chunks of at least 8192 elements: a block reduces one chunk
    long chunk = 8192;
    while (((long)n + chunk - 1) / chunk > 1024) chunk *= 2;
    const int chunks = (int)(((long)n + chunk - 1) / chunk);
    NEED(c, c->metrics_ws, (size_t)B * chunks * sizeof(double));
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    (void)car_launch_psnr(a, a_dtype == CAR_DT_U8, a_map, b, b_dtype == CAR_DT_U8, b_map, B, (long)n, chunk, chunks, data_range, (double*)c->metrics_ws.p, out, st);
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int car_recon_to_u8(car_ctx* c, const float* x, int64_t n, uint8_t* out, void* stream_) {
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!x || !out || n <= 0) FAIL(c, "car_recon_to_u8: x and out must not be NULL and n positive");
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    (void)car_launch_recon_to_u8(x, out, (long)n, st);
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}
