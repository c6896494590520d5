// engine_depth.hip — car_depth_configure / car_depth: the DPT depth estimator (transformers modeling_dpt.py DPTForDepthEstimation; callers
// sample_t2i.py:33,114-116,133-139, demo/model.py:192-284).  The ViT backbone runs on the launchers car_encode_control uses (a second layer loop: the
// first one keeps its bits untouched); the neck and the head run on dpt.hip.  The loader of the weight images ("depth.*") is here too.
// (one of the translation units behind include/controlar_hip.h; shared declarations: engine_internal.h)
#include "engine_internal.h"

extern "C" {
int car_launch_dpt_patchify(int mode, const float* img, void* out, int nimg, int S, hipStream_t st);
int car_launch_dpt_conv(int mode, const DptConvP* p, int nimg, hipStream_t st);
int car_launch_dpt_shuffle(int mode, const void* in, void* out, int nimg, int g, int k, int C, hipStream_t st);
int car_launch_dpt_up2(int mode, const void* in, void* out, int nimg, int h, int w, int C, hipStream_t st);
int car_launch_dpt_max(const float* map, long map_img, float* mx, int nimg, long P, hipStream_t st);
int car_launch_dpt_control(int mode, const float* map, long map_img, const float* mx, void* control, int nimg, long P, hipStream_t st);
}

#define DPTCHK(ctx, x) do { const int _e = (x); if (_e != 0) FAIL(ctx, "car_depth: %s failed: %s (%s:%d)", #x, hipGetErrorString((hipError_t)_e), __FILE__, __LINE__); } while (0)

extern "C" int car_depth_configure(car_ctx* c, const car_dpt_config* d) {
    if (!c || !d) { if (c) c->err = "car_depth_configure: null argument"; return -1; }
    if (d->hidden <= 0 || d->layers <= 0 || d->heads <= 0 || d->mlp <= 0 || d->pos_grid <= 0 || d->fusion_hidden <= 0 || !(d->ln_eps > 0.f))
        FAIL(c, "car_depth_configure: non-positive field");
    for (int i = 0; i < 8; ++i) if (d->reserved[i]) FAIL(c, "car_depth_configure: reserved fields must be zero");
    if (d->hidden % 32 || d->mlp % 32 || d->hidden % d->heads || (d->hidden / d->heads) % 32 || d->hidden > 16384 || d->pos_grid > 256)
        FAIL(c, "car_depth_configure: hidden, mlp and hidden/heads must be multiples of 32 (hidden <= 16384, pos_grid <= 256)");
    if (c->mode == CAR_BF16 && d->hidden / d->heads != 64)
        FAIL(c, "car_depth_configure: the bf16 mode runs the backbone's attention on the fused 64-wide-head kernel; hidden/heads = %d is outside it", d->hidden / d->heads);
    for (int i = 0; i < 4; ++i) {
        if (d->out_indices[i] < 0 || d->out_indices[i] >= d->layers || (i && d->out_indices[i] <= d->out_indices[i - 1]))
            FAIL(c, "car_depth_configure: out_indices must be four increasing layer indices in [0, %d)", d->layers);
        if (d->neck_hidden[i] <= 0 || d->neck_hidden[i] % 32) FAIL(c, "car_depth_configure: neck_hidden[%d] = %d must be a positive multiple of 32", i, d->neck_hidden[i]);
    }
    if (d->fusion_hidden % 64) FAIL(c, "car_depth_configure: fusion_hidden must be a multiple of 64 (the head halves it in front of a 3x3 conv)");
    if (c->has_dpt && memcmp(&c->dpt, d, sizeof(*d)) != 0)
        for (auto& kv : c->w) if (starts_with(kv.first, "depth.")) FAIL(c, "car_depth_configure: the context already holds depth.* tensors of another configuration");
    c->dpt = *d; c->has_dpt = true;
    return 0;
}

// every tensor the configured DPT needs, under its "depth." name
void depth_tensor_names(const car_ctx* c, std::vector<std::string>& v) {
    const car_dpt_config& d = c->dpt;
    const std::string e = "depth.dpt.embeddings.";
    for (const char* s : {"cls_token", "position_embeddings", "patch_embeddings.projection.weight", "patch_embeddings.projection.bias"}) v.push_back(e + s);
    for (int l = 0; l < d.layers; ++l) {
        const std::string p = "depth.dpt.encoder.layer." + std::to_string(l) + ".";
        for (const char* m : {"attention.attention.query", "attention.attention.key", "attention.attention.value", "attention.output.dense", "intermediate.dense",
                              "output.dense", "layernorm_before", "layernorm_after"}) for (const char* s : {".weight", ".bias"}) v.push_back(p + m + s);
    }
    const std::string r = "depth.neck.reassemble_stage.";
    for (int i = 0; i < 4; ++i) {
        const std::string is = std::to_string(i);
        for (const char* s : {".weight", ".bias"}) {
            v.push_back(r + "readout_projects." + is + ".0" + s);
            v.push_back(r + "layers." + is + ".projection" + s);
            if (i != 2) v.push_back(r + "layers." + is + ".resize" + s);
        }
        v.push_back("depth.neck.convs." + is + ".weight");
        const std::string f = "depth.neck.fusion_stage.layers." + is + ".";
        for (const char* m : {"projection", "residual_layer1.convolution1", "residual_layer1.convolution2", "residual_layer2.convolution1", "residual_layer2.convolution2"})
            for (const char* s : {".weight", ".bias"}) v.push_back(f + m + s);
    }
    for (const char* m : {"0", "2", "4"}) for (const char* s : {".weight", ".bias"}) v.push_back(std::string("depth.head.head.") + m + s);
}

// Linear weights, LayerNorm parameters and every bias a car_launch_gemm epilogue adds stay [N, K] / [N] in the context's element type; 1x1 convs drop their
// trailing 1x1; 3x3 conv weights become implicit-GEMM images [Cout][9*Cin] (k = tap*Cin + ci); a ConvTranspose2d(k = stride) weight [Cin, Cout, k, k] becomes
// the GEMM image [(ky*k + kx)*Cout + co][ci] and its bias is replicated per tap; the biases dpt_conv adds in its fp32 epilogue stay fp32; position_embeddings
// stays on the host (resized per grid).
int depth_load_tensor(car_ctx* c, const LoadedTensor& t) {
    const std::string& name = t.name; const char* cname = t.cname;
    const std::vector<int64_t>& shp = t.shape; const std::vector<float>& h = t.h;
    if (!c->has_dpt) FAIL(c, "%s: call car_depth_configure before loading depth.* tensors", cname);
    if (starts_with(name, "depth.dpt.layernorm.") || starts_with(name, "depth.dpt.pooler.")) return 0;     // never reach the depth map
    const car_dpt_config& d = c->dpt;
    std::vector<std::string> names;
    depth_tensor_names(c, names);
    if (!has_name(names, name)) FAIL(c, "%s: not a tensor of the configured DPT depth estimator (DPTForDepthEstimation)", cname);
    const std::string key = name.substr(6);
    const int64_t D = d.hidden, Fh = d.fusion_hidden, G = d.pos_grid;
    auto is_shape = [&](std::initializer_list<int64_t> ex) { return shp.size() == ex.size() && std::equal(ex.begin(), ex.end(), shp.begin()); };
    auto conv3 = [&](int64_t Co, int64_t Ci) -> int {
        if (!is_shape({Co, Ci, 3, 3})) FAIL(c, "%s: expected [%lld,%lld,3,3]", cname, (long long)Co, (long long)Ci);
        return upload(c, name, pack_conv(h.data(), (int)Co, (int)Ci, 3, 3, (int)(9 * Ci)), {Co, 9 * Ci});
    };
    auto vec = [&](int64_t N, bool f32) -> int { if (!is_shape({N})) FAIL(c, "%s: expected [%lld]", cname, (long long)N); return upload(c, name, h, shp, f32); };
    auto mat = [&](int64_t N, int64_t K) -> int {          // Linear [N,K] or 1x1 conv [N,K,1,1]
        if (!is_shape({N, K}) && !is_shape({N, K, 1, 1})) FAIL(c, "%s: expected [%lld,%lld]", cname, (long long)N, (long long)K);
        return upload(c, name, h, {N, K});
    };
    const bool isw = ends_with(name, ".weight");
    int i = -1;
    if (key == "dpt.embeddings.cls_token") { if (t.n != D) FAIL(c, "%s: expected [1,1,%lld]", cname, (long long)D); return upload(c, name, h, {D}); }
    if (key == "dpt.embeddings.position_embeddings") {
        if (t.n != (G * G + 1) * D) FAIL(c, "%s: expected [1,%lld,%lld]", cname, (long long)(G * G + 1), (long long)D);
        for (auto& kv : c->depth_pos_cache) (void)hipFree(kv.second);
        c->depth_pos_cache.clear(); c->host_keep[name] = h; return 0;
    }
    if (key == "dpt.embeddings.patch_embeddings.projection.weight") { if (!is_shape({D, 3, 16, 16})) FAIL(c, "%s: expected [%lld,3,16,16]", cname, (long long)D); return upload(c, name, h, {D, 768}); }
    if (key == "dpt.embeddings.patch_embeddings.projection.bias") return vec(D, false);
    if (starts_with(key, "dpt.encoder.layer.")) {
        if (ends_with(key, "intermediate.dense.weight")) return mat(d.mlp, D);
        if (ends_with(key, "intermediate.dense.bias")) return vec(d.mlp, false);
        if (ends_with(key, "attention.output.dense.weight")) return mat(D, D);
        if (ends_with(key, "output.dense.weight")) return mat(D, d.mlp);
        if (isw && key.find("layernorm_") == std::string::npos) return mat(D, D);
        return vec(D, false);
    }
    if (sscanf(key.c_str(), "neck.reassemble_stage.readout_projects.%d.", &i) == 1) return isw ? mat(D, 2 * D) : vec(D, false);
    if (sscanf(key.c_str(), "neck.reassemble_stage.layers.%d.", &i) == 1) {
        const int64_t Ci = d.neck_hidden[i];
        if (key.find(".projection.") != std::string::npos) return isw ? mat(Ci, D) : vec(Ci, false);
        if (i == 3) return isw ? conv3(Ci, Ci) : vec(Ci, true);
        const int k = i == 0 ? 4 : 2;
        if (!isw) {
            if (!is_shape({Ci})) FAIL(c, "%s: expected [%lld]", cname, (long long)Ci);
            return upload(c, name, pack_convT_taps_bias(h.data(), (int)Ci, k), {(int64_t)k * k * Ci});
        }
        if (!is_shape({Ci, Ci, k, k})) FAIL(c, "%s: expected [%lld,%lld,%d,%d]", cname, (long long)Ci, (long long)Ci, k, k);
        return upload(c, name, pack_convT_taps(h.data(), (int)Ci, (int)Ci, k), {(int64_t)k * k * Ci, Ci});
    }
    if (sscanf(key.c_str(), "neck.convs.%d.", &i) == 1) return conv3(Fh, d.neck_hidden[i]);
    if (starts_with(key, "neck.fusion_stage.layers.")) {
        if (key.find(".projection.") != std::string::npos) return isw ? mat(Fh, Fh) : vec(Fh, false);
        return isw ? conv3(Fh, Fh) : vec(Fh, true);
    }
    if (key == "head.head.0.weight") return conv3(Fh / 2, Fh);
    if (key == "head.head.0.bias") return vec(Fh / 2, true);
    if (key == "head.head.2.weight") return conv3(32, Fh / 2);
    if (key == "head.head.2.bias") return vec(32, true);
    if (key == "head.head.4.weight") { if (!is_shape({1, 32, 1, 1})) FAIL(c, "%s: expected [1,32,1,1]", cname); return upload(c, name, h, {32}); }
    if (key == "head.head.4.bias") return vec(1, true);
    FAIL(c, "%s: not a tensor of the configured DPT depth estimator", cname);
}

// DPTViTEmbeddings._resize_pos_embed: the grid part through F.interpolate(mode="bilinear") (align_corners = False, no antialiasing), the CLS row untouched;
// in fp32, once per token grid
static int get_depth_pos(car_ctx* c, int g, void** out) {
    auto it = c->depth_pos_cache.find(g);
    if (it != c->depth_pos_cache.end()) { *out = it->second; return 0; }
    auto pit = c->host_keep.find("depth.dpt.embeddings.position_embeddings");
    const int D = c->dpt.hidden, G = c->dpt.pos_grid;
    if (pit == c->host_keep.end() || (int64_t)pit->second.size() != (int64_t)(G * G + 1) * D) FAIL(c, "car_depth: depth.dpt.embeddings.position_embeddings is not loaded");
    const std::vector<float>& pe = pit->second;
    std::vector<float> o((size_t)(g * g + 1) * D);
    memcpy(o.data(), pe.data(), (size_t)D * 4);
    std::vector<int> i0(g), i1(g); std::vector<float> l1(g);
    const float sc = (float)G / (float)g;
    for (int d = 0; d < g; ++d) {
        float src = sc * ((float)d + 0.5f) - 0.5f; if (src < 0.f) src = 0.f;
        int a = (int)src; if (a > G - 1) a = G - 1;
        i0[d] = a; i1[d] = a < G - 1 ? a + 1 : a; l1[d] = src - (float)a;
    }
    for (int y = 0; y < g; ++y) for (int x = 0; x < g; ++x) {
        const float ly1 = l1[y], ly0 = 1.f - ly1, lx1 = l1[x], lx0 = 1.f - lx1;
        const float* v00 = &pe[(size_t)(1 + i0[y] * G + i0[x]) * D]; const float* v01 = &pe[(size_t)(1 + i0[y] * G + i1[x]) * D];
        const float* v10 = &pe[(size_t)(1 + i1[y] * G + i0[x]) * D]; const float* v11 = &pe[(size_t)(1 + i1[y] * G + i1[x]) * D];
        float* dst = &o[(size_t)(1 + y * g + x) * D];
        for (int d = 0; d < D; ++d) dst[d] = ly0 * (lx0 * v00[d] + lx1 * v01[d]) + ly1 * (lx0 * v10[d] + lx1 * v11[d]);
    }
    void* dp = nullptr;
    const size_t bytes = o.size() * c->esz;
    HIPCHK(c, hipMalloc(&dp, bytes));
    hipError_t e;
    if (c->mode == CAR_F32) e = hipMemcpy(dp, o.data(), bytes, hipMemcpyHostToDevice);
    else { std::vector<bf16_t> hb(o.size()); for (size_t i = 0; i < o.size(); ++i) hb[i] = f2bf(o[i]); e = hipMemcpy(dp, hb.data(), bytes, hipMemcpyHostToDevice); }
    if (e != hipSuccess) { (void)hipFree(dp); FAIL(c, "car_depth: upload of the position embeddings failed: %s", hipGetErrorString(e)); }
    c->depth_pos_cache[g] = dp; *out = dp;
    return 0;
}

extern "C" int car_depth(car_ctx* c, const float* pixel_values, int32_t B, int32_t H, int32_t W, float* out, void* control_out, void* stream_) {
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (B <= 0) FAIL(c, "car_depth: bad arguments");
    if (!c->has_dpt || !c->finalized || !Wp(c, "depth.head.head.4.weight"))
        FAIL(c, "car_depth: the context holds no DPT weights (car_depth_configure, load depth.* tensors, then car_finalize_weights)");
    if (H != W) FAIL(c, "car_depth: the image must be square (got %d x %d): the reference's reassemble stage takes the square root of the token count", H, W);
    if (H < 32 || H % 32 || H > 4096) FAIL(c, "car_depth: the side must be a multiple of 32 in [32, 4096] (got %d): the token grid has to be even", H);
    if (!pixel_values || (!out && !control_out)) FAIL(c, "car_depth: bad arguments (no image, or neither output)");
    const car_dpt_config& d = c->dpt;
    const int mode = c->mode; const size_t e = c->esz;
    const int S = H, g = S / 16, n = g * g, Tn = n + 1, D = d.hidden, nh = d.heads, hd = D / nh, F = d.fusion_hidden;
    const int Kp = 768, Tpad = (int)rup(Tn, 32);
    const size_t P = (size_t)S * S;
    void* pos = nullptr; if (get_depth_pos(c, g, &pos)) return -1;
    const bool flash = use_flash(c, hd);
    if (mode == CAR_BF16 && !flash) FAIL(c, "car_depth: the bf16 mode needs the fused 64-wide-head attention kernel");
    // per-image elements of the neck: the four fused-width feature maps, three rotating buffers that hold every other activation (the largest is the
    // head's up-sampled map, S x S x F/2), the fp32 map
    int maxC = 0; for (int i = 0; i < 4; ++i) maxC = std::max(maxC, d.neck_hidden[i]);
    const int lvl[4] = {4 * g, 2 * g, g, g / 2};                      // side of reassembled feature i
    size_t b_f[4], b_fs = 0;
    for (int i = 0; i < 4; ++i) { b_f[i] = rup((size_t)lvl[i] * lvl[i] * F * e, 256); b_fs += b_f[i]; }
    size_t big = (size_t)128 * n * F;
    big = std::max(big, (size_t)n * D); big = std::max(big, (size_t)16 * n * d.neck_hidden[0]); big = std::max(big, (size_t)4 * n * d.neck_hidden[1]); big = std::max(big, (size_t)n * maxC);
    const size_t b_big = rup(big * e, 256), b_map = rup(P * 4, 256), b_cls = rup((size_t)D * e, 256);
    const size_t per_img = b_fs + 3 * b_big + b_map + b_cls + 256;
    // chunking: every step is image-local, so the grouping changes no bit.  The backbone follows car_encode_control's rule (the exact mode holds fp32 scores
    // and probabilities of a chunk), the neck a workspace budget.
    int chmax = flash ? 64 : 96;
    if (!flash) while (chmax > 1 && (size_t)chmax * nh * Tn * (size_t)(Tn + Tpad) * 4 > ((size_t)6 << 30)) chmax /= 2;
    const size_t budget = (size_t)8 << 30;
    const int CH = (int)std::min<size_t>(std::min<size_t>((size_t)B, (size_t)chmax), std::max<size_t>(1, budget / per_img));
    NEED(c, c->depth_ws, per_img * CH);
    char* base = (char*)c->depth_ws.p;
    char* feat[4]; for (int i = 0; i < 4; ++i) { feat[i] = base; base += b_f[i] * CH; }
    char* rot[3]; for (int i = 0; i < 3; ++i) { rot[i] = base; base += b_big * CH; }
    float* wmap = (float*)base; base += b_map * CH;
    char* vcls = base; base += b_cls * CH;
    float* mx = (float*)base;
    NEED(c, c->ws[0], (size_t)CH * n * Kp * e);            // patches
    NEED(c, c->ws[1], (size_t)CH * Tn * D * e);            // h
    NEED(c, c->ws[2], (size_t)CH * Tn * D * e);            // y (normed) / tok
    NEED(c, c->ws[3], (size_t)CH * Tn * 3 * D * e);        // q | k | v (separate planes)
    const AttnBytes ab = attn_bytes(c, CH, Tn, nh, hd);
    if (ab.S) NEED(c, c->ws[WS_ATTN_S], ab.S);                     // S fp32
    if (ab.P) NEED(c, c->ws[WS_ATTN_P], ab.P);                     // P
    NEED(c, c->ws[WS_ATTN_VT], ab.Vt);                              // V^T
    NEED(c, c->ws[7], (size_t)CH * Tn * d.mlp * e);        // mlp mid
    NEED(c, c->ws[8], (size_t)CH * Tn * D * e);            // ctx
    // development build only: time the backbone alone (outputs are not written), and the reference's order up-sample -> 1x1 projection (DPT section)
    const bool bb_only = CAR_KNOB("CAR_DEPTH_BACKBONE_ONLY") != nullptr, up_first = CAR_KNOB("CAR_DEPTH_UP_FIRST") != nullptr;
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    const std::string a = "depth.dpt.", rs = "depth.neck.reassemble_stage.";
    auto W_ = [&](const std::string& nm) { return Wp(c, nm); };
    // one 3x3 conv launch on dense per-image maps
    auto conv = [&](const void* in, int Hi, int Cin, int stride, const std::string& wname, bool bias, int N, void* o, int relu_in, int relu_out,
                    const void* r1, const void* r2, int nb) -> int {
        DptConvP p; memset(&p, 0, sizeof(p));
        p.in = in; p.w = W_(wname + ".weight"); p.bias = bias ? (const float*)W_(wname + ".bias") : nullptr; p.out = o;
        if (!p.w || (bias && !p.bias)) FAIL(c, "car_depth: %s is not loaded", wname.c_str());
        p.Hi = p.Wi = Hi; p.H = p.W = stride == 1 ? Hi : (Hi - 1) / 2 + 1; p.Cin = Cin; p.N = N; p.K = 9 * Cin; p.stride = stride; p.relu_in = relu_in; p.relu_out = relu_out;
        p.in_img = (long)Hi * Hi * Cin; p.out_img = (long)p.H * p.W * N; p.res1 = r1; p.res2 = r2; p.res1_img = p.res2_img = p.out_img;
        DPTCHK(c, car_launch_dpt_conv(mode, &p, nb, st));
        return 0;
    };
    for (int b0 = 0; b0 < B; b0 += CH) {
        const int nb = std::min(CH, B - b0);
        void *patches = c->ws[0].p, *h = c->ws[1].p, *y = c->ws[2].p, *qkv = c->ws[3].p, *mid = c->ws[7].p, *ctx = c->ws[8].p;
        DPTCHK(c, car_launch_dpt_patchify(mode, pixel_values + (size_t)b0 * 3 * P, patches, nb, S, st));
        {   // patch projection -> y used as the token buffer, then cls | tokens + resized position embeddings (DPTViTEmbeddings.forward)
            GemmP q = gp(patches, Kp, W_(a + "embeddings.patch_embeddings.projection.weight"), Kp, y, D, nb * n, D, Kp);
            q.bias = W_(a + "embeddings.patch_embeddings.projection.bias"); q.bias_mode = BIAS_N;
            car_launch_gemm(mode, AMODE_PLAIN, &q, st);
        }
        car_launch_vit_assemble(mode, y, W_(a + "embeddings.cls_token"), pos, h, nb, n, D, st);
        const long rows = (long)nb * Tn;
        void* qp = qkv; void* kp = off(qkv, (size_t)rows * D, e); void* vp = off(qkv, (size_t)2 * rows * D, e);
        int tap = 0;
        for (int l = 0; l <= d.out_indices[3]; ++l) {          // DPTViTLayer.forward; layers past the last tap reach nothing
            const std::string L = a + "encoder.layer." + std::to_string(l) + ".";
            car_launch_layernorm(mode, h, W_(L + "layernorm_before.weight"), W_(L + "layernorm_before.bias"), y, rows, D, d.ln_eps, st);
            const char* names[3] = {"query", "key", "value"}; void* dst[3] = {qp, kp, vp};
            for (int t = 0; t < 3; ++t) {
                GemmP q = gp(y, D, W_(L + "attention.attention." + names[t] + ".weight"), D, dst[t], D, (int)rows, D, D);
                q.bias = W_(L + "attention.attention." + std::string(names[t]) + ".bias"); q.bias_mode = BIAS_N;
                car_launch_gemm(mode, AMODE_PLAIN, &q, st);
            }
            {   // ctx = softmax(Q K^T * hd^-0.5) V   (eager_attention_forward; softmax in fp32)
                const AttnCall at = {qp, kp, vp, D, ctx, nb, Tn, nh, hd, 1.0f / std::sqrt((float)hd), ATTN_NONE, nullptr, nullptr, 0};
                if (attn_run(c, at, st)) FAIL(c, "car_depth: the fused attention kernel refused %d tokens x %d heads", Tn, nh);
            }
            {   // h = dense(ctx) + h
                GemmP q = gp(ctx, D, W_(L + "attention.output.dense.weight"), D, h, D, (int)rows, D, D);
                q.bias = W_(L + "attention.output.dense.bias"); q.bias_mode = BIAS_N; q.R = h; q.ldr = D;
                car_launch_gemm(mode, AMODE_PLAIN, &q, st);
            }
            car_launch_layernorm(mode, h, W_(L + "layernorm_after.weight"), W_(L + "layernorm_after.bias"), y, rows, D, d.ln_eps, st);
            {   // erf-GELU MLP, h = output.dense(gelu(intermediate.dense(y))) + h
                GemmP q = gp(y, D, W_(L + "intermediate.dense.weight"), D, mid, d.mlp, (int)rows, d.mlp, D);
                q.bias = W_(L + "intermediate.dense.bias"); q.bias_mode = BIAS_N; q.act = ACT_GELU_ERF;
                car_launch_gemm(mode, AMODE_PLAIN, &q, st);
                GemmP r = gp(mid, d.mlp, W_(L + "output.dense.weight"), d.mlp, h, D, (int)rows, D, d.mlp);
                r.bias = W_(L + "output.dense.bias"); r.bias_mode = BIAS_N; r.R = h; r.ldr = D;
                car_launch_gemm(mode, AMODE_PLAIN, &r, st);
            }
            if (!bb_only && tap < 4 && l == d.out_indices[tap]) {
                // ---- reassemble tap `tap` from h (hidden_states[1:][l], before dpt.layernorm) while it is still there
                const std::string is = std::to_string(tap);
                const int Ci = d.neck_hidden[tap];
                const void* wro = W_(rs + "readout_projects." + is + ".0.weight");
                {   // readout "project": GELU(W[:, :D] tok + (W[:, D:] cls + b)) — the second term is one vector per image, the concatenation never exists
                    GemmP q = gp(h, (long)Tn * D, off(wro, (size_t)D, e), 2 * D, vcls, D, nb, D, D);
                    q.bias = W_(rs + "readout_projects." + is + ".0.bias"); q.bias_mode = BIAS_N;
                    car_launch_gemm(mode, AMODE_PLAIN, &q, st);
                    for (int i = 0; i < nb; ++i) {
                        GemmP r = gp(off(h, ((size_t)i * Tn + 1) * D, e), D, wro, 2 * D, off(rot[0], (size_t)i * n * D, e), D, n, D, D);
                        r.bias = off(vcls, (size_t)i * D, e); r.bias_mode = BIAS_N; r.act = ACT_GELU_ERF;
                        car_launch_gemm(mode, AMODE_PLAIN, &r, st);
                    }
                }
                {   // 1x1 conv D -> Ci: the token matrix already is the NHWC map
                    GemmP q = gp(rot[0], D, W_(rs + "layers." + is + ".projection.weight"), D, rot[1], Ci, nb * n, Ci, D);
                    q.bias = W_(rs + "layers." + is + ".projection.bias"); q.bias_mode = BIAS_N;
                    car_launch_gemm(mode, AMODE_PLAIN, &q, st);
                }
                const void* fmap = rot[1];
                if (tap < 2) {   // ConvTranspose2d(k = stride): a GEMM with N = k*k*Ci (bias replicated per tap at load time) and a pixel-shuffle store
                    const int k = tap == 0 ? 4 : 2;
                    GemmP q = gp(rot[1], Ci, W_(rs + "layers." + is + ".resize.weight"), Ci, rot[0], (long)k * k * Ci, nb * n, k * k * Ci, Ci);
                    q.bias = W_(rs + "layers." + is + ".resize.bias"); q.bias_mode = BIAS_N;
                    car_launch_gemm(mode, AMODE_PLAIN, &q, st);
                    DPTCHK(c, car_launch_dpt_shuffle(mode, rot[0], rot[1], nb, g, k, Ci, st));
                } else if (tap == 3) {   // Conv2d(3x3, stride 2, pad 1)
                    if (conv(rot[1], g, Ci, 2, rs + "layers.3.resize", true, Ci, rot[0], 0, 0, nullptr, nullptr, nb)) return -1;
                    fmap = rot[0];
                }
                if (conv(fmap, lvl[tap], Ci, 1, "depth.neck.convs." + is, false, F, feat[tap], 0, 0, nullptr, nullptr, nb)) return -1;   // neck.convs[tap]: no bias
                ++tap;
            }
        }
        if (bb_only) continue;
        // ---- fusion stage, from the coarsest map to the finest.  RCU(x) = conv2(relu(conv1(relu(x)))) + x: conv1 reads through the ReLU and stores the
        // ReLU of its output (only conv2 reads it); conv2 adds x, and in residual_layer1 also the running state h.  The x2 up-sampling is commuted with
        // the 1x1 projection behind it (the same linear map on a quarter of the pixels; the bias survives because bilinear weights sum to 1).
        int hb = -1;                                  // rotating buffer that holds the running state
        for (int j = 0; j < 4; ++j) {
            const int s = lvl[3 - j];
            const std::string fl = "depth.neck.fusion_stage.layers." + std::to_string(j) + ".";
            const void* x = feat[3 - j];
            int ia, ib;
            if (j == 0) { ia = 0; ib = 1; hb = 2; }
            else {
                ia = (hb + 1) % 3; ib = (hb + 2) % 3;
                if (conv(x, s, F, 1, fl + "residual_layer1.convolution1", true, F, rot[ia], 1, 1, nullptr, nullptr, nb)) return -1;
                if (conv(rot[ia], s, F, 1, fl + "residual_layer1.convolution2", true, F, rot[ib], 0, 0, x, rot[hb], nb)) return -1;   // h + RCU1(x)
                x = rot[ib];
            }
            if (conv(x, s, F, 1, fl + "residual_layer2.convolution1", true, F, rot[ia], 1, 1, nullptr, nullptr, nb)) return -1;
            if (conv(rot[ia], s, F, 1, fl + "residual_layer2.convolution2", true, F, rot[hb], 0, 0, x, nullptr, nb)) return -1;          // RCU2(h)
            if (!up_first) {
                GemmP q = gp(rot[hb], F, W_(fl + "projection.weight"), F, rot[ia], F, nb * s * s, F, F);
                q.bias = W_(fl + "projection.bias"); q.bias_mode = BIAS_N;
                car_launch_gemm(mode, AMODE_PLAIN, &q, st);
                DPTCHK(c, car_launch_dpt_up2(mode, rot[ia], rot[ib], nb, s, s, F, st));      // ib is free by now
            } else {                                  // the reference's order, four times the projection's rows (A/B only)
                DPTCHK(c, car_launch_dpt_up2(mode, rot[hb], rot[ia], nb, s, s, F, st));
                GemmP q = gp(rot[ia], F, W_(fl + "projection.weight"), F, rot[ib], F, nb * 4 * s * s, F, F);
                q.bias = W_(fl + "projection.bias"); q.bias_mode = BIAS_N;
                car_launch_gemm(mode, AMODE_PLAIN, &q, st);
            }
            hb = ib;
        }
        // ---- head: conv3x3 F -> F/2, x2, conv3x3 F/2 -> 32 + ReLU with the 32 -> 1 projection + ReLU in its epilogue
        const int ia = (hb + 1) % 3, ib = (hb + 2) % 3, s8 = 8 * g;
        if (conv(rot[hb], s8, F, 1, "depth.head.head.0", true, F / 2, rot[ia], 0, 0, nullptr, nullptr, nb)) return -1;
        DPTCHK(c, car_launch_dpt_up2(mode, rot[ia], rot[ib], nb, s8, s8, F / 2, st));
        float* map = out ? out + (size_t)b0 * P : wmap; const long map_img = out ? (long)P : (long)(b_map / 4);
        {
            DptConvP p; memset(&p, 0, sizeof(p));
            p.in = rot[ib]; p.w = W_("depth.head.head.2.weight"); p.bias = (const float*)W_("depth.head.head.2.bias");
            p.proj = W_("depth.head.head.4.weight"); p.proj_bias = (const float*)W_("depth.head.head.4.bias"); p.map = map; p.map_img = map_img;
            if (!p.w || !p.bias || !p.proj || !p.proj_bias) FAIL(c, "car_depth: depth.head.head is not loaded");
            p.Hi = p.Wi = p.H = p.W = S; p.Cin = F / 2; p.N = 32; p.K = 9 * p.Cin; p.stride = 1; p.relu_out = 1; p.in_img = (long)P * p.Cin;
            DPTCHK(c, car_launch_dpt_conv(mode, &p, nb, st));
        }
        if (control_out) {
            DPTCHK(c, car_launch_dpt_max(map, map_img, mx, nb, (long)P, st));
            DPTCHK(c, car_launch_dpt_control(mode, map, map_img, mx, (char*)control_out + (size_t)b0 * 3 * P * e, nb, (long)P, st));
        }
    }
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}
