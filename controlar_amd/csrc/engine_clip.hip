// engine_clip.hip — the CLIP score (car_clip_configure / car_clip_encode_image / car_clip_encode_text / car_clip_score): compute_clip_score of
// evaluations/t2i/evaluation.py:129-176 with the model as HF transformers' CLIPModel evaluates it (modeling_clip.py).
// (one of the translation units behind include/controlar_hip.h; shared declarations: engine_internal.h)
//
// Chunk rule (fixed): both towers run in chunks of at most max(1, 16384 / Tn) sequences (images or captions) of Tn rows each — car_score's 16384 activation
// rows, where the wide linears have the tile count at which car_launch_gemm takes its LDS-DMA kernel; in the fp32 mode the count is halved until the chunk's
// score tensor fits 1 GiB.  Scratch is bounded, a call of any B works, and no kernel of a chunk lets a row depend on its chunk-mates (every GEMM kernel sums an
// output's k-blocks in order whatever M; LayerNorm, softmax and the fused attention work per row / per (sequence, head)), so a row encoded alone returns
// the bits of its slice of any batch.
#include "engine_internal.h"

enum { kClipRows = 16384 };
static int clip_chunk(const car_ctx* c, int B, int Tn, int nh) {
    int ch = kClipRows / Tn; if (ch < 1) ch = 1;
    if (!use_flash(c, 64)) while (ch > 1 && (size_t)ch * nh * Tn * Tn * 4 > ((size_t)1 << 30)) ch /= 2;
    return B < ch ? B : ch;
}
static const float kClipMean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, kClipStd[3] = {0.26862954f, 0.26130258f, 0.27577711f};

extern "C" int car_clip_configure(car_ctx* c, const car_clip_config* k) {
    if (!c || !k) { if (c) c->err = "car_clip_configure: null argument"; return -1; }
    if (k->vision_width <= 0 || k->vision_layers <= 0 || k->vision_heads <= 0 || k->vision_mlp <= 0 || k->image_size <= 0 || k->patch <= 0 || k->text_width <= 0 ||
        k->text_layers <= 0 || k->text_heads <= 0 || k->text_mlp <= 0 || k->vocab_size <= 0 || k->context_length <= 0 || k->proj_dim <= 0 || !(k->ln_eps > 0.f))
        FAIL(c, "car_clip_configure: non-positive field");
    if (k->vision_width != 64 * k->vision_heads || k->text_width != 64 * k->text_heads)
        FAIL(c, "car_clip_configure: heads must be 64 wide (vision %d / %d, text %d / %d): ViT-B/32, B/16 and L/14 are; ViT-g/14's 88 is out of scope",
             k->vision_width, k->vision_heads, k->text_width, k->text_heads);
    if (k->image_size % k->patch) FAIL(c, "car_clip_configure: image_size %d is no multiple of patch %d", k->image_size, k->patch);
    if (k->vision_mlp % 32 || k->text_mlp % 32) FAIL(c, "car_clip_configure: the MLP widths must be multiples of 32 (the K step of the GEMMs), got %d and %d", k->vision_mlp, k->text_mlp);
    if (k->proj_dim % 8) FAIL(c, "car_clip_configure: proj_dim must be a multiple of 8, got %d", k->proj_dim);
    if (k->context_length > 128) FAIL(c, "car_clip_configure: context_length %d exceeds 128", k->context_length);
    if (k->image_size > 4096) FAIL(c, "car_clip_configure: image_size %d exceeds 4096", k->image_size);
    c->clip = *k; c->has_clip = true;
    return 0;
}

static void clip_layer_names(const std::string& p, std::vector<std::string>& v) {
    for (const char* s : {"self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2", "layer_norm1", "layer_norm2"}) {
        v.push_back(p + s + ".weight"); v.push_back(p + s + ".bias");
    }
}
void clip_tensor_names(const car_ctx* c, std::vector<std::string>& v) {
    const car_clip_config& k = c->clip;
    for (const char* s : {"clip.text_model.embeddings.token_embedding.weight", "clip.text_model.embeddings.position_embedding.weight", "clip.text_model.final_layer_norm.weight",
                          "clip.text_model.final_layer_norm.bias", "clip.vision_model.embeddings.class_embedding", "clip.vision_model.embeddings.patch_embedding.weight",
                          "clip.vision_model.embeddings.position_embedding.weight", "clip.vision_model.pre_layrnorm.weight", "clip.vision_model.pre_layrnorm.bias",
                          "clip.vision_model.post_layernorm.weight", "clip.vision_model.post_layernorm.bias", "clip.visual_projection.weight", "clip.text_projection.weight"}) v.push_back(s);
    for (int i = 0; i < k.text_layers; ++i) clip_layer_names("clip.text_model.encoder.layers." + std::to_string(i) + ".", v);
    for (int i = 0; i < k.vision_layers; ++i) clip_layer_names("clip.vision_model.encoder.layers." + std::to_string(i) + ".", v);
}

int clip_load_tensor(car_ctx* c, const LoadedTensor& ld) {
    const std::string& name = ld.name; const char* cname = ld.cname;
    const std::vector<int64_t>& shp = ld.shape; const int ndim = ld.ndim();
    if (!c->has_clip) FAIL(c, "%s: call car_clip_configure before loading clip.* tensors", cname);
    if (name == "clip.logit_scale" || ends_with(name, ".position_ids")) return 0;
    const car_clip_config& k = c->clip;
    const bool vis = starts_with(name, "clip.vision_model.");
    if (!vis && !starts_with(name, "clip.text_model.") && name != "clip.visual_projection.weight" && name != "clip.text_projection.weight")
        FAIL(c, "%s: not a tensor of CLIPModel", cname);
    const int D = vis ? k.vision_width : k.text_width, F = vis ? k.vision_mlp : k.text_mlp, g = k.image_size / k.patch;
    if (name == "clip.vision_model.embeddings.patch_embedding.weight") {
        // [D, 3, patch, patch] -> [D, Kp]: the columns (c, py, px) of clip_pixels_to_patches, zero padded to the GEMMs' K step
        const int K = 3 * k.patch * k.patch, Kp = (int)rup(K, 32);
        if (ndim != 4 || shp[0] != D || shp[1] != 3 || shp[2] != k.patch || shp[3] != k.patch) FAIL(c, "%s: expected [%d,3,%d,%d]", cname, D, k.patch, k.patch);
        return upload(c, name, pad_rows(ld.h.data(), D, K, Kp), {D, Kp});
    }
    int64_t e0 = -1, e1 = -1;
    if (name == "clip.visual_projection.weight") { e0 = k.proj_dim; e1 = k.vision_width; }
    else if (name == "clip.text_projection.weight") { e0 = k.proj_dim; e1 = k.text_width; }
    else if (name == "clip.vision_model.embeddings.class_embedding") { e0 = D; }
    else if (name == "clip.vision_model.embeddings.position_embedding.weight") { e0 = g * g + 1; e1 = D; }
    else if (name == "clip.text_model.embeddings.token_embedding.weight") { e0 = k.vocab_size; e1 = D; }
    else if (name == "clip.text_model.embeddings.position_embedding.weight") { e0 = k.context_length; e1 = D; }
    else if (ends_with(name, "_proj.weight")) { e0 = D; e1 = D; }
    else if (ends_with(name, "mlp.fc1.weight")) { e0 = F; e1 = D; }
    else if (ends_with(name, "mlp.fc2.weight")) { e0 = D; e1 = F; }
    else if (ends_with(name, "mlp.fc1.bias")) { e0 = F; }
    else if (ends_with(name, "_proj.bias") || ends_with(name, "mlp.fc2.bias") || ends_with(name, "norm1.weight") || ends_with(name, "norm1.bias") ||
             ends_with(name, "norm2.weight") || ends_with(name, "norm2.bias") || ends_with(name, "layrnorm.weight") || ends_with(name, "layrnorm.bias") ||
             ends_with(name, "layernorm.weight") || ends_with(name, "layernorm.bias") || ends_with(name, "layer_norm.weight") || ends_with(name, "layer_norm.bias")) { e0 = D; }
    else FAIL(c, "%s: not a tensor of CLIPModel", cname);
    if (shp.empty() || shp[0] != e0 || (e1 >= 0 && (ndim != 2 || shp[1] != e1)) || (e1 < 0 && ndim != 1)) FAIL(c, "%s: unexpected shape", cname);
    return upload(c, name, ld.h, shp);
}

static int clip_ready(car_ctx* c, const char* who) {
    if (!c->has_clip) FAIL(c, "%s: call car_clip_configure first", who);
    if (!c->finalized || !Wp(c, "clip.text_projection.weight") || !Wp(c, "clip.visual_projection.weight")) FAIL(c, "%s: CLIP weights not loaded / finalised", who);
    return 0;
}

// The pre-norm layers of one tower over `nb` sequences of Tn rows in h (modeling_clip.py CLIPEncoderLayer): h += out_proj(attn(LN1 h)); h += fc2(quick_gelu(fc1(LN2 h))).
// causal: the text tower's mask (key j <= query i, no padding mask).  Scratch: ws[2] xn, ws[3] q|k|v, ws[WS_ATTN_S], ws[WS_ATTN_P], ws[WS_ATTN_VT], ws[7] mid, ws[8] ctx.
static int clip_layers(car_ctx* c, const std::string& tower, int layers, void* h, int nb, int Tn, int D, int nh, int F, bool causal, hipStream_t st) {
    const int mode = c->mode; const size_t e = c->esz; const float eps = c->clip.ln_eps;
    const long rows = (long)nb * Tn;
    void *xn = c->ws[2].p, *qkv = c->ws[3].p, *mid = c->ws[7].p, *ctx = c->ws[8].p;
    void* qp = qkv; void* kp = off(qkv, (size_t)rows * D, e); void* vp = off(qkv, (size_t)2 * rows * D, e);
    // ctx = softmax(Q K^T * head_dim^-0.5) V, head_dim = 64 (eager_attention_forward); the text tower's causal form takes an all-ones pad mask
    const AttnCall at = {qp, kp, vp, D, ctx, nb, Tn, nh, 64, 0.125f, causal ? ATTN_CAUSAL : ATTN_NONE, causal ? (const unsigned char*)c->clip_ones.p : nullptr, nullptr, 0};
    auto lin = [&](const void* x, int K, const std::string& w, void* y, int N, int act, const void* R) {
        GemmP q = gp(x, K, Wp(c, w + ".weight"), K, y, N, (int)rows, N, K);
        q.bias = Wp(c, w + ".bias"); q.bias_mode = BIAS_N; q.act = act; q.R = R; q.ldr = N;
        return car_launch_gemm(mode, AMODE_PLAIN, &q, st);
    };
    for (int l = 0; l < layers; ++l) {
        const std::string L = tower + "encoder.layers." + std::to_string(l) + ".";
        car_launch_layernorm(mode, h, Wp(c, L + "layer_norm1.weight"), Wp(c, L + "layer_norm1.bias"), xn, rows, D, eps, st);
        if (lin(xn, D, L + "self_attn.q_proj", qp, D, ACT_NONE, nullptr) || lin(xn, D, L + "self_attn.k_proj", kp, D, ACT_NONE, nullptr) ||
            lin(xn, D, L + "self_attn.v_proj", vp, D, ACT_NONE, nullptr)) FAIL(c, "CLIP: a projection GEMM was refused (width %d)", D);
        if (attn_run(c, at, st)) FAIL(c, "CLIP: the fused attention kernel refused %d rows x %d heads", Tn, nh);
        if (lin(ctx, D, L + "self_attn.out_proj", h, D, ACT_NONE, h)) FAIL(c, "CLIP: the out_proj GEMM was refused (width %d)", D);
        car_launch_layernorm(mode, h, Wp(c, L + "layer_norm2.weight"), Wp(c, L + "layer_norm2.bias"), xn, rows, D, eps, st);
        if (lin(xn, D, L + "mlp.fc1", mid, F, ACT_QUICK_GELU, nullptr) || lin(mid, F, L + "mlp.fc2", h, D, ACT_NONE, h)) FAIL(c, "CLIP: an MLP GEMM was refused (widths %d, %d)", D, F);
    }
    return 0;
}

// scratch of one chunk of `CH` sequences of Tn rows (the buffers clip_layers names, plus ws[0] patches / pooled rows and ws[1] h)
static int clip_scratch(car_ctx* c, int CH, int Tn, int D, int nh, int F, size_t ws0_elems) {
    const size_t e = c->esz; const long rows = (long)CH * Tn; const AttnBytes ab = attn_bytes(c, CH, Tn, nh, 64);
    NEED(c, c->ws[0], ws0_elems * e);
    NEED(c, c->ws[1], (size_t)rows * D * e);
    NEED(c, c->ws[2], (size_t)rows * D * e);
    NEED(c, c->ws[3], (size_t)rows * 3 * D * e);
    if (ab.S) NEED(c, c->ws[WS_ATTN_S], ab.S);
    if (ab.P) NEED(c, c->ws[WS_ATTN_P], ab.P);
    NEED(c, c->ws[WS_ATTN_VT], ab.Vt);
    NEED(c, c->ws[7], (size_t)rows * F * e);
    NEED(c, c->ws[8], (size_t)rows * D * e);
    return 0;
}

// rows [nb, D] in `pooled` -> LayerNorm -> projection (no bias) -> fp32 [nb, proj]
static int clip_head(car_ctx* c, void* pooled, void* normed, const std::string& ln, const char* proj, int nb, int D, float* out, hipStream_t st) {
    car_launch_layernorm(c->mode, pooled, Wp(c, ln + ".weight"), Wp(c, ln + ".bias"), normed, nb, D, c->clip.ln_eps, st);
    GemmP q = gp(normed, D, Wp(c, proj), D, out, c->clip.proj_dim, nb, c->clip.proj_dim, D);
    q.out_f32 = 1;
    if (car_launch_gemm(c->mode, AMODE_PLAIN, &q, st)) FAIL(c, "CLIP: the projection GEMM was refused (width %d)", D);
    return 0;
}

// the ToTensor / Normalize(0.5, 0.5) / tensor2pil round trip of one byte (evaluation.py:63-73,117-126), in fp32 with torch's operation order
#pragma clang fp contract(off)
static unsigned char clip_requant_byte(int u) {
    volatile float x = (float)u / 255.0f;        // ToTensor
    x = (x - 0.5f) / 0.5f;                       // Normalize(0.5, 0.5)
    x = (x + 1.0f) * 127.5f;                     // tensor2pil
    x = x < 0.0f ? 0.0f : (x > 255.0f ? 255.0f : x);
    return (unsigned char)(int)x;                // .to(torch.uint8) truncates
}
extern "C" int car_debug_clip_requant_table(unsigned char* out) {      // host-only helper (tests)
    if (!out) return -1;
    for (int u = 0; u < 256; ++u) out[u] = clip_requant_byte(u);
    return 0;
}

extern "C" int car_clip_encode_image(car_ctx* c, const uint8_t* img, int32_t B, int32_t H, int32_t W, int32_t requant, float* out_emb, float* pixel_values_out, void* stream_) {
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!c->has_clip) FAIL(c, "car_clip_encode_image: call car_clip_configure first");
    if (out_emb && clip_ready(c, "car_clip_encode_image")) return -1;
    if (!img) FAIL(c, "car_clip_encode_image: the image pointer is NULL");
    if (!out_emb && !pixel_values_out) FAIL(c, "car_clip_encode_image: no output requested (out_emb and pixel_values_out are both NULL)");
    if (B <= 0 || H <= 0 || W <= 0 || H > 65536 || W > 65536) FAIL(c, "car_clip_encode_image: sizes must be positive and at most 65536 (got B %d, %d x %d)", B, H, W);
    const car_clip_config& k = c->clip;
    const int n = k.image_size, p = k.patch, g = n / p, np = g * g, Tn = np + 1, D = k.vision_width, nh = k.vision_heads, F = k.vision_mlp;
    const int Kp = (int)rup((size_t)3 * p * p, 32);
    // torchvision's Resize(n): the short side becomes n, the long side int(n * long / short); CenterCrop(n): offset round((side - n) / 2), half to even
    const int Hr = H <= W ? n : (int)((long long)n * H / W), Wr = H <= W ? (int)((long long)n * W / H) : n;
    auto crop0 = [&](int side) { const int d = side - n, q = d / 2; return (d & 1) ? q + (q & 1) : q; };
    const int top = crop0(Hr), left = crop0(Wr);
    const int mode = c->mode; const size_t e = c->esz;
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    const int CH = clip_chunk(c, B, Tn, nh);
    const bool resize = Hr != H || Wr != W;
    const size_t src_bytes = rup((size_t)H * W * 3 * CH, 256), rs_bytes = rup((size_t)Hr * Wr * 3 * CH, 256);
    NEED(c, c->clip_u8, 256 + (requant ? src_bytes : 0) + (resize ? rs_bytes : 0));
    unsigned char* rq = (unsigned char*)c->clip_u8.p; unsigned char* rs = rq + (requant ? src_bytes : 0);
    unsigned char tab[256];
    for (int u = 0; u < 256; ++u) tab[u] = clip_requant_byte(u);
    if (clip_scratch(c, CH, Tn, D, nh, F, std::max((size_t)CH * np * Kp, (size_t)2 * CH * D))) return -1;
    fence_in(c, caller);
    const std::string V = "clip.vision_model.";
    for (int b0 = 0; b0 < B; b0 += CH) {
        const int nb = (B - b0) < CH ? (B - b0) : CH;
        const unsigned char* src = img + (size_t)b0 * H * W * 3;
        if (requant) { car_launch_clip_requant(src, rq, tab, (long)nb * H * W * 3, st); src = rq; }
        if (resize) {
            if (car_resize(c, src, nb, H, W, 3, Hr, Wr, CAR_FILTER_BICUBIC, nullptr, rs, nullptr, nullptr, 0, st)) return -1;
            src = rs;
        }
        void *patches = c->ws[0].p, *h = c->ws[1].p, *y = c->ws[2].p;
        ClipPatchP pp; memset(&pp, 0, sizeof(pp));
        pp.src = src; pp.patches = patches; pp.pixel_values = pixel_values_out ? pixel_values_out + (size_t)b0 * 3 * n * n : nullptr;
        pp.B = nb; pp.Hr = Hr; pp.Wr = Wr; pp.top = top; pp.left = left; pp.n_px = n; pp.patch = p; pp.g = g; pp.Kp = Kp;
        for (int i = 0; i < 3; ++i) { pp.mean[i] = kClipMean[i]; pp.std[i] = kClipStd[i]; }
        car_launch_clip_pixels_to_patches(mode, &pp, st);
        if (!out_emb) continue;
        {   // the bias-free patch convolution as a GEMM -> y (the token buffer); class token and positions -> xn; pre_layrnorm -> h
            GemmP q = gp(patches, Kp, Wp(c, V + "embeddings.patch_embedding.weight"), Kp, y, D, nb * np, D, Kp);
            if (car_launch_gemm(mode, AMODE_PLAIN, &q, st)) FAIL(c, "car_clip_encode_image: the patch GEMM was refused");
        }
        void* asm_ = c->ws[8].p;
        car_launch_vit_assemble(mode, y, Wp(c, V + "embeddings.class_embedding"), Wp(c, V + "embeddings.position_embedding.weight"), asm_, nb, np, D, st);
        car_launch_layernorm(mode, asm_, Wp(c, V + "pre_layrnorm.weight"), Wp(c, V + "pre_layrnorm.bias"), h, (long)nb * Tn, D, k.ln_eps, st);
        if (clip_layers(c, V, k.vision_layers, h, nb, Tn, D, nh, F, false, st)) return -1;
        void* pooled = c->ws[0].p; void* normed = off(pooled, (size_t)CH * D, e);
        car_launch_clip_pool(mode, h, nullptr, pooled, nb, Tn, D, 0, st);
        if (clip_head(c, pooled, normed, V + "post_layernorm", "clip.visual_projection.weight", nb, D, out_emb + (size_t)b0 * k.proj_dim, st)) return -1;
    }
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int car_clip_encode_text(car_ctx* c, const int64_t* ids, int32_t B, int32_t T, float* out_emb, void* stream_) {
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (clip_ready(c, "car_clip_encode_text")) return -1;
    if (!ids || !out_emb || B <= 0 || T <= 0) FAIL(c, "car_clip_encode_text: bad arguments");
    const car_clip_config& k = c->clip;
    if (T > k.context_length) FAIL(c, "car_clip_encode_text: %d tokens exceed the context length %d", T, k.context_length);
    const int D = k.text_width, nh = k.text_heads, F = k.text_mlp;
    const int mode = c->mode; const size_t e = c->esz;
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    if (ensure_host_flags(c)) return -1;
    const int CH = clip_chunk(c, B, T, nh);
    if (clip_scratch(c, CH, T, D, nh, F, (size_t)2 * CH * D)) return -1;
    NEED(c, c->clip_ones, (size_t)CH * T);
    fence_in(c, caller);
    HIPCHK(c, hipMemsetAsync(c->clip_ones.p, 1, (size_t)CH * T, st));
    const std::string Tm = "clip.text_model.";
    for (int b0 = 0; b0 < B; b0 += CH) {
        const int nb = (B - b0) < CH ? (B - b0) : CH;
        const long long* idc = (const long long*)ids + (size_t)b0 * T;
        void* h = c->ws[1].p;
        car_launch_clip_text_embed(mode, idc, Wp(c, Tm + "embeddings.token_embedding.weight"), Wp(c, Tm + "embeddings.position_embedding.weight"), h, nb, T, D,
                                   k.vocab_size, c->host_flags + 3, st);
        if (clip_layers(c, Tm, k.text_layers, h, nb, T, D, nh, F, true, st)) return -1;
        // final_layer_norm is per row: pooling first leaves B rows to normalise and project
        void* pooled = c->ws[0].p; void* normed = off(pooled, (size_t)CH * D, e);
        car_launch_clip_pool(mode, h, idc, pooled, nb, T, D, k.vocab_size, st);
        if (clip_head(c, pooled, normed, Tm + "final_layer_norm", "clip.text_projection.weight", nb, D, out_emb + (size_t)b0 * k.proj_dim, st)) return -1;
    }
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int car_clip_score(car_ctx* c, const float* img_emb, const float* txt_emb, int32_t B, int32_t n_mean, float* out_scores, double* out_mean, void* stream_) {
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!c->has_clip) FAIL(c, "car_clip_score: call car_clip_configure first (the embedding width is its proj_dim)");
    if (!img_emb || !txt_emb || !out_scores || B <= 0) FAIL(c, "car_clip_score: bad arguments");
    if (out_mean && (n_mean <= 0 || n_mean > B)) FAIL(c, "car_clip_score: n_mean must lie in [1, B = %d], got %d", B, n_mean);
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    car_launch_clip_cosine(img_emb, txt_emb, B, c->clip.proj_dim, 1e-8f, out_scores, st);
    if (out_mean) car_launch_clip_mean(out_scores, n_mean, out_mean, st);
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}
