// engine_weights.hip — car_load_tensor (reference state-dict names -> packed device images: the dispatcher, the decode linears, the GPT and its ViT adapter;
// every other family packs next to its runner, layouts in weight_pack.h), car_finalize_weights, the packed-image cache
// (one of the translation units behind include/controlar_hip.h; shared declarations: engine_internal.h)
#include "engine_internal.h"

// ------------------------------------------------------------------------------------- weights

// upload a host fp32 array as element type T (or as fp32 when force_f32)
int upload(car_ctx* c, const std::string& name, const std::vector<float>& h, const std::vector<int64_t>& shape, bool force_f32) {
    Wt t; t.shape = shape; t.numel = (int64_t)h.size();
    const bool f32 = force_f32 || c->mode == CAR_F32;
    const size_t bytes = h.size() * (f32 ? 4 : 2);
    t.bytes = bytes;
    HIPCHK(c, hipMalloc(&t.p, bytes ? bytes : 4));
    if (f32) { HIPCHK(c, hipMemcpy(t.p, h.data(), bytes, hipMemcpyHostToDevice)); }
    else {
        std::vector<bf16_t> hb(h.size());
        for (size_t i = 0; i < h.size(); ++i) hb[i] = f2bf(h[i]);
        HIPCHK(c, hipMemcpy(t.p, hb.data(), bytes, hipMemcpyHostToDevice));
    }
    auto it = c->w.find(name);
    if (it != c->w.end() && it->second.p) (void)hipFree(it->second.p);
    c->w[name] = t;
    // a re-loaded tensor invalidates its exact-mode fragment image (rebuilt by car_finalize_weights); a re-loaded RMSNorm weight invalidates the image of the
    // linear it is folded into (decode_f32.hip NX: wqkv <- attention_norm, w1|w3 <- ffn_norm, output <- norm)
    std::vector<std::string> stale = {name + "#pk32"};
    auto dep = [&](const char* sfx, const char* lin) { const size_t n = strlen(sfx); if (name.size() >= n && name.compare(name.size() - n, n, sfx) == 0) stale.push_back(name.substr(0, name.size() - n) + lin + "#pk32"); };
    dep("attention_norm.weight", "attention.wqkv.weight"); dep("ffn_norm.weight", "feed_forward.w13.weight");
    if (name == "norm.weight") stale.push_back("output.weight#pk32");
    for (auto& sname : stale) { auto pk = c->w.find(sname); if (pk != c->w.end()) { if (pk->second.p) (void)hipFree(pk->second.p); c->w.erase(pk); } }
    return 0;
}

// fp32 -> OCP e4m3fn (bias 7, max 448, no inf), round-to-nearest-even, saturating
static unsigned char f32_to_e4m3(float f) {
    if (f != f) return 0x7f;
    const unsigned char sign = std::signbit(f) ? 0x80 : 0;
    float a = std::fabs(f);
    if (a >= 464.0f) return sign | 0x7e;                       // beyond the midpoint above 448 (and inf): saturate
    if (a < 0.015625f) {                                        // below 2^-6: subnormal grid of 2^-9
        const int q = (int)std::nearbyint(a * 512.0f);
        return sign | (unsigned char)(q >= 8 ? 0x08 : q);
    }
    int e; const float m = std::frexp(a, &e);                   // a = m * 2^e, m in [0.5, 1)
    int ee = e - 1; float mm = m * 2.0f;                        // a = mm * 2^ee, mm in [1, 2)
    int mant = (int)std::nearbyint((mm - 1.0f) * 8.0f);
    if (mant == 8) { mant = 0; ++ee; }
    if (ee > 8 || (ee == 8 && mant > 6)) return sign | 0x7e;
    return sign | (unsigned char)(((ee + 7) << 3) | mant);
}
static float e4m3_to_f32(unsigned char v) {
    const int e = (v >> 3) & 15, m = v & 7; const float s = (v & 0x80) ? -1.f : 1.f;
    if (e == 15 && m == 7) return NAN;
    return s * (e == 0 ? (float)m * 0.001953125f : std::ldexp(1.0f + (float)m / 8.0f, e - 7));
}
extern "C" int car_debug_f32_to_e4m3(const float* in, unsigned char* out, int64_t n) {      // host-only helper (tests)
    if (!in || !out) return -1;
    for (int64_t i = 0; i < n; ++i) out[i] = f32_to_e4m3(in[i]);
    return 0;
}

// dec_linear weight image: [N/16][K/32] chunks of 64 lanes x 8 bf16 (lane l: row l&15, k (l>>4)*8..+8) — decode.hip
static void pack_decode_bf16(const float* h, int N, int K, bf16_t* pk) {
    const int nkb = K / 32;
    for (int rb = 0; rb < N / 16; ++rb) for (int kb = 0; kb < nkb; ++kb) for (int l = 0; l < 64; ++l) {
        const float* src = &h[(size_t)(rb * 16 + (l & 15)) * K + kb * 32 + (l >> 4) * 8];
        bf16_t* dst = &pk[(((size_t)rb * nkb + kb) * 64 + l) * 8];
        for (int e = 0; e < 8; ++e) dst[e] = f2bf(src[e]);
    }
}
extern "C" int car_debug_pack_decode_weight(const float* w, int32_t N, int32_t K, uint16_t* out) {      // host-only helper (tests)
    if (!w || !out || N <= 0 || K <= 0 || N % 16 || K % 32) return -1;
    pack_decode_bf16(w, N, K, out);
    return 0;
}
// ---- device-side packing of one decode linear (pack.hip).  `name` is the row-major image ([Ntot, K] bf16, the prefill operand:
// for w1 / w3 the 16-row interleaved "w13" image); `src` is the checkpoint tensor [Nsrc, K] in `dtype` (host or device).
// bf16 weights: name#pk = MFMA-fragment image.  fp8 weights: name#pk8 = e4m3 image, name#sc = fp32 row scales, and the
// row-major image holds the DEQUANTISED values so that prefill and decode see one set of effective weights.
int ensure_w(car_ctx* c, const std::string& name, size_t bytes, const std::vector<int64_t>& shape, int64_t numel) {
    auto it = c->w.find(name);
    if (it != c->w.end() && it->second.p && it->second.bytes == bytes) return 0;
    if (it != c->w.end() && it->second.p) (void)hipFree(it->second.p);
    Wt t; t.shape = shape; t.numel = numel; t.bytes = bytes;
    HIPCHK(c, hipMalloc(&t.p, bytes ? bytes : 4));
    c->w[name] = t;
    return 0;
}
static int dev_linear(car_ctx* c, const std::string& name, const void* src, bool on_dev, int dtype, int Nsrc, int K, int ileave, int Ntot) {
    const bool f8 = c->cfg.decode_weight_fp8 != 0;
    if (Ntot % 16 || K % (f8 ? 64 : 32)) FAIL(c, "%s: decode packing needs N%%16==0 and K%%%d==0 (got %d x %d)", name.c_str(), f8 ? 64 : 32, Ntot, K);
    const size_t eb = dtype == CAR_DT_F32 ? 4 : 2;
    void* stage = nullptr;
    if (!on_dev) {
        HIPCHK(c, hipMalloc(&stage, (size_t)Nsrc * K * eb));
        HIPCHK(c, hipMemcpy(stage, src, (size_t)Nsrc * K * eb, hipMemcpyHostToDevice));
        src = stage;
    }
    const int dt = dtype == CAR_DT_F32 ? 0 : 1;
    int rc = ensure_w(c, name, (size_t)Ntot * K * 2, {Ntot, K}, (int64_t)Ntot * K);
    bool complete = ileave == 0;
    if (!rc && ileave) { int& seen = c->w13_seen[name]; seen |= ileave; complete = seen == 3; }
    if (!rc && !f8) {
        car_launch_rows_to_bf16(src, dt, c->w[name].p, Nsrc, K, ileave, 0);
        if (complete) {
            rc = ensure_w(c, name + "#pk", (size_t)Ntot * K * 2, {Ntot, K}, (int64_t)Ntot * K);
            if (!rc) car_launch_pack_frag_bf16(c->w[name].p, c->w[name + "#pk"].p, Ntot, K, 0);
        }
    } else if (!rc) {
        rc = ensure_w(c, name + "#sc", (size_t)Ntot * 4, {Ntot}, Ntot);
        if (!rc) rc = ensure_w(c, name + "#pk8", (size_t)Ntot * K, {Ntot, K}, (int64_t)Ntot * K);
        if (!rc) {
            car_launch_row_amax_scale(src, dt, (float*)c->w[name + "#sc"].p, Nsrc, K, ileave, 0);
            car_launch_quant_pack_fp8(src, dt, (const float*)c->w[name + "#sc"].p, c->w[name].p, c->w[name + "#pk8"].p, Nsrc, K, ileave, 0);
        }
    }
    if (!rc) { hipError_t e2 = hipStreamSynchronize(0); if (e2 == hipSuccess) e2 = hipGetLastError(); if (e2 != hipSuccess) { c->err = std::string("device packing failed: ") + hipGetErrorString(e2); rc = -1; } }
    if (stage) (void)hipFree(stage);
    return rc;
}

static void replace_all(std::string& s, const std::string& a, const std::string& b) {
    size_t p = 0; while ((p = s.find(a, p)) != std::string::npos) { s.replace(p, a.size(), b); p += b.size(); }
}
// HF ViTModel key names (transformers 5.x "layers.N.attention.q_proj", and the 4.x checkpoint names
// "encoder.layer.N.attention.attention.query / intermediate.dense / output.dense") -> the encoder's canonical names
static std::string canon_name(const std::string& in) {
    if (in.compare(0, 14, "adapter.model.") != 0) return in;
    std::string s = in;
    replace_all(s, "adapter.model.layers.", "adapter.model.encoder.layer.");
    replace_all(s, ".attention.q_proj.", ".attention.attention.query.");
    replace_all(s, ".attention.k_proj.", ".attention.attention.key.");
    replace_all(s, ".attention.v_proj.", ".attention.attention.value.");
    replace_all(s, ".attention.o_proj.", ".attention.output.dense.");
    replace_all(s, ".layernorm_before.", ".norm1.");
    replace_all(s, ".layernorm_after.", ".norm2.");
    replace_all(s, ".intermediate.dense.", ".mlp.fc1.");
    if (s.find(".attention.output.dense.") == std::string::npos) replace_all(s, ".output.dense.", ".mlp.fc2.");
    return s;
}

// the halves of a gated feed-forward pair (w1 | w3, wi_0 | wi_1) arrive as two tensors: see engine_internal.h
int load_interleaved_half(car_ctx* c, const LoadedTensor& t, const char* sfx_a, const char* sfx_b, const char* sfx_joint, int rows, int cols) {
    const bool is_a = ends_with(t.name, sfx_a);
    const std::string base = t.name.substr(0, t.name.size() - strlen(sfx_a));
    const std::string other = base + (is_a ? sfx_b : sfx_a);
    auto it = c->host_keep.find(other);
    if (it == c->host_keep.end()) { c->host_keep[t.name] = std::move(t.h); return 0; }
    const std::vector<float>& a = is_a ? t.h : it->second; const std::vector<float>& b = is_a ? it->second : t.h;
    int rc = upload(c, base + sfx_joint, interleave16(a.data(), b.data(), rows, cols), {2 * (int64_t)rows, cols});
    c->host_keep.erase(other);
    return rc;
}

// the GPT and its ViT adapter: everything that belongs to no other family
int gpt_load_tensor(car_ctx* c, const LoadedTensor& t) {
    const car_config& g = c->cfg;
    if (ends_with(t.name, "feed_forward.w1.weight") || ends_with(t.name, "feed_forward.w3.weight")) {
        // w1 | w3 interleaved in blocks of 16 rows so the GEMM epilogue sees (a, c) pairs (gemm.hip SWIGLU); exact mode only (fast mode: dev_linear)
        if (t.ndim() != 2 || t.shape[0] != g.ffn_hidden || t.shape[1] != g.dim) FAIL(c, "%s: expected [%d,%d]", t.cname, g.ffn_hidden, g.dim);
        return load_interleaved_half(c, t, "w1.weight", "w3.weight", "w13.weight", g.ffn_hidden, g.dim);
    }
    if (t.name == "adapter.model.embeddings.position_embeddings") { c->host_keep[t.name] = t.h; return 0; }   // interpolated per resolution
    if (t.name == "adapter.model.embeddings.patch_embeddings.projection.weight") {
        // [D,3,p,p] -> [D, Kpad] zero padded to a multiple of 32
        const int K = 3 * g.vit_patch * g.vit_patch, Kp = (int)rup(K, 32);
        if (t.n != (int64_t)g.vit_hidden * K) FAIL(c, "%s: bad shape", t.cname);
        return upload(c, t.name, pad_rows(t.h.data(), g.vit_hidden, K, Kp), {g.vit_hidden, Kp});
    }
    return upload(c, t.name, t.h, t.shape);
}

static std::vector<std::string> decode_linear_names(const car_config& g) {
    std::vector<std::string> lin = {"output.weight"};
    for (int i = 0; i < g.n_layer; ++i) {
        const std::string p = "layers." + std::to_string(i) + ".";
        for (const char* s : {"attention.wqkv.weight", "attention.wo.weight", "feed_forward.w13.weight", "feed_forward.w2.weight"}) lin.push_back(p + s);
    }
    return lin;
}

void gpt_tensor_names(const car_ctx* c, std::vector<std::string>& req) {
    const car_config& g = c->cfg;
    for (const char* s : {"tok_embeddings.weight", "adapter_mlp.fc1.weight", "adapter_mlp.fc2.weight", "condition_mlp.cap_proj.fc1.weight", "condition_mlp.cap_proj.fc2.weight",
                          "norm.weight", "output.weight"}) req.push_back(s);
    if (g.model_type == 1) req.push_back("cls_embedding.embedding_table.weight");
    else for (const char* s : {"cls_embedding.cap_proj.fc1.weight", "cls_embedding.cap_proj.fc2.weight", "cls_embedding.uncond_embedding"}) req.push_back(s);
    for (int k = 0; k < 3; ++k) { req.push_back("condition_layers." + std::to_string(k) + ".fc1.weight"); req.push_back("condition_layers." + std::to_string(k) + ".fc2.weight"); }
    for (int i = 0; i < g.n_layer; ++i) {
        const std::string p = "layers." + std::to_string(i) + ".";
        for (const char* s : {"attention.wqkv.weight", "attention.wo.weight", "feed_forward.w13.weight", "feed_forward.w2.weight", "attention_norm.weight", "ffn_norm.weight"}) req.push_back(p + s);
    }
    const std::string a = "adapter.model.";
    for (const char* s : {"embeddings.cls_token", "embeddings.patch_embeddings.projection.weight", "embeddings.patch_embeddings.projection.bias", "layernorm.weight", "layernorm.bias"}) req.push_back(a + s);
    for (int i = 0; i < g.vit_layers; ++i) {
        const std::string p = a + "encoder.layer." + std::to_string(i) + ".";
        for (const char* s : {"norm1.weight", "norm1.bias", "attention.attention.query.weight", "attention.attention.query.bias", "attention.attention.key.weight",
                              "attention.attention.key.bias", "attention.attention.value.weight", "attention.attention.value.bias", "attention.output.dense.weight",
                              "attention.output.dense.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
                              "mlp.fc2.bias"}) req.push_back(p + s);
        if (g.vit_variant == 0) { req.push_back(p + "layer_scale1.lambda1"); req.push_back(p + "layer_scale2.lambda1"); }
    }
}

static bool pointer_on_device(const void* ptr) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ptr) == hipSuccess) return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
    (void)hipGetLastError();
    return false;
}

extern "C" int car_load_tensor(car_ctx* c, const char* cname, const void* ptr, const int64_t* shape, int32_t ndim, int32_t dtype) {
    if (!c || !cname || !ptr || (ndim > 0 && !shape)) { if (c) c->err = "car_load_tensor: null argument"; return -1; }
    if (dtype != CAR_DT_F32 && dtype != CAR_DT_BF16) FAIL(c, "car_load_tensor(%s): dtype must be F32 or BF16", cname);
    const std::string name = canon_name(cname);
    if (name.find("adapter.model.pooler.") == 0 || name == "condition_norm.weight") return 0;   // present in c2i checkpoints, unused on the path
    // reference tensors that the inference path never reads
    if (name == "condition_embeddings.weight" || name == "condition_mlp.uncond_embedding" || ends_with(name, "mask_token") ||
        name == "quantize.codebook_used") return 0;
    const std::vector<int64_t> shp(shape, shape + ndim);
    int64_t n = 1; for (auto s : shp) n *= s;
    const car_config& g = c->cfg;
    // fast mode: the five decode linears are packed on the device straight from the checkpoint tensor (pack.hip)
    const bool is13 = ends_with(name, "feed_forward.w1.weight") || ends_with(name, "feed_forward.w3.weight");
    const bool islin = ndim == 2 && (ends_with(name, "attention.wqkv.weight") || ends_with(name, "attention.wo.weight") ||
                                     ends_with(name, "feed_forward.w2.weight") || name == "output.weight");
    if (c->mode == CAR_BF16 && (is13 || islin)) {
        const bool on_dev = pointer_on_device(ptr);
        c->finalized = false;
        if (!is13) return dev_linear(c, name, ptr, on_dev, dtype, (int)shp[0], (int)shp[1], 0, (int)shp[0]);
        if (ndim != 2 || shp[0] != g.ffn_hidden || shp[1] != g.dim) FAIL(c, "%s: expected [%d,%d]", cname, g.ffn_hidden, g.dim);
        const std::string base = name.substr(0, name.size() - strlen("w1.weight"));
        return dev_linear(c, base + "w13.weight", ptr, on_dev, dtype, g.ffn_hidden, g.dim, ends_with(name, "w1.weight") ? 1 : 2, 2 * g.ffn_hidden);
    }
    // bring to host fp32
    std::vector<float> h((size_t)n);
    {
        const size_t eb = dtype == CAR_DT_F32 ? 4 : 2;
        std::vector<unsigned char> raw;
        const void* src = ptr;
        if (pointer_on_device(ptr)) { raw.resize((size_t)n * eb); HIPCHK(c, hipMemcpy(raw.data(), ptr, raw.size(), hipMemcpyDeviceToHost)); src = raw.data(); }
        if (dtype == CAR_DT_F32) memcpy(h.data(), src, (size_t)n * 4);
        else { const bf16_t* b = (const bf16_t*)src; for (int64_t i = 0; i < n; ++i) h[(size_t)i] = bf2f(b[i]); }
    }
    c->finalized = false;
    // every family packs its own tensors, next to its runner; what carries no family's prefix belongs to the GPT or its ViT adapter
    const LoadedTensor t{name, cname, shp, n, h};
    static const struct { const char* prefix; int (*load)(car_ctx*, const LoadedTensor&); } kFamilies[] = {
        {"lineart.", lineart_load_tensor}, {"hed.", hed_load_tensor}, {"depth.", depth_load_tensor}, {"t5.", t5_load_tensor}, {"clip.", clip_load_tensor}, {"lpips.", lpips_load_tensor},
        {"decoder.", vq_load_tensor}, {"encoder.", vq_load_tensor}, {"quant", vq_load_tensor}, {"post_quant_conv.", vq_load_tensor}};
    for (auto& f : kFamilies) if (starts_with(name, f.prefix)) return f.load(c, t);
    return gpt_load_tensor(c, t);
}

// a model family is optional as a group and must be complete if present: reports the names of `names` that `have` does not find (the first six of a call
// by name, all of them in the count).  present_if_any: the group counts as present once one of its names is there; otherwise the caller has decided that it is.
struct Missing { std::string names; int n = 0; void add(const std::string& r) { if (n < 6) names += r + " "; ++n; } };
template <class Have> static bool require_group(const std::vector<std::string>& names, Have have, bool present_if_any, Missing& miss) {
    bool present = !present_if_any;
    for (auto& r : names) if (have(r)) present = true;
    if (present) for (auto& r : names) if (!have(r)) miss.add(r);
    return present;
}

extern "C" int car_finalize_weights(car_ctx* c) {
    if (!c) return -1;
    const car_config& g = c->cfg;
    Missing miss;
    auto have = [&](const std::string& r) { return Wp(c, r) || c->host_keep.find(r) != c->host_keep.end(); };
    auto group = [&](void (*list)(const car_ctx*, std::vector<std::string>&), bool present_if_any) {
        std::vector<std::string> names;
        list(c, names);
        return require_group(names, have, present_if_any, miss);
    };
    // a context may serve only decode_code (VQ weights alone) — the reference keeps GPT and VQ as separate modules; the extractors and the caption encoder
    // may be held alone as well
    const bool have_la = group(lineart_tensor_names, true), have_hed = group(hed_tensor_names, true), have_dpt = c->has_dpt && group(depth_tensor_names, true);
    const bool have_clip = c->has_clip && group(clip_tensor_names, true), have_lpips = group(lpips_tensor_names, true);
    const bool have_t5 = c->has_t5 && Wp(c, "t5.shared.weight"), have_vq = Wp(c, "quantize.embedding.weight") != nullptr;
    const bool vq_only = (have_vq || have_t5 || have_la || have_hed || have_dpt || have_clip || have_lpips) && !Wp(c, "tok_embeddings.weight") && !Wp(c, "output.weight");
    c->has_gpt = !vq_only;
    auto host_table = [&](const char* r) { if (!have(r)) { miss.names += std::string(r) + " "; ++miss.n; } };      // named even behind six others
    if (have_t5) { group(t5_tensor_names, false); host_table("t5.encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"); }
    if (!vq_only) { group(gpt_tensor_names, false); host_table("adapter.model.embeddings.position_embeddings"); }
    if (have_vq) group(vq_tensor_names, false);
    const std::vector<std::string> lin = decode_linear_names(g);
    if (!vq_only && c->mode == CAR_BF16) {       // fast mode: every decode linear must have its packed image (both w1 and w3 arrived)
        const char* sfx = g.decode_weight_fp8 ? "#pk8" : "#pk";
        for (int i = 0; i < g.n_layer; ++i) {
            const std::string p = "layers." + std::to_string(i) + ".";
            auto it = c->w13_seen.find(p + "feed_forward.w13.weight");
            if (it != c->w13_seen.end() && it->second != 3) miss.add(p + (it->second == 1 ? "feed_forward.w3.weight" : "feed_forward.w1.weight"));
        }
        for (auto& r : lin) if (Wp(c, r) && !Wp(c, r + sfx)) miss.add(r + sfx);
    }
    if (miss.n) FAIL(c, "car_finalize_weights: %d required tensors missing, e.g. %s", miss.n, miss.names.c_str());
    if (!vq_only && c->mode == CAR_F32) {
        // exact mode: the five decode linears also get their fp32 MFMA-fragment image (decode_f32.hip dec_gemm_f32; the row-major copy stays the
        // prefill operand).  Built on the device from the resident row-major tensor, once.
        for (auto& r : lin) {
            const Wt& src = c->w[r];
            if (src.shape.size() != 2 || src.shape[0] % 16 || src.shape[1] % 16) FAIL(c, "%s: exact-mode decode packing needs N%%16==0 and K%%16==0", r.c_str());
            auto it = c->w.find(r + "#pk32");
            if (it != c->w.end() && it->second.p && it->second.bytes == src.bytes) continue;
            if (ensure_w(c, r + "#pk32", src.bytes, src.shape, src.numel)) return -1;
            // the linears behind an RMSNorm get the norm weight folded into their columns: their decode GEMM multiplies the raw residual rows and applies
            // rstd in its epilogue (decode_f32.hip NX).  The row-major tensor (prefill operand) stays as loaded.
            const void* fold = nullptr;
            auto folded = [&](const char* lin, const char* nrm) { const size_t n = strlen(lin); if (r.size() >= n && r.compare(r.size() - n, n, lin) == 0) fold = Wp(c, r.substr(0, r.size() - n) + nrm); };
            folded("attention.wqkv.weight", "attention_norm.weight"); folded("feed_forward.w13.weight", "ffn_norm.weight");
            if (r == "output.weight") fold = Wp(c, "norm.weight");
            if ((r == "output.weight" || r.find("wqkv") != std::string::npos || r.find("w13") != std::string::npos) && !fold) FAIL(c, "%s: the RMSNorm weight in front of it is missing", r.c_str());
            car_launch_pack_frag_f32(c->w[r].p, c->w[r + "#pk32"].p, src.shape[0], src.shape[1], fold, 0);
        }
        hipError_t e2 = hipStreamSynchronize(0); if (e2 == hipSuccess) e2 = hipGetLastError();
        if (e2 != hipSuccess) FAIL(c, "car_finalize_weights: fp32 fragment packing failed: %s", hipGetErrorString(e2));
    }
    c->finalized = true;
    return 0;
}


// ------------------------------------------------------------------------------------- packed-image cache
// The reference re-reads and re-loads its checkpoints on every start (sample_t2i.py:64-83; demo/model.py:66-75 even per request).
// car_export_packed writes every device-resident weight image of a finalised context (row-major operands, MFMA-fragment / e4m3
// images, scales, conv layouts) plus the host-side tables into one file; car_import_packed restores them with plain copies —
// no conversion, no packing — into a context created with the SAME car_config by the SAME build.  Layout: magic, build id, car_config, entry count, then
// per entry {kind, name, shape, numel, bytes, payload}.  The caller keys the file (controlar_amd/checkpoint.py: content hash).
static const char kPackMagic[8] = {'C', 'A', 'R', 'P', 'K', '0', '3', 0};
static bool same_config(const car_config& a, const car_config& b) {
    car_config x = a, y = b; x.stream_priority = y.stream_priority = 0;
    return memcmp(&x, &y, sizeof(car_config)) == 0;
}
extern "C" int car_export_packed(car_ctx* c, const char* path) {
    if (!c || !path) return -1;
    if (!c->finalized) FAIL(c, "car_export_packed: call car_finalize_weights first");
    (void)hipDeviceSynchronize();
    FILE* f = fopen(path, "wb");
    if (!f) FAIL(c, "car_export_packed: cannot open %s for writing", path);
    char bid[48]; memset(bid, 0, sizeof(bid)); strncpy(bid, car_build_id(), sizeof(bid) - 1);
    bool ok = fwrite(kPackMagic, 1, 8, f) == 8 && fwrite(bid, 1, sizeof(bid), f) == sizeof(bid) && fwrite(&c->cfg, sizeof(car_config), 1, f) == 1;
    const uint64_t n = c->w.size() + c->host_keep.size();
    ok = ok && fwrite(&n, 8, 1, f) == 1;
    std::vector<unsigned char> buf;
    auto put = [&](uint32_t kind, const std::string& name, const std::vector<int64_t>& shape, int64_t numel, const void* data, uint64_t bytes) {
        const uint32_t nl = (uint32_t)name.size(), nd = (uint32_t)shape.size();
        ok = ok && fwrite(&kind, 4, 1, f) == 1 && fwrite(&nl, 4, 1, f) == 1 && fwrite(name.data(), 1, nl, f) == nl && fwrite(&nd, 4, 1, f) == 1;
        if (nd) ok = ok && fwrite(shape.data(), 8, nd, f) == nd;
        ok = ok && fwrite(&numel, 8, 1, f) == 1 && fwrite(&bytes, 8, 1, f) == 1;
        if (bytes) ok = ok && fwrite(data, 1, bytes, f) == bytes;
    };
    for (auto& kv : c->w) {
        const Wt& t = kv.second;
        buf.resize(t.bytes);
        if (t.bytes && hipMemcpy(buf.data(), t.p, t.bytes, hipMemcpyDeviceToHost) != hipSuccess) { fclose(f); FAIL(c, "car_export_packed: device read of %s failed", kv.first.c_str()); }
        put(0, kv.first, t.shape, t.numel, buf.data(), t.bytes);
    }
    for (auto& kv : c->host_keep) put(1, kv.first, {(int64_t)kv.second.size()}, (int64_t)kv.second.size(), kv.second.data(), kv.second.size() * 4);
    ok = (fclose(f) == 0) && ok;
    if (!ok) { remove(path); FAIL(c, "car_export_packed: short write to %s", path); }
    return 0;
}
static int import_packed_impl(car_ctx* c, const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) FAIL(c, "car_import_packed: cannot open %s", path);
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
    (void)fseek(f, 0, SEEK_END); const long fsize = ftell(f); (void)fseek(f, 0, SEEK_SET);
    char magic[8], bid[48]; car_config cfg; uint64_t n = 0;
    if (fsize < 0 || fread(magic, 1, 8, f) != 8 || memcmp(magic, kPackMagic, 8) || fread(bid, 1, sizeof(bid), f) != sizeof(bid) || fread(&cfg, sizeof(car_config), 1, f) != 1 || fread(&n, 8, 1, f) != 1)
        FAIL(c, "car_import_packed: %s is not a packed-weight file of this library version", path);
    { char mine[48]; memset(mine, 0, sizeof(mine)); strncpy(mine, car_build_id(), sizeof(mine) - 1);
      if (memcmp(bid, mine, sizeof(mine))) FAIL(c, "car_import_packed: %s was written by a different build of the library (packed layouts are per build)", path); }
    if (!same_config(cfg, c->cfg)) FAIL(c, "car_import_packed: %s was written for a different car_config", path);
    if (n > (1u << 20)) FAIL(c, "car_import_packed: %s is corrupt (entry count)", path);
    // two passes.  Pass 1 reads the entry HEADERS only (names, shapes, payload sizes checked against the file size; payloads are skipped with fseek), so a
    // truncated or corrupt file fails before the context is touched and without holding several GB of payload on the host (eight ranks of a node import at
    // once).  Pass 2 streams one payload at a time through a bounded staging buffer; a read error there clears the images this call had already imported.
    struct Ent { uint32_t kind; std::string name; std::vector<int64_t> shape; int64_t numel; uint64_t bytes; long offset; };
    std::vector<Ent> ents; ents.reserve((size_t)n);
    for (uint64_t i = 0; i < n; ++i) {
        Ent e; uint32_t nl = 0, nd = 0; uint64_t bytes = 0;
        bool ok = fread(&e.kind, 4, 1, f) == 1 && fread(&nl, 4, 1, f) == 1 && nl > 0 && nl < 4096 && e.kind <= 1;
        if (ok) { e.name.assign((size_t)nl, ' '); ok = fread(&e.name[0], 1, nl, f) == nl && fread(&nd, 4, 1, f) == 1 && nd <= 8; }
        if (ok && nd) { e.shape.resize(nd); ok = fread(e.shape.data(), 8, nd, f) == nd; }
        ok = ok && fread(&e.numel, 8, 1, f) == 1 && fread(&bytes, 8, 1, f) == 1;
        const long here = ok ? ftell(f) : -1;
        ok = ok && here >= 0 && e.numel >= 0 && bytes <= (uint64_t)(fsize - here);             // the payload must fit in what is left of the file
        if (ok && e.kind == 1) ok = bytes == (uint64_t)e.numel * 4;                              // host tables are fp32
        if (ok && e.kind == 0) {                                                                 // device images: 1, 2 or 4 bytes per element of the stated shape
            int64_t prod = 1; for (int64_t d : e.shape) { if (d < 0 || (d && prod > INT64_MAX / d)) { ok = false; break; } prod *= d; }
            ok = ok && prod == e.numel && (bytes == (uint64_t)e.numel || bytes == (uint64_t)e.numel * 2 || bytes == (uint64_t)e.numel * 4);
        }
        if (ok) { e.bytes = bytes; e.offset = here; ok = fseek(f, (long)bytes, SEEK_CUR) == 0; }
        if (!ok) FAIL(c, "car_import_packed: %s is truncated or corrupt (entry %llu)", path, (unsigned long long)i);
        ents.push_back(std::move(e));
    }
    std::vector<std::string> done_w, done_h;
    auto undo = [&]() {      // a failure in pass 2: drop what this call imported, so that the context does not hold half a model
        for (auto& nme : done_w) { auto it = c->w.find(nme); if (it != c->w.end()) { if (it->second.p) (void)hipFree(it->second.p); c->w.erase(it); } c->w13_seen.erase(nme); }
        for (auto& nme : done_h) c->host_keep.erase(nme);
        c->finalized = false;
    };
    std::vector<unsigned char> stage;
    const size_t kStage = (size_t)256 << 20;
    for (Ent& e : ents) {
        if (fseek(f, e.offset, SEEK_SET) != 0) { undo(); FAIL(c, "car_import_packed: seek failed in %s", path); }
        if (e.kind == 1) {
            std::vector<float> v((size_t)e.numel);
            if (e.bytes && fread(v.data(), 1, (size_t)e.bytes, f) != e.bytes) { undo(); FAIL(c, "car_import_packed: read error in %s (%s)", path, e.name.c_str()); }
            c->host_keep[e.name] = std::move(v); done_h.push_back(e.name); continue;
        }
        if (ensure_w(c, e.name, (size_t)e.bytes, e.shape, e.numel)) { undo(); return -1; }
        done_w.push_back(e.name);
        for (uint64_t o = 0; o < e.bytes; o += kStage) {
            const size_t nb = (size_t)std::min<uint64_t>(kStage, e.bytes - o);
            if (stage.size() < nb) stage.resize(nb);
            if (fread(stage.data(), 1, nb, f) != nb) { undo(); FAIL(c, "car_import_packed: read error in %s (%s)", path, e.name.c_str()); }
            if (hipMemcpy((char*)c->w[e.name].p + o, stage.data(), nb, hipMemcpyHostToDevice) != hipSuccess) { undo(); FAIL(c, "car_import_packed: upload of %s failed", e.name.c_str()); }
        }
        if (ends_with(e.name, "feed_forward.w13.weight")) c->w13_seen[e.name] = 3;
    }
    c->finalized = false;
    return car_finalize_weights(c);       // names / shapes are checked against the config there: a missing image fails the import
}
extern "C" int car_import_packed(car_ctx* c, const char* path) {
    if (!c || !path) return -1;
    try { return import_packed_impl(c, path); }
    catch (const std::exception& ex) { c->err = std::string("car_import_packed: ") + ex.what(); return -1; }   // no C++ exception crosses the C ABI
}
