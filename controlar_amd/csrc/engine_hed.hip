// engine_hed.hip — car_hed: the HED edge extractor (condition/hed.py:17-81; callers sample_t2i.py:108-109,126-128, sample_t2i_MR.py,
// autoregressive/test/test_t2i.py:172-173, test_c2i.py, evaluations/hed_ssim.py) as a chain of hed.hip launches, and the loader of its weight images ("hed.*").
// (one of the translation units behind include/controlar_hip.h; shared declarations: engine_internal.h)
#include "engine_internal.h"

extern "C" {
int car_launch_hed_to_nhwc(int mode, const float* img, const float* norm, void* out, long HW, hipStream_t st);
int car_launch_hed_conv(int mode, const HedConvP* p, int nimg, hipStream_t st);
int car_launch_hed_fuse(int mode, const HedFuseP* p, int nimg, hipStream_t st);
}

#define HEDCHK(ctx, x) do { const int _e = (x); if (_e != 0) FAIL(ctx, "car_hed: %s failed: %s (%s:%d)", #x, hipGetErrorString((hipError_t)_e), __FILE__, __LINE__); } while (0)

// ControlNetHED_Apache2 (condition/hed.py:36-44): input channels, output channels and 3x3 convs of block1..5 (the loader, the name list and the runner)
static const int kCin[5] = {3, 64, 128, 256, 512}, kCout[5] = {64, 128, 256, 512, 512}, kConvs[5] = {2, 2, 3, 3, 3};

// the 37 tensors of its state_dict(), under the "hed." prefix of the C ABI
void hed_tensor_names(const car_ctx*, std::vector<std::string>& v) {
    v.push_back("hed.norm");
    for (int b = 0; b < 5; ++b) {
        const std::string p = "hed.block" + std::to_string(b + 1) + ".";
        for (int i = 0; i < kConvs[b]; ++i) for (const char* s : {".weight", ".bias"}) v.push_back(p + "convs." + std::to_string(i) + s);
        v.push_back(p + "projection.weight"); v.push_back(p + "projection.bias");
    }
}

// 3x3 conv weights become implicit-GEMM images [Cout][9*Cin] (k = tap*Cin + ci, K padded to the 32-wide k step: 27 -> 32 for block1.convs.0) in the
// context's element type; a 1x1 side projection becomes its [Cout] vector in the element type (the reference projects the stored activation with a conv in
// the model dtype); norm and every bias stay fp32.
int hed_load_tensor(car_ctx* c, const LoadedTensor& t) {
    const std::string& name = t.name;
    const std::vector<int64_t>& shp = t.shape;
    std::vector<std::string> names;
    hed_tensor_names(c, names);
    if (!has_name(names, name)) FAIL(c, "%s: not a tensor of the HED network (ControlNetHED_Apache2)", t.cname);
    if (name == "hed.norm") {
        if (t.n != 3) FAIL(c, "%s: expected [1,3,1,1]", t.cname);
        return upload(c, name, t.h, {3}, true);
    }
    const int blk = name[9] - '1';                          // "hed.blockN."
    const int Co = kCout[blk];
    if (ends_with(name, "projection.bias")) { if (t.n != 1) FAIL(c, "%s: expected [1]", t.cname); return upload(c, name, t.h, {1}, true); }
    if (ends_with(name, "projection.weight")) {
        if (t.ndim() != 4 || shp[0] != 1 || shp[1] != Co || shp[2] != 1 || shp[3] != 1) FAIL(c, "%s: expected [1,%d,1,1]", t.cname, Co);
        return upload(c, name, t.h, {Co});
    }
    if (ends_with(name, ".bias")) { if (t.ndim() != 1 || shp[0] != Co) FAIL(c, "%s: expected [%d]", t.cname, Co); return upload(c, name, t.h, shp, true); }
    const int Ci = name.compare(11, 8, "convs.0.") == 0 ? kCin[blk] : Co, Kp = conv_kp(9 * Ci);
    if (t.ndim() != 4 || shp[0] != Co || shp[1] != Ci || shp[2] != 3 || shp[3] != 3) FAIL(c, "%s: expected [%d,%d,3,3]", t.cname, Co, Ci);
    return upload(c, name, pack_conv(t.h.data(), Co, Ci, 3, 3, Kp), {Co, Kp});
}

extern "C" int car_hed(car_ctx* c, const float* img_nchw, int32_t B, int32_t H, int32_t W, float* out, void* control_out, void* stream_) {
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!img_nchw || B <= 0 || (!out && !control_out)) FAIL(c, "car_hed: bad arguments");
    // the reference raises below 16: four 2x2 pools turn 15 into 0
    if (H < 16 || W < 16) FAIL(c, "car_hed: the image must be at least 16 x 16 (got %d x %d): four 2x2 max-pools leave no pixel below that", H, W);
    if ((long)H * W > (1L << 26)) FAIL(c, "car_hed: image too large");
    if (!Wp(c, "hed.norm") || !c->finalized) FAIL(c, "car_hed: the context holds no HED weights (load hed.* tensors, then car_finalize_weights)");
    const size_t P = (size_t)H * W, esz = c->esz;
    // per-image bytes: the NHWC copy of the image, two activation buffers (the largest map is 64 channels at full resolution), the side partials
    const size_t b_in3 = rup(P * 3 * esz, 256), b_act = rup(P * 64 * esz, 256);
    size_t b_part[5], b_parts = 0;
    for (int l = 0; l < 5; ++l) { b_part[l] = rup((size_t)(kCout[l] / 64) * (H >> l) * (W >> l) * 4, 256); b_parts += b_part[l]; }
    const size_t per_img = b_in3 + 2 * b_act + b_parts;
    // chunking: large batches run as groups of images inside a bounded workspace (every step is image-local, so the grouping changes no bit)
    const size_t budget = (size_t)1536 << 20;
    const int chunk = (int)std::min<size_t>((size_t)B, std::max<size_t>(1, budget / per_img));
    NEED(c, c->hed_ws, per_img * chunk);
    char* base = (char*)c->hed_ws.p;
    char* in3 = base; base += b_in3 * chunk;
    char* act[2]; for (int i = 0; i < 2; ++i) { act[i] = base; base += b_act * chunk; }
    float* part[5]; for (int l = 0; l < 5; ++l) { part[l] = (float*)base; base += b_part[l] * chunk; }
    const long in3_img = (long)(b_in3 / esz), act_img = (long)(b_act / esz);
    const float* norm = (const float*)Wp(c, "hed.norm");
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        const float* src = img_nchw + (size_t)b0 * 3 * P;
        for (int i = 0; i < nb; ++i) HEDCHK(c, car_launch_hed_to_nhwc(c->mode, src + (size_t)i * 3 * P, norm, in3 + (size_t)i * in3_img * esz, (long)P, st));
        HedFuseP f; memset(&f, 0, sizeof(f));
        const void* cur = in3; long cur_img = in3_img; int x = 0;
        for (int l = 0; l < 5; ++l) {
            const std::string blk = "hed.block" + std::to_string(l + 1) + ".";
            const int Hl = H >> l, Wl = W >> l;
            for (int i = 0; i < kConvs[l]; ++i) {
                const std::string cv = blk + "convs." + std::to_string(i);
                HedConvP p; memset(&p, 0, sizeof(p));
                p.in = cur; p.in_img = cur_img; p.out = act[x]; p.out_img = act_img;
                p.w = Wp(c, cv + ".weight"); p.bias = (const float*)Wp(c, cv + ".bias");
                if (!p.w || !p.bias) FAIL(c, "car_hed: %s is not loaded", cv.c_str());
                p.Cin = i == 0 ? kCin[l] : kCout[l]; p.N = kCout[l]; p.K = 9 * p.Cin; p.Kp = conv_kp(p.K);
                p.pool = (i == 0 && l > 0) ? 1 : 0;
                p.H = Hl; p.W = Wl; p.Hi = p.pool ? H >> (l - 1) : Hl; p.Wi = p.pool ? W >> (l - 1) : Wl;
                if (i == kConvs[l] - 1) {              // the block's side output rides in its last conv
                    p.proj = Wp(c, blk + "projection.weight"); p.part = part[l]; p.part_img = (long)(b_part[l] / 4);
                    f.bias[l] = (const float*)Wp(c, blk + "projection.bias");
                    if (!p.proj || !f.bias[l]) FAIL(c, "car_hed: %sprojection is not loaded", blk.c_str());
                    f.part[l] = part[l]; f.part_img[l] = p.part_img; f.nblk[l] = kCout[l] / 64;
                }
                HEDCHK(c, car_launch_hed_conv(c->mode, &p, nb, st));
                cur = act[x]; cur_img = act_img; x ^= 1;
            }
        }
        f.out = out ? out + (size_t)b0 * P : nullptr;
        f.control = control_out ? (char*)control_out + (size_t)b0 * 3 * P * esz : nullptr;
        f.H = H; f.W = W;
        HEDCHK(c, car_launch_hed_fuse(c->mode, &f, nb, st));
    }
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}
