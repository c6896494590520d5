// experiments/nhwc_conv_check.hip — kernel-level pin of the three NHWC implicit-GEMM convolutions on the matrix cores: car_launch_hed_conv (hed.hip),
// car_launch_dpt_conv (dpt.hip) and car_launch_la_conv (lineart.hip), called directly.  Operands are small integers — activations and residuals in
// [-3, 3], weights and projection vectors in [-2, 2], integer biases — so every product and every sum is exact in fp32 (|sum| stays far below 2^24) and
// the expected output has NO tolerance: fp32 mode must equal the host's integer result bit for bit, bf16 mode f2bf of it, the projection partials and
// the DPT map the exact fp32 sums of the rounded channels.  Every case runs with two images (per-image strides with slack behind each image) in both
// modes, twice, and the two runs must agree bit for bit.  Output buffers are pre-filled with a byte pattern and compared whole: a store outside the
// expected elements shows as well.  The shapes are the smallest at which each branch can go wrong (partial tile, tile + tail, exact tiles, masked
// channel tile, stride 2 on odd and even maps, pool over an odd map, element-wise Cin = 3 gather with K below Kp, reflection, a transposed-conv phase).
// For la_conv the raw fp32 tile and cnt are compared; its (mean, M2) partials are covered by tests/test_lineart_gpu.py.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I controlar_amd/csrc experiments/nhwc_conv_check.hip -o experiments/nhwc_conv_check && experiments/nhwc_conv_check quick
#include "../controlar_amd/csrc/hed.hip"
#include "../controlar_amd/csrc/dpt.hip"
#include "../controlar_amd/csrc/lineart.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)

typedef std::vector<unsigned char> bytes;
static const unsigned char FILL = 0xCD;
static unsigned rs = 4242u;
static int irand(int lo, int hi) { rs = rs * 1664525u + 1013904223u; return lo + (int)((rs >> 8) % (unsigned)(hi - lo + 1)); }
static std::vector<int> ivec(size_t n, int lo, int hi) { std::vector<int> v(n); for (auto& x : v) x = irand(lo, hi); return v; }

static std::vector<void*> g_dev;
static void* dalloc(size_t nbytes) { void* d; CK(hipMalloc(&d, nbytes ? nbytes : 16)); g_dev.push_back(d); return d; }
static void dfree_all() { for (void* d : g_dev) CK(hipFree(d)); g_dev.clear(); }
static size_t esz(int mode) { return mode == 1 ? 2 : 4; }
static void put_t(bytes& b, int mode, size_t i, float v) { if (mode == 1) { const bf16_t h = f2bf(v); memcpy(&b[2 * i], &h, 2); } else memcpy(&b[4 * i], &v, 4); }
static void put_f(bytes& b, size_t i, float v) { memcpy(&b[4 * i], &v, 4); }
static float rnd_t(int mode, float v) { return mode == 1 ? bf2f(f2bf(v)) : v; }
static void* up_t(const std::vector<int>& v, int mode) {           // integers as T (every |value| used here is exact in bf16)
    bytes b(v.size() * esz(mode));
    for (size_t i = 0; i < v.size(); ++i) put_t(b, mode, i, (float)v[i]);
    void* d = dalloc(b.size()); CK(hipMemcpy(d, b.data(), b.size(), hipMemcpyHostToDevice)); return d;
}
static float* up_f(const std::vector<int>& v) {
    std::vector<float> f(v.begin(), v.end());
    float* d = (float*)dalloc(f.size() * 4); CK(hipMemcpy(d, f.data(), f.size() * 4, hipMemcpyHostToDevice)); return d;
}
// one output buffer: device memory pre-filled with FILL, the expected bytes (FILL wherever nothing may be written), the bytes of the first run
struct Out {
    void* d = nullptr; bytes want, first;
    void make(size_t nbytes) { want.assign(nbytes, FILL); d = dalloc(nbytes); }
    void reset() { CK(hipMemset(d, FILL, want.size())); }
    int check(const char* what, size_t el, int run) {
        bytes got(want.size()); CK(hipMemcpy(got.data(), d, got.size(), hipMemcpyDeviceToHost));
        int bad = 0;
        if (got != want) { size_t i = 0; while (got[i] == want[i]) ++i; printf("    %s: run %d differs from the host result, first at element %zu of %zu\n", what, run, i / el, want.size() / el); bad = 1; }
        if (run == 0) first = got;
        else if (got != first) { printf("    %s: BITS DIFFER between two runs\n", what); bad = 1; }
        return bad;
    }
};
static int verdict(const char* name, int mode, int bad) { printf("%-68s %s  %s\n", name, mode == 1 ? "bf16" : "fp32", bad ? "FAIL" : "ok"); return bad ? 1 : 0; }

// ---------------------------------------------------------------------------------------------------------------- hed_conv
static int hed_case(const char* name, int mode, int Cin, int N, int Hi, int Wi, int pool, int side) {
    const int H = pool ? Hi / 2 : Hi, W = pool ? Wi / 2 : Wi, M = H * W, K = 9 * Cin, Kp = (K + 31) / 32 * 32, nblk = N / 64;
    const long in_img = (long)Hi * Wi * Cin + 32, out_img = (long)M * N + 64, part_img = (long)nblk * M + 5;
    std::vector<int> in = ivec(2 * in_img, -3, 3), w = ivec((size_t)N * Kp, -2, 2), bias = ivec(N, -20, 20), proj = ivec(N, -2, 2);   // weights beyond K stay non-zero: the A tile is zero there
    if (pool) for (int img = 0; img < 2; ++img) for (int y = 0; y < Hi; ++y) for (int x = 0; x < Wi; ++x)
        if (y >= 2 * H || x >= 2 * W) for (int c = 0; c < Cin; ++c) in[img * in_img + ((long)y * Wi + x) * Cin + c] = 100;        // the odd last row / column: never read
    Out out, part; out.make(2 * out_img * esz(mode)); part.make(2 * part_img * 4);
    auto at = [&](int img, int y, int x, int c) {
        const int* s = &in[img * in_img];
        if (!pool) return s[((long)y * Wi + x) * Cin + c];
        int m = -1000;
        for (int a = 0; a < 2; ++a) for (int b = 0; b < 2; ++b) { const int v = s[((long)(2 * y + a) * Wi + 2 * x + b) * Cin + c]; m = v > m ? v : m; }
        return m;
    };
    for (int img = 0; img < 2; ++img) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        std::vector<float> ps(nblk, 0.f);
        for (int n = 0; n < N; ++n) {
            long s = 0;
            for (int tap = 0; tap < 9; ++tap) {
                const int iy = y + tap / 3 - 1, ix = x + tap % 3 - 1;
                if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
                for (int c = 0; c < Cin; ++c) s += at(img, iy, ix, c) * w[(size_t)n * Kp + tap * Cin + c];
            }
            s += bias[n];
            const float r = rnd_t(mode, (float)(s > 0 ? s : 0));
            put_t(out.want, mode, img * out_img + (long)(y * W + x) * N + n, r);
            ps[n / 64] += r * (float)proj[n];
        }
        if (side) for (int b = 0; b < nblk; ++b) put_f(part.want, img * part_img + (long)b * M + y * W + x, ps[b]);
    }
    HedConvP p; memset(&p, 0, sizeof(p));
    p.in = up_t(in, mode); p.w = up_t(w, mode); p.bias = up_f(bias); p.out = out.d; p.proj = up_t(proj, mode); p.part = side ? (float*)part.d : nullptr;
    p.in_img = in_img; p.out_img = out_img; p.part_img = part_img; p.Hi = Hi; p.Wi = Wi; p.H = H; p.W = W; p.Cin = Cin; p.N = N; p.K = K; p.Kp = Kp; p.pool = pool;
    int bad = 0;
    for (int run = 0; run < 2; ++run) {
        out.reset(); part.reset();
        const int rc = car_launch_hed_conv(mode, &p, 2, 0);
        if (rc) { printf("    car_launch_hed_conv returned %d\n", rc); bad = 1; break; }
        CK(hipDeviceSynchronize());
        bad |= out.check("out", esz(mode), run); bad |= part.check("part", 4, run);
    }
    dfree_all();
    return verdict(name, mode, bad);
}

// ---------------------------------------------------------------------------------------------------------------- dpt_conv
static int dpt_case(const char* name, int mode, int Cin, int N, int Hi, int Wi, int stride, int relu_in, int has_bias, int relu_out, int has_res, int has_proj) {
    const int H = stride == 1 ? Hi : (Hi - 1) / 2 + 1, W = stride == 1 ? Wi : (Wi - 1) / 2 + 1, M = H * W, K = 9 * Cin;
    const long in_img = (long)Hi * Wi * Cin + 32, out_img = (long)M * N + 64, res1_img = (long)M * N + 32, res2_img = (long)M * N + 96, map_img = M + 3;
    std::vector<int> in = ivec(2 * in_img, -3, 3), w = ivec((size_t)N * K, -2, 2), bias = ivec(N, -20, 20), proj = ivec(N, -2, 2), pb = {-7};
    std::vector<int> r1 = ivec(2 * res1_img, -3, 3), r2 = ivec(2 * res2_img, -3, 3);
    Out out, map; out.make(2 * out_img * esz(mode)); map.make(2 * map_img * 4);
    for (int img = 0; img < 2; ++img) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        float ms = 0.f;
        for (int n = 0; n < N; ++n) {
            long s = 0;
            for (int tap = 0; tap < 9; ++tap) {
                const int iy = y * stride + tap / 3 - 1, ix = x * stride + tap % 3 - 1;
                if (iy < 0 || iy >= Hi || ix < 0 || ix >= Wi) continue;
                for (int c = 0; c < Cin; ++c) { const int a = in[img * in_img + ((long)iy * Wi + ix) * Cin + c]; s += (relu_in && a < 0 ? 0 : a) * w[(size_t)n * K + tap * Cin + c]; }
            }
            const long o = (long)(y * W + x) * N + n;
            if (has_bias) s += bias[n];
            if (has_res) s += r1[img * res1_img + o] + r2[img * res2_img + o];
            const float r = rnd_t(mode, (float)(relu_out && s < 0 ? 0 : s));
            if (!has_proj) put_t(out.want, mode, img * out_img + o, r);
            ms += r * (float)proj[n];
        }
        ms += (float)pb[0];
        if (has_proj) put_f(map.want, img * map_img + y * W + x, ms > 0.f ? ms : 0.f);
    }
    DptConvP p; memset(&p, 0, sizeof(p));
    p.in = up_t(in, mode); p.w = up_t(w, mode); p.bias = has_bias ? up_f(bias) : nullptr; p.out = has_proj ? nullptr : out.d;     // with the projection: out NULL, map only
    if (has_res) { p.res1 = up_t(r1, mode); p.res2 = up_t(r2, mode); }
    if (has_proj) { p.proj = up_t(proj, mode); p.proj_bias = up_f(pb); p.map = (float*)map.d; }
    p.in_img = in_img; p.out_img = out_img; p.res1_img = res1_img; p.res2_img = res2_img; p.map_img = map_img;
    p.Hi = Hi; p.Wi = Wi; p.H = H; p.W = W; p.Cin = Cin; p.N = N; p.K = K; p.stride = stride; p.relu_in = relu_in; p.relu_out = relu_out;
    int bad = 0;
    for (int run = 0; run < 2; ++run) {
        out.reset(); map.reset();
        const int rc = car_launch_dpt_conv(mode, &p, 2, 0);
        if (rc) { printf("    car_launch_dpt_conv returned %d\n", rc); bad = 1; break; }
        CK(hipDeviceSynchronize());
        bad |= out.check("out", esz(mode), run); bad |= map.check("map", 4, run);
    }
    dfree_all();
    return verdict(name, mode, bad);
}

// ---------------------------------------------------------------------------------------------------------------- la_conv
enum { LA_7X7_REFLECT = 0, LA_3X3_S2_ZERO = 1, LA_PHASE11 = 2 };
static int la_reflect_host(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }
static int la_case(const char* name, int mode, int kind, int Cin, int N, int Hi, int Wi) {
    LaConvP p; memset(&p, 0, sizeof(p));
    p.Hi = Hi; p.Wi = Wi; p.Cin = Cin; p.N = N; p.stride = 1; p.os = 1;
    if (kind == LA_PHASE11) {                          // odd rows and columns of ConvTranspose2d(k 3, s 2, p 1, output_padding 1): taps (0|1, 0|1) over the input grid
        p.Hg = Hi; p.Wg = Wi; p.Hout = 2 * Hi; p.Wout = 2 * Wi; p.os = 2; p.py = p.px = 1; p.ntaps = 4;
        for (int t = 0; t < 4; ++t) { p.dy[t] = (signed char)(t >> 1); p.dx[t] = (signed char)(t & 1); }
    } else {
        const int ks = kind == LA_7X7_REFLECT ? 7 : 3, pad = ks / 2;
        p.stride = kind == LA_3X3_S2_ZERO ? 2 : 1; p.reflect = kind == LA_7X7_REFLECT; p.ntaps = ks * ks;
        for (int t = 0; t < p.ntaps; ++t) { p.dy[t] = (signed char)(t / ks - pad); p.dx[t] = (signed char)(t % ks - pad); }
        p.Hg = p.Hout = (Hi - 1) / p.stride + 1; p.Wg = p.Wout = (Wi - 1) / p.stride + 1;
    }
    p.K = p.ntaps * Cin; p.Kp = (p.K + 31) / 32 * 32;
    const int Mg = p.Hg * p.Wg, tiles = (Mg + 63) / 64;
    p.tile0 = 1; p.tiles_img = tiles + 2;              // a slot in front of this launch's and one behind: neither may be written
    p.in_img = (long)Hi * Wi * Cin + 32; p.raw_img = (long)p.Hout * p.Wout * N + 64;
    std::vector<int> in = ivec(2 * p.in_img, -3, 3), w = ivec((size_t)N * p.Kp, -2, 2);                                           // weights beyond K stay non-zero: the A tile is zero there
    Out raw, cnt; raw.make(2 * p.raw_img * 4); cnt.make(2 * p.tiles_img * 4);
    for (int img = 0; img < 2; ++img) {
        for (int gy = 0; gy < p.Hg; ++gy) for (int gx = 0; gx < p.Wg; ++gx) for (int n = 0; n < N; ++n) {
            long s = 0;
            for (int t = 0; t < p.ntaps; ++t) {
                int iy = gy * p.stride + p.dy[t], ix = gx * p.stride + p.dx[t];
                if (p.reflect) { iy = la_reflect_host(iy, Hi); ix = la_reflect_host(ix, Wi); }
                if (iy < 0 || iy >= Hi || ix < 0 || ix >= Wi) continue;
                for (int c = 0; c < Cin; ++c) s += in[img * p.in_img + ((long)iy * Wi + ix) * Cin + c] * w[(size_t)n * p.Kp + t * Cin + c];
            }
            put_f(raw.want, img * p.raw_img + ((long)(gy * p.os + p.py) * p.Wout + gx * p.os + p.px) * N + n, (float)s);
        }
        for (int t = 0; t < tiles; ++t) { const int rows = Mg - 64 * t < 64 ? Mg - 64 * t : 64; memcpy(&cnt.want[4 * (img * p.tiles_img + p.tile0 + t)], &rows, 4); }
    }
    p.in = up_t(in, mode); p.w = up_t(w, mode); p.raw = (float*)raw.d; p.cnt = (int*)cnt.d;
    p.part = (float*)dalloc((size_t)2 * p.tiles_img * N * 8);
    int bad = 0;
    for (int run = 0; run < 2; ++run) {
        raw.reset(); cnt.reset();
        const int rc = car_launch_la_conv(mode, &p, 2, 0);
        if (rc) { printf("    car_launch_la_conv returned %d\n", rc); bad = 1; break; }
        CK(hipDeviceSynchronize());
        bad |= raw.check("raw", 4, run); bad |= cnt.check("cnt", 4, run);
    }
    dfree_all();
    return verdict(name, mode, bad);
}

// ---------------------------------------------------------------------------------------------------------------- refusals
// every refused parameter block must return hipErrorInvalidValue and launch nothing: the output buffer keeps its fill
static int refusals(int mode) {
    int fails = 0;
    Out out; out.make(64 * 1024); out.reset();
    void* src = dalloc(256 * 1024); CK(hipMemset(src, 0, 256 * 1024));
    HedConvP h; memset(&h, 0, sizeof(h));
    h.in = src; h.w = src; h.bias = (const float*)src; h.out = out.d; h.Hi = h.H = 8; h.Wi = h.W = 8; h.Cin = 32; h.N = 64; h.K = h.Kp = 288;
    DptConvP d; memset(&d, 0, sizeof(d));
    d.in = src; d.w = src; d.out = out.d; d.Hi = d.H = 8; d.Wi = d.W = 8; d.Cin = 32; d.N = 64; d.K = 288; d.stride = 1;
    auto expect = [&](const char* what, int rc) {
        const bool ok = rc == (int)hipErrorInvalidValue;
        printf("refused: %-59s %s  %s\n", what, mode == 1 ? "bf16" : "fp32", ok ? "ok" : "FAIL");
        if (!ok) { printf("    returned %d\n", rc); ++fails; }
    };
    { HedConvP q = h; q.N = 96; expect("hed N % 64", car_launch_hed_conv(mode, &q, 2, 0)); }
    { HedConvP q = h; q.H = 7; expect("hed H != Hi without the pool", car_launch_hed_conv(mode, &q, 2, 0)); }
    { HedConvP q = h; q.pool = 1; expect("hed H != Hi / 2 with the pool", car_launch_hed_conv(mode, &q, 2, 0)); }
    { HedConvP q = h; q.pool = 1; q.Hi = 17; q.Wi = 16; q.W = 9; expect("hed W != Wi / 2 with the pool", car_launch_hed_conv(mode, &q, 2, 0)); }
    { DptConvP q = d; q.Cin = 48; q.K = 432; expect("dpt Cin % 32", car_launch_dpt_conv(mode, &q, 2, 0)); }
    { DptConvP q = d; q.H = 4; expect("dpt H != Hi at stride 1", car_launch_dpt_conv(mode, &q, 2, 0)); }
    { DptConvP q = d; q.stride = 2; expect("dpt H != (Hi - 1) / 2 + 1 at stride 2", car_launch_dpt_conv(mode, &q, 2, 0)); }
    { DptConvP q = d; q.stride = 2; q.Hi = q.Wi = 9; q.H = 5; q.W = 4; expect("dpt W != (Wi - 1) / 2 + 1 at stride 2", car_launch_dpt_conv(mode, &q, 2, 0)); }
    CK(hipDeviceSynchronize());
    fails += out.check("out after the refused launches", 1, 0);
    dfree_all();
    return fails;
}

int main(int, char**) {                                // one size only: the `quick` argument of the other harnesses is accepted and changes nothing
    int fails = 0;
    for (int mode = 0; mode < 2; ++mode) {
        fails += hed_case("hed Cin 3 (K 27 in 32) 5x7 N 64: one partial tile", mode, 3, 64, 5, 7, 0, 0);
        fails += hed_case("hed Cin 32 N 128 19x31 pooled to 9x15 (tile + 7 rows), side partials", mode, 32, 128, 19, 31, 1, 1);
        fails += hed_case("hed Cin 64 N 64 16x16: two full tiles, no pool", mode, 64, 64, 16, 16, 0, 0);
        fails += dpt_case("dpt Cin 32 N 96 12x12 stride 1, relu_in, bias, relu_out", mode, 32, 96, 12, 12, 1, 1, 1, 1, 0, 0);
        fails += dpt_case("dpt Cin 64 N 64 9x9 -> 5x5 stride 2, res1 + res2", mode, 64, 64, 9, 9, 2, 0, 0, 0, 1, 0);
        fails += dpt_case("dpt Cin 64 N 64 8x8 -> 4x4 stride 2, res1 + res2", mode, 64, 64, 8, 8, 2, 0, 0, 0, 1, 0);
        fails += dpt_case("dpt Cin 32 N 32 11x13 bias, relu_out, projection -> map, out NULL", mode, 32, 32, 11, 13, 1, 0, 1, 1, 0, 1);
        fails += la_case("la 7x7 reflect Cin 3 (K 147 in 160) 9x9 N 64", mode, LA_7X7_REFLECT, 3, 64, 9, 9);
        fails += la_case("la 3x3 zero pad stride 2 Cin 64 N 128 9x7 -> 5x4", mode, LA_3X3_S2_ZERO, 64, 128, 9, 7);
        fails += la_case("la transposed phase (1, 1), four taps, Cin 32 N 64, 6x5 grid", mode, LA_PHASE11, 32, 64, 6, 5);
        fails += refusals(mode);
    }
    if (fails) { printf("%d checks FAILED\n", fails); return 1; }
    printf("all checks passed\n");
    return 0;
}
