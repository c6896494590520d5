// experiments/ops_check.hip — the helper kernels of controlar_amd/csrc/ops.hip and t5.hip through their real car_launch_* entry points against EXACT references:
// GroupNorm (gn_partial / gn_partial_vec / gn_finalize / gn_apply / gn_apply_vec), vq_argmin, vq_lookup, conv_out (scalar and MFMA form), conv_in3, rmsnorm_kernel,
// layernorm_kernel, swiglu, swiglu_parts, t5_gated_act, convert, build_text, gather_rows, label_index, t5_prep, patchify, vit_assemble, ctrl_scale_rows,
// row_mix_scale, set_pos_step, advance.  (The softmax kernels, transpose_pad and t5_softmax belong to attn_check.hip, the samplers to tests/test_sampler_gpu.py.)
// Compiled with -DCAR_DEV_KNOBS so that CAR_GN_SCALAR is live; CAR_KNOB reads the environment at every launch, so the harness sets and unsets it per case.
//
// Every buffer of a case lives in ONE arena poisoned with 0xff bytes, 256 guard bytes in front of, between and behind the buffers.  After the launch the WHOLE arena is
// compared with the expected image: outputs, unchanged inputs, guards.  Every case runs twice (equal bits), on two images / several rows with different data, in both
// modes where the kernel has both.  Before a launch every pointer is taken through need(), which asserts on the host that the bytes the launch may touch (computed
// from the launch parameters) lie inside the buffer; `selftest` runs the same assertions without a GPU.
//
// NO tolerance wherever the arithmetic can be made exact: operands are small hashed integers, powers of two or dyadic fractions, so every fp32 partial sum is an exact
// integer multiple of a unit and below 2^24 units whatever the order of the summation (the builders check that per output element: "PRECONDITION"); one final rounding
// of an exact value to bf16 has one possible result.  The bf16 rounding of the references is written out below (r_bf: nearest-even, ties, NaN quieted with its
// payload, overflow to inf) and does not call f2bf / bf2f of car_common.h, which convert_kernel is built from.
//
// Derived bounds (never measured), worst error / bound printed per case:
//   stats      gn_finalize works in double on exact integer partials; only the contraction of q/n - mean*mean is not fixed -> the rounded float of the host's
//              double expression or one of its two neighbours.  Sign rows x = +-2^a(b, g): mean 0, var 4^a, rstd 2^-a, all exact.
//   swish      y = v / (1 + e), e = expf(-v): expf 1 ulp (HIP math API), the add and the correctly rounded division half an ulp each:
//              |dy| <= (2^-23 e/(1+e) + 2^-24 + 2^-24) |y| <= 2^-22 |y| in fp32; in bf16 the rounded fp64 function or its neighbour (one bf16 ulp) on at most 1 % of the
//              elements, the rule of gemm_check.hip — for expf and for gn_apply_vec_kernel's __expf alike (their difference, a few 2^-23, is far below 2^-9).
//   rstd(GN)   dense data: one stage-1 partial is an fp32 chain of L adds (ceil(256 / nslot) pixels of a slot, nslot - 1 folds, one product rounding), each
//              2^-24 relative to the running sum <= q; stage 2 is double.  d(var) <= L 2^-24 q/n, hence d(rstd)/rstd <= L 2^-24 (q/n) / (var + eps)
//              (first order; the factor 1/2 of the square root pays for the same error of mean^2).  fp32-grade while mean/std stays small: at mean/std = 16 the
//              bound itself is 257 L 2^-24.
//   argmin     fp32 distance d = z2 + e2 - 2 dot of normalised vectors: z2, e2 chains of cd terms (cd 2^-24 each, values <= 1 + ...), the normalisations
//              (sqrt, reciprocal, product: 3 x 2^-24 per component, entering z2, e2 and dot twice), dot cd fmas, two final roundings on values <= 4:
//              |d - d64| <= (2 cd + 16) 2^-24 * 2 = (2 cd + 16) 2^-23 covers both the winner's and the runner-up's error.
//   lookup     inv = 1 / max(sqrt(nn), 1e-12): nn chain cd, sqrt, reciprocal; e * inv one rounding; cd fmas; the bias add:
//              |dz| <= (cd + 5) 2^-24 (sum_k |w_k e_k| / |e| + |b|)  (+ half a bf16 ulp of the result in bf16 mode).
//   layernorm  mean: chain L = ceil(D/128) + 8 (a thread's columns, six butterfly steps, two waves); d = x - mean; var the same chain; rsqrtf 1 ulp:
//              |dy| <= (L + 8) 2^-24 |w| rstd (|d| + mean|x|) + 2^-24 |y|  (+ half a bf16 ulp in bf16 mode).  Sign rows x = c(r) +- 2^a(r) (D even): mean c, rstd
//              2^-a to rsqrtf's ulp, y = +-w + b with |b| > |w|: a bf16 store has one possible result (memcmp); fp32 within 4 2^-24 |w| + 2^-24 |y|.
//   rmsnorm    no bound at all: integer rows have an exact sum of squares, so every row must be bit-equal to the row computed with ONE of three candidate rstd values
//              (the correctly rounded 1/sqrt and its neighbours: rsqrtf's documented 1 ulp), in both modes.  Sign rows +-2^a(r) make the three rows coincide in bf16
//              mode: rnd(v rstd) = +-1 for every rstd within 2 ulp, eps = 1e-5 and 0 (checked).  fp32 mode uses dyadic cs only (v + cs c may contract to an fma).
//   SwiGLU     the bound of gemm_check.hip in bf16 mode: ulp(gate) |c| + ulp(out) from the rounded fp64 function on at most 1 % of the elements, SiLU over |x| <= 30.5,
//              GELU-tanh over [-3.5, 30.5].  fp32 mode: SiLU 5 2^-24 |ref| (the swish bound plus the product); GELU-tanh 10 2^-24 |x g / 2| + 4 2^-24 |ref| (tanhf 2 ulp
//              and the argument's three roundings through tanh' <= 1, the sum 1 + tanh, two products).  The layout itself has no tolerance: gates are integers in
//              [24, 60], where silu(a) and gelu_new(a) round to a in fp32 and bf16 (selftest: within 2^-30 relative in fp64).
//
//   quick      all device checks, one line per case; prints "all checks passed"
//   selftest   no HIP call: every case's data, reference, extents and exactness preconditions on the host
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -DCAR_DEV_KNOBS -I controlar_amd/csrc experiments/ops_check.hip -o experiments/ops_check && experiments/ops_check quick
#ifndef CAR_DEV_KNOBS
#error "ops_check needs -DCAR_DEV_KNOBS: without it CAR_KNOB() is a null constant and the CAR_GN_SCALAR cases would silently run the vector route"
#endif
#include "../controlar_amd/csrc/ops.hip"
#include "../controlar_amd/csrc/t5.hip"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

extern "C" { int g_car_knob_hits = 0; }        // the development build's counter lives in engine.hip, which is not part of this program

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)

typedef unsigned char u8;
static int g_fail = 0, g_cases = 0;
static bool g_selftest = false, g_dry = false;
static u8* g_base = nullptr;          // arena base of the running case (a fake address during the host-only extent pass)
#define GO(call) do { if (!g_dry) { call; } } while (0)

static unsigned hsh(unsigned a, unsigned b, unsigned seed) {
    unsigned x = a * 2654435761u + b * 0x85ebca6bu + seed * 0x9e3779b9u; x ^= x >> 15; x *= 2246822519u; x ^= x >> 13; x *= 3266489917u; x ^= x >> 16; return x;
}
static int hint(unsigned a, unsigned b, unsigned seed, int lo, int hi) { return lo + (int)(hsh(a, b, seed) % (unsigned)(hi - lo + 1)); }
static double gauss(unsigned a, unsigned b, unsigned seed) {
    const double u1 = (hsh(a, b, seed * 2u + 1u) + 1.0) / 4294967297.0, u2 = hsh(a, b, seed * 2u + 2u) / 4294967296.0;
    return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
}

// ---------------------------------------------------------------------------------------------------------------- the reference's own bf16 (not car_common.h's)
static uint16_t r_bf(float f) {
    uint32_t u; memcpy(&u, &f, 4);
    if (((u >> 23) & 0xffu) == 0xffu && (u & 0x7fffffu)) return (uint16_t)((u >> 16) | 0x40u);      // NaN: quieted, sign and the upper payload kept
    uint32_t hi = u >> 16; const uint32_t lo = u & 0xffffu;
    if (lo > 0x8000u || (lo == 0x8000u && (hi & 1u))) ++hi;      // nearest, ties to even; a carry out of the mantissa raises the exponent, 0x7f7f -> inf
    return (uint16_t)hi;
}
static float bfv(uint16_t b) { const uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; }
static float rT(int mode, float v) { return mode == 1 ? bfv(r_bf(v)) : v; }
static int esz(int mode) { return mode == 1 ? 2 : 4; }
static double ulp_bf16(double v) { if (v == 0 || !(std::fabs(v) < 1e300)) return 0; int e; (void)std::frexp(std::fabs(v), &e); return std::ldexp(1.0, e - 8); }
// single IEEE operations the host compiler must not fuse
static float fmul(float a, float b) {
#pragma clang fp contract(off)
    volatile float r = a * b; return r;
}
static float fadd(float a, float b) {
#pragma clang fp contract(off)
    volatile float r = a + b; return r;
}
static float fdiv(float a, float b) { volatile float r = a / b; return r; }
static double silu64(double x) { return x / (1.0 + std::exp(-x)); }
static double gelu64(double x) { return 0.5 * x * (1.0 + std::tanh(0.79788456080286535588 * (x + 0.044715 * x * x * x))); }

template <typename X> static void putv(std::vector<u8>& im, size_t off, size_t i, X v) { memcpy(&im[off + i * sizeof(X)], &v, sizeof(X)); }
template <typename X> static X getv(const u8* im, size_t off, size_t i) { X v; memcpy(&v, im + off + i * sizeof(X), sizeof(X)); return v; }
static void put(std::vector<u8>& im, size_t off, size_t i, int mode, float v) { if (mode == 1) putv<uint16_t>(im, off, i, r_bf(v)); else putv<float>(im, off, i, v); }
static float get(const u8* im, size_t off, size_t i, int mode) { return mode == 1 ? bfv(getv<uint16_t>(im, off, i)) : getv<float>(im, off, i); }

// ---------------------------------------------------------------------------------------------------------------- arena + runner
struct Arena {
    std::vector<u8> init, exp, soft;          // soft[i] != 0: byte belongs to an output with a derived bound (checked by the case's own function, not by memcmp)
    std::vector<size_t> off, len;
    int add(size_t bytes) {
        const size_t o = ((init.size() + 255) / 256) * 256 + 256;
        off.push_back(o); len.push_back(bytes); init.resize(o + bytes, 0xff); return (int)off.size() - 1;
    }
    void seal() { init.resize(((init.size() + 255) / 256) * 256 + 256, 0xff); exp = init; soft.assign(init.size(), 0); }
    void mark_soft(int id) { memset(&soft[off[id]], 1, len[id]); }
};
struct Case {
    std::string name; Arena A; bool pre = true; std::string why; const char* knob = nullptr;
    std::function<void()> launch;
    std::function<double(const u8* got, std::string& msg)> soft;      // worst error / bound (> 1 fails); msg: extra text for the case line
    std::vector<u8> got;
    const Case* same_as = nullptr; int same_buf = -1;               // report (and with same_exact require 0) differing elements of one buffer against another case's run
    bool same_exact = false; int same_esz = 2;
};
// pointer into buffer `id` of the running case; `bytes` = what the launch may touch from there
static void* need(const Case& c, int id, size_t bytes, size_t at = 0) {
    if (id < 0 || id >= (int)c.A.off.size() || at + bytes > c.A.len[id]) { printf("%s: EXTENT FAIL buffer %d needs %zu + %zu bytes of %zu\n", c.name.c_str(), id, at, bytes, id >= 0 && id < (int)c.A.len.size() ? c.A.len[id] : 0); exit(3); }
    return g_base + c.A.off[id] + at;
}
static void pre_fail(Case& c, const std::string& w) { if (c.pre) { c.pre = false; c.why = w; } }

static u8* g_dev = nullptr; static size_t g_dev_cap = 0;
static void run(Case& c) {
    ++g_cases;
    if (!c.pre) { printf("%-74s PRECONDITION %s FAIL\n", c.name.c_str(), c.why.c_str()); ++g_fail; return; }
    g_dry = true; g_base = (u8*)(uintptr_t)0x10000000; c.launch();      // host-only pass: every extent asserted, nothing launched
    if (g_selftest) { printf("%-74s host ok (%zu bytes)\n", c.name.c_str(), c.A.init.size()); return; }
    const size_t n = c.A.init.size();
    if (n > g_dev_cap) { if (g_dev) CK(hipFree(g_dev)); g_dev_cap = n + (n >> 2); CK(hipMalloc((void**)&g_dev, g_dev_cap)); }
    std::vector<u8> got2(n); c.got.resize(n);
    for (int rep = 0; rep < 2; ++rep) {
        CK(hipMemcpy(g_dev, c.A.init.data(), n, hipMemcpyHostToDevice));
        if (c.knob) setenv(c.knob, "1", 1);
        g_dry = false; g_base = g_dev; c.launch();
        if (c.knob) unsetenv(c.knob);
        CK(hipGetLastError()); CK(hipDeviceSynchronize());
        CK(hipMemcpy(rep ? got2.data() : c.got.data(), g_dev, n, hipMemcpyDeviceToHost));
    }
    bool ok = true; std::string msg;
    if (memcmp(c.got.data(), got2.data(), n) != 0) { ok = false; msg += " BITS DIFFER between two runs"; }
    for (size_t i = 0; i < n; ++i) if (!c.A.soft[i] && c.got[i] != c.A.exp[i]) {
        int b = -1; for (size_t k = 0; k < c.A.off.size(); ++k) if (i >= c.A.off[k] && i < c.A.off[k] + c.A.len[k]) b = (int)k;
        char t[160]; snprintf(t, sizeof t, " byte %zu (buffer %d + %zu): got %02x expected %02x", i, b, b >= 0 ? i - c.A.off[b] : i, c.got[i], c.A.exp[i]);
        ok = false; msg += t; break;
    }
    double ratio = -1;
    if (c.soft) { std::string m2; ratio = c.soft(c.got.data(), m2); if (!(ratio <= 1.0)) ok = false; char t[64]; snprintf(t, sizeof t, " worst/bound %.3f", ratio); msg += t; msg += m2; }
    if (c.same_as && c.same_as->got.size() && c.same_buf >= 0) {
        const size_t o = c.A.off[c.same_buf], o2 = c.same_as->A.off[c.same_buf], l = c.A.len[c.same_buf]; size_t nd = 0;
        for (size_t i = 0; i + c.same_esz <= l; i += c.same_esz) if (memcmp(&c.got[o + i], &c.same_as->got[o2 + i], c.same_esz) != 0) ++nd;
        char t[96]; snprintf(t, sizeof t, " differs from '%s' on %zu of %zu", c.same_as->name.c_str(), nd, l / c.same_esz); msg += t;
        if (c.same_exact && nd) ok = false;
    }
    printf("%-74s %s%s\n", c.name.c_str(), ok ? "ok" : "FAIL", msg.c_str());
    if (!ok) ++g_fail;
}
// lowest set bit of a finite non-zero double, as a power of two
static double lsb(double v) { int e; double m = std::frexp(std::fabs(v), &e); int k = 0; while (m != std::floor(m) && k < 60) { m *= 2; ++k; } return std::ldexp(1.0, e - k); }
// true iff a sum of the non-negative terms is exact in fp32 in every order: all are multiples of one unit and the total stays below 2^24 units
static bool exact_sum_ok(const std::vector<double>& terms) {
    double unit = 0, tot = 0;
    for (double t : terms) if (t != 0) { const double l = lsb(t); if (unit == 0 || l < unit) unit = l; tot += std::fabs(t); }
    return unit == 0 || tot / unit < 16777216.0;
}

// ================================================================================================================ GroupNorm
struct GnOpt {
    int mode = 1, HW = 64, C = 64, B = 2; int data = 0;        // data 0: integers (stage 1 only), 1: sign rows, 2: dense gaussian (fp32, statistics only)
    bool with_y = false, swish = false, have_part = false, direct_scalar = false; const char* knob = nullptr; double ms = 0; float eps = 1e-6f; unsigned seed = 1;
};
static int gn_chain(int mode, int C) {      // longest fp32 add chain of one stage-1 partial (+1: the rounding of the square)
    const bool vec = mode == 1 && C >= 8 && C <= 2048 && (C & (C - 1)) == 0;
    if (!vec && C > 256) return 256 + 1;
    const int nslot = vec ? 256 / (C >> 3) : 256 / C;
    return (256 + nslot - 1) / nslot + nslot - 1 + 1;
}
static std::shared_ptr<Case> gn_case(const GnOpt& o) {
    auto cp = std::make_shared<Case>(); Case& c = *cp;
    const int G = 32, cpg = o.C / G, nchunk = (o.HW + 255) / 256, es = esz(o.mode); const long nx = (long)o.B * o.HW * o.C;
    char nm[200]; snprintf(nm, sizeof nm, "groupnorm %s HW %d C %d %s%s%s%s%s%s", o.mode ? "bf16" : "fp32", o.HW, o.C, o.data == 0 ? "ints" : o.data == 1 ? "sign" : "dense",
                           o.with_y ? " y" : " stats-only", o.swish ? " swish" : "", o.have_part ? " have_part" : "", o.knob ? " CAR_GN_SCALAR" : "", o.direct_scalar ? " gn_partial_kernel<bf16> direct" : "");
    c.name = nm; if (o.data == 2) { char t[40]; snprintf(t, sizeof t, " mean/std %g", o.ms); c.name += t; }
    c.knob = o.knob;
    const int bx = c.A.add(nx * es), bg = c.A.add((size_t)o.C * es), bb = c.A.add((size_t)o.C * es), by = o.with_y ? c.A.add(nx * es) : -1;
    const int bp = c.A.add((size_t)o.B * nchunk * 2 * o.C * 4), bs = c.A.add((size_t)o.B * G * 2 * 4);
    std::vector<float> x(nx), gam(o.C), bet(o.C);
    std::vector<int> aexp((size_t)o.B * G, 0);
    for (int b = 0; b < o.B; ++b) for (int g = 0; g < G; ++g) aexp[b * G + g] = hint(b, g, o.seed * 8 + 1, -3, 3);
    if (o.data == 1 && ((long)o.HW * cpg) % 2) pre_fail(c, "sign rows need an even group");
    for (int b = 0; b < o.B; ++b) for (int p = 0; p < o.HW; ++p) for (int ch = 0; ch < o.C; ++ch) {
        const long i = ((long)b * o.HW + p) * o.C + ch; const int g = ch / cpg;
        if (o.data == 0) x[i] = (float)hint((unsigned)(b * o.HW + p), ch, o.seed * 8 + 2, -4, 4);
        else if (o.data == 1) { const long e = (long)p * cpg + (ch - g * cpg); const int s = (hsh((unsigned)(b * G + g), (unsigned)(e >> 1), o.seed * 8 + 3) & 1) ^ (int)(e & 1); x[i] = std::ldexp(s ? -1.f : 1.f, aexp[b * G + g]); }
        else x[i] = (float)(o.ms + gauss((unsigned)(b * o.HW + p), ch, o.seed * 8 + 4));
    }
    for (int ch = 0; ch < o.C; ++ch) { gam[ch] = (float)hint(ch, 0, o.seed * 8 + 5, -3, 3); bet[ch] = (float)hint(ch, 1, o.seed * 8 + 5, -4, 4); }
    for (long i = 0; i < nx; ++i) put(c.A.init, c.A.off[bx], i, o.mode, x[i]);
    for (int ch = 0; ch < o.C; ++ch) { put(c.A.init, c.A.off[bg], ch, o.mode, gam[ch]); put(c.A.init, c.A.off[bb], ch, o.mode, bet[ch]); }
    // stage-1 partials of x (exact for data 0 / 1), or of 2x when the host supplies them (have_part: the statistics must come from `part`, not from x)
    const double pf = o.have_part ? 2.0 : 1.0;
    std::vector<double> ps((size_t)o.B * nchunk * o.C, 0), pq(ps.size(), 0);
    for (int b = 0; b < o.B; ++b) for (int p = 0; p < o.HW; ++p) for (int ch = 0; ch < o.C; ++ch) {
        const double v = pf * x[((long)b * o.HW + p) * o.C + ch]; const size_t k = ((size_t)b * nchunk + p / 256) * o.C + ch; ps[k] += v; pq[k] += v * v;
    }
    if (o.data != 2) {      // every term of a partial is a multiple of one unit (1 for the integers, (pf 2^a)^2 for the sign rows of a group): exact while below 2^24 units
        for (int b = 0; b < o.B; ++b) for (int k = 0; k < nchunk; ++k) for (int ch = 0; ch < o.C; ++ch) {
            const double unit = o.data == 0 ? 1.0 : pf * pf * std::ldexp(1.0, 2 * aexp[b * G + ch / cpg]);
            if (!(pq[((size_t)b * nchunk + k) * o.C + ch] / unit < 16777216.0)) pre_fail(c, "stage-1 partial not exact");
        }
    }
    if (o.have_part) for (int b = 0; b < o.B; ++b) for (int k = 0; k < nchunk; ++k) for (int ch = 0; ch < o.C; ++ch) {
        const size_t s = ((size_t)b * nchunk + k) * o.C + ch;
        putv<float>(c.A.init, c.A.off[bp], ((size_t)b * nchunk + k) * 2 * o.C + ch, (float)ps[s]); putv<float>(c.A.init, c.A.off[bp], ((size_t)b * nchunk + k) * 2 * o.C + o.C + ch, (float)pq[s]);
    }
    c.A.seal();
    if (o.data != 2 && !o.have_part) for (int b = 0; b < o.B; ++b) for (int k = 0; k < nchunk; ++k) for (int ch = 0; ch < o.C; ++ch) {
        const size_t s = ((size_t)b * nchunk + k) * o.C + ch;
        putv<float>(c.A.exp, c.A.off[bp], ((size_t)b * nchunk + k) * 2 * o.C + ch, (float)ps[s]); putv<float>(c.A.exp, c.A.off[bp], ((size_t)b * nchunk + k) * 2 * o.C + o.C + ch, (float)pq[s]);
    }
    if (o.data == 2) c.A.mark_soft(bp);
    c.A.mark_soft(bs);
    // group statistics in double: one pass from the exact partials (data 0 / 1: what the kernel computes), two passes for dense data
    auto st_mean = std::make_shared<std::vector<double>>((size_t)o.B * G), st_rstd = std::make_shared<std::vector<double>>((size_t)o.B * G), st_bound = std::make_shared<std::vector<double>>((size_t)o.B * G, 0.0), st_mb = std::make_shared<std::vector<double>>((size_t)o.B * G, 0.0);
    const double n = (double)o.HW * cpg; const int L = gn_chain(o.mode, o.C);
    for (int b = 0; b < o.B; ++b) for (int g = 0; g < G; ++g) {
        double s = 0, q = 0;
        for (int k = 0; k < nchunk; ++k) for (int ci = 0; ci < cpg; ++ci) { s += ps[((size_t)b * nchunk + k) * o.C + g * cpg + ci]; q += pq[((size_t)b * nchunk + k) * o.C + g * cpg + ci]; }
        double mean = s / n, var = q / n - mean * mean;
        if (o.data == 2) { var = 0; for (int p = 0; p < o.HW; ++p) for (int ci = 0; ci < cpg; ++ci) { const double d = x[((long)b * o.HW + p) * o.C + g * cpg + ci] - mean; var += d * d; } var /= n; (*st_bound)[b * G + g] = L * std::ldexp(1.0, -24) * (q / n) / (var + o.eps); (*st_mb)[b * G + g] = (L + 1) * std::ldexp(1.0, -24) * std::sqrt(q / n); }
        if (var < 0) var = 0;
        (*st_mean)[b * G + g] = mean; (*st_rstd)[b * G + g] = 1.0 / std::sqrt(var + (double)o.eps);
        if (o.data == 1 && (mean != 0 || (*st_rstd)[b * G + g] != std::ldexp(1.0, -aexp[b * G + g] - (o.have_part ? 1 : 0)))) pre_fail(c, "sign-row statistics not exact");
    }
    // y
    auto yref = std::make_shared<std::vector<double>>();
    if (o.with_y) {
        yref->resize(nx);
        for (int b = 0; b < o.B; ++b) for (int p = 0; p < o.HW; ++p) for (int ch = 0; ch < o.C; ++ch) {
            const long i = ((long)b * o.HW + p) * o.C + ch; const int g = ch / cpg;
            const double v = (x[i] - (*st_mean)[b * G + g]) * (*st_rstd)[b * G + g] * gam[ch] + bet[ch];      // exact for sign rows: +-gamma (/2) + beta
            if (rT(o.mode, (float)v) != v) pre_fail(c, "y not exact");
            (*yref)[i] = o.swish ? silu64(v) : v;
            if (!o.swish) put(c.A.exp, c.A.off[by], i, o.mode, (float)v);
        }
        if (o.swish) c.A.mark_soft(by);
    }
    const GnOpt oo = o; Case* self = &c; const size_t ofs_s = c.A.off[bs], ofs_y = o.with_y ? c.A.off[by] : 0, ofs_p = c.A.off[bp];
    auto psum = std::make_shared<std::vector<double>>(ps), pqs = std::make_shared<std::vector<double>>(pq);
    c.soft = [=](const u8* got, std::string& msg) -> double {
        double worst = 0, wrel = 0, wbnd = 0; const int G = 32;
        for (int i = 0; i < oo.B * G; ++i) {
            const float m = getv<float>(got, ofs_s, 2 * i), r = getv<float>(got, ofs_s, 2 * i + 1);
            if (oo.data == 2) {
                // mean: the same chain on sums of magnitude <= n sqrt(q/n), plus the final rounding to float
                const double er = std::fabs(r - (*st_rstd)[i]) / (*st_rstd)[i] / (*st_bound)[i], em = std::fabs(m - (*st_mean)[i]) / (*st_mb)[i];
                worst = std::max(worst, std::max(er, em));
                wrel = std::max(wrel, std::fabs(r - (*st_rstd)[i]) / (*st_rstd)[i]); wbnd = std::max(wbnd, (*st_bound)[i]);
            } else {
                const float fm = (float)(*st_mean)[i], fr = (float)(*st_rstd)[i];
                const bool okm = m == fm || m == nextafterf(fm, -INFINITY) || m == nextafterf(fm, INFINITY), okr = r == fr || r == nextafterf(fr, -INFINITY) || r == nextafterf(fr, INFINITY);
                if (!okm || !okr) { char t[96]; snprintf(t, sizeof t, " stats[%d] got (%.9g, %.9g) expected (%.9g, %.9g)", i, m, r, fm, fr); msg = t; return 99; }
            }
        }
        if (oo.data == 2) {      // the partials themselves: L 2^-24 of the sum of magnitudes
            const double Lb = gn_chain(oo.mode, oo.C) * std::ldexp(1.0, -24);
            for (size_t k = 0; k < psum->size(); ++k) {
                const size_t bk = k / oo.C, ch = k % oo.C;
                const double gs = getv<float>(got, ofs_p, bk * 2 * oo.C + ch), gq = getv<float>(got, ofs_p, bk * 2 * oo.C + oo.C + ch);
                worst = std::max(worst, std::fabs(gq - (*pqs)[k]) / (Lb * (*pqs)[k] + 1e-30));
                worst = std::max(worst, std::fabs(gs - (*psum)[k]) / (Lb * std::sqrt(256.0 * (*pqs)[k]) + 1e-30));      // sum |x| <= sqrt(256 q)
            }
            char t[160]; snprintf(t, sizeof t, " (chain L %d; worst relative error of rstd %.2e, largest bound %.2e)", gn_chain(oo.mode, oo.C), wrel, wbnd); msg = t;
        }
        if (oo.with_y && oo.swish) {
            long nd = 0;
            for (long i = 0; i < nx; ++i) {
                const double ref = (*yref)[i]; const float g = get(got, ofs_y, i, oo.mode);
                if (oo.mode == 1) { const float e = bfv(r_bf((float)ref)); if (g != e) { ++nd; worst = std::max(worst, std::fabs((double)g - e) / ulp_bf16(ref)); } }
                else worst = std::max(worst, ref == 0 ? (g == 0 ? 0.0 : 9.0) : std::fabs(g - ref) / (std::ldexp(1.0, -22) * std::fabs(ref)));
            }
            if (oo.mode == 1) { char t[64]; snprintf(t, sizeof t, " (%ld of %ld off the rounded fp64 value)", nd, nx); msg += t; if (nd * 100 > nx) worst = std::max(worst, 9.0); }
        }
        (void)self; return worst;
    };
    c.launch = [=]() {
        Case& c = *self; const size_t xb = (size_t)nx * es;
        void* x = need(c, bx, xb); void* g = need(c, bg, (size_t)oo.C * es); void* be = need(c, bb, (size_t)oo.C * es); void* y = oo.with_y ? need(c, by, xb) : nullptr;
        float* part = (float*)need(c, bp, (size_t)oo.B * nchunk * 2 * oo.C * 4); float* stats = (float*)need(c, bs, (size_t)oo.B * 32 * 2 * 4);
        if (oo.direct_scalar) {      // gn_partial_kernel<bf16_t> at a shape the launcher gives to the vector kernel: same partials, bit for bit
            GO(hipLaunchKernelGGL(gn_partial_kernel<bf16_t>, dim3(nchunk, oo.B), dim3(256), (size_t)(2 * oo.C + 512) * 4, 0, x, part, oo.HW, oo.C));
            GO(car_launch_groupnorm_ex(oo.mode, x, g, be, y, part, stats, oo.B, oo.HW, oo.C, 32, oo.eps, oo.swish, 1, 0));
        } else GO(car_launch_groupnorm_ex(oo.mode, x, g, be, y, part, stats, oo.B, oo.HW, oo.C, 32, oo.eps, oo.swish, oo.have_part, 0));
    };
    return cp;
}
static void gn_all() {
    const int HWs[] = {1, 64, 255, 256, 257, 600}, Cs[] = {32, 64, 96, 128, 256, 320, 512};
    for (int mode = 0; mode < 2; ++mode) for (int HW : HWs) for (int C : Cs) { GnOpt o; o.mode = mode; o.HW = HW; o.C = C; o.seed = HW + C; run(*gn_case(o)); }
    for (int C : {64, 256}) { GnOpt o; o.mode = 1; o.HW = 257; o.C = C; o.direct_scalar = true; o.seed = 257 + C; run(*gn_case(o)); }      // same seed, same expected partials as the vector case above
    // stages 2 and 3 on sign rows
    for (int mode = 0; mode < 2; ++mode) for (int HW : {64, 256, 600}) for (int C : Cs) {
        GnOpt o; o.mode = mode; o.HW = HW; o.C = C; o.data = 1; o.with_y = true; o.eps = 0.f; o.seed = 3 * HW + C;
        auto a = gn_case(o); run(*a);
        if (mode == 1 && (C & (C - 1)) == 0) { o.knob = "CAR_GN_SCALAR"; auto b = gn_case(o); b->same_as = a.get(); b->same_buf = 3; b->same_exact = true; run(*b); }
        if (HW == 600 && C != 512) continue;
        o.knob = nullptr; o.swish = true; auto s = gn_case(o); run(*s);
        if (mode == 1 && (C & (C - 1)) == 0) { o.knob = "CAR_GN_SCALAR"; auto b = gn_case(o); b->same_as = s.get(); b->same_buf = 3; run(*b); }
    }
    for (int mode = 0; mode < 2; ++mode) { GnOpt o; o.mode = mode; o.HW = 257; o.C = 64; o.data = 1; o.with_y = true; o.eps = 0.f; o.seed = 77; run(*gn_case(o)); o.have_part = true; run(*gn_case(o)); }
    { GnOpt o; o.mode = 1; o.HW = 4100; o.C = 256; o.data = 1; o.with_y = true; o.eps = 0.f; o.knob = "CAR_GN_SCALAR"; o.seed = 91; run(*gn_case(o)); }      // 2 * 4100 * 256 > 8192 * 256: the stride loop runs twice
    for (double ms : {0.0, 4.0, 16.0}) for (int C : {128, 320}) { GnOpt o; o.mode = 0; o.HW = 600; o.C = C; o.data = 2; o.ms = ms; o.seed = 5; run(*gn_case(o)); }
}

// ================================================================================================================ vq_argmin
struct AmOpt { int mode = 0, cd = 8, ncode = 256; int kind = 0; unsigned seed = 1; };      // kind 0: dyadic winners, 1: dyadic ties, 2: dense
static const double AM_CAP = 0.01;
static std::shared_ptr<Case> am_case(const AmOpt& o) {
    auto cp = std::make_shared<Case>(); Case& c = *cp;
    char nm[160]; snprintf(nm, sizeof nm, "vq_argmin %s cd %d ncode %d %s", o.mode ? "bf16" : "fp32", o.cd, o.ncode, o.kind == 0 ? "dyadic winners, zero / NaN / inf rows" : o.kind == 1 ? "exact ties" : "dense vs fp64");
    c.name = nm;
    const int cd = o.cd, nc = o.ncode, es = esz(o.mode);
    std::vector<float> cb((size_t)nc * cd, 0.f), z;
    std::vector<int> tokexp;
    if (o.kind != 2) {
        std::vector<int> ax(nc), sg(nc);      // row j = sg * 2^a e_ax
        for (int j = 0; j < nc; ++j) { ax[j] = hint(j, 0, o.seed, 0, cd - 1); sg[j] = -1; }
        std::vector<int> wins;
        if (o.kind == 0) { const int cand[] = {0, 63, 64, 255, 256, 257, nc - 1}; for (int j : cand) if (j >= 0 && j < nc && std::find(wins.begin(), wins.end(), j) == wins.end()) wins.push_back(j); for (size_t i = 0; i < wins.size(); ++i) { ax[wins[i]] = (int)i; sg[wins[i]] = 1; } }
        else { const int pr[][2] = {{10, 11}, {20, 84}, {30, 286}, {300, 45}, {70, 130}, {511, 767}}; int i = 0; for (auto& p : pr) { if (p[0] < nc && p[1] < nc) { ax[p[0]] = ax[p[1]] = i; sg[p[0]] = sg[p[1]] = 1; wins.push_back(p[0]); } ++i; } }
        for (int j = 0; j < nc; ++j) cb[(size_t)j * cd + ax[j]] = std::ldexp((float)sg[j], o.kind == 1 && sg[j] > 0 ? 2 : hint(j, 1, o.seed, -3, 3));      // tie pairs: identical bits
        // pixels: +e_i for each winner axis, then -e_k for every axis, then zero, NaN, inf rows
        struct Px { int k, s, special; }; std::vector<Px> px;
        for (size_t i = 0; i < wins.size(); ++i) px.push_back({(int)i, 1, 0});
        for (int k = 0; k < cd; ++k) px.push_back({k, -1, 0});
        px.push_back({0, 0, 1}); px.push_back({0, 0, 2}); px.push_back({0, 0, 3}); px.push_back({cd - 1, 0, 3});
        z.assign(px.size() * cd, 0.f);
        for (size_t p = 0; p < px.size(); ++p) {
            int best = 0;
            if (px[p].special == 0) { z[p * cd + px[p].k] = std::ldexp((float)px[p].s, hint((unsigned)p, 2, o.seed, -3, 3)); int bd = 9; for (int j = 0; j < nc; ++j) { const int d = ax[j] != px[p].k ? 2 : (sg[j] == px[p].s ? 0 : 4); if (d < bd) { bd = d; best = j; } } }
            else if (px[p].special == 2) z[p * cd + px[p].k] = NAN;
            else if (px[p].special == 3) z[p * cd + px[p].k] = INFINITY;
            tokexp.push_back(best);      // zero row: every distance exactly 1 -> 0; NaN / inf rows: torch.argmin's 0
        }
    } else {
        for (size_t i = 0; i < cb.size(); ++i) cb[i] = (float)gauss((unsigned)i, 7, o.seed);
        z.resize((size_t)512 * cd); for (size_t i = 0; i < z.size(); ++i) z[i] = rT(o.mode, (float)gauss((unsigned)i, 8, o.seed));
    }
    const long npix = (long)z.size() / cd;
    const int bz = c.A.add(z.size() * es), bc = c.A.add(cb.size() * 4), bt = c.A.add(npix * 4);
    for (size_t i = 0; i < z.size(); ++i) put(c.A.init, c.A.off[bz], i, o.mode, z[i]);
    for (size_t i = 0; i < cb.size(); ++i) putv<float>(c.A.init, c.A.off[bc], i, cb[i]);
    c.A.seal();
    if (o.kind != 2) for (long p = 0; p < npix; ++p) putv<int>(c.A.exp, c.A.off[bt], p, tokexp[p]);
    else {
        c.A.mark_soft(bt);
        auto en = std::make_shared<std::vector<double>>(cb.size()); auto zn = std::make_shared<std::vector<double>>(z.size());
        auto dmin = std::make_shared<std::vector<double>>(npix), gap = std::make_shared<std::vector<double>>(npix); auto amin = std::make_shared<std::vector<int>>(npix);
        for (int j = 0; j < nc; ++j) { double s = 0; for (int k = 0; k < cd; ++k) s += (double)cb[(size_t)j * cd + k] * cb[(size_t)j * cd + k]; s = std::max(std::sqrt(s), 1e-12); for (int k = 0; k < cd; ++k) (*en)[(size_t)j * cd + k] = cb[(size_t)j * cd + k] / s; }
        for (long p = 0; p < npix; ++p) { double s = 0; for (int k = 0; k < cd; ++k) s += (double)z[p * cd + k] * z[p * cd + k]; s = std::max(std::sqrt(s), 1e-12); for (int k = 0; k < cd; ++k) (*zn)[p * cd + k] = z[p * cd + k] / s; }
        auto e2 = std::make_shared<std::vector<double>>(nc, 0.0), z2 = std::make_shared<std::vector<double>>(npix, 0.0);
        for (int j = 0; j < nc; ++j) for (int k = 0; k < cd; ++k) (*e2)[j] += (*en)[(size_t)j * cd + k] * (*en)[(size_t)j * cd + k];
        for (long p = 0; p < npix; ++p) for (int k = 0; k < cd; ++k) (*z2)[p] += (*zn)[p * cd + k] * (*zn)[p * cd + k];
        auto dist = [=](long p, int j) { const double* zz = &(*zn)[p * cd]; const double* ee = &(*en)[(size_t)j * cd]; double dot = 0; for (int k = 0; k < cd; ++k) dot += zz[k] * ee[k]; return (*z2)[p] + (*e2)[j] - 2 * dot; };
        const double bound = (2 * cd + 16) * std::ldexp(1.0, -23); long amb = 0;
        for (long p = 0; p < npix; ++p) {
            double d0 = 1e300, d1 = 1e300; int a0 = 0;
            for (int j = 0; j < nc; ++j) { const double d = dist(p, j); if (d < d0) { d1 = d0; d0 = d; a0 = j; } else if (d < d1) d1 = d; }
            (*dmin)[p] = d0; (*gap)[p] = d1 - d0; (*amin)[p] = a0; if (d1 - d0 <= bound) ++amb;
        }
        if (amb > AM_CAP * npix) pre_fail(c, "more than 1 % of the pixels ambiguous in the fp64 reference");
        const size_t ot = c.A.off[bt];
        c.soft = [=](const u8* got, std::string& msg) -> double {
            double worst = 0; long na = 0;
            for (long p = 0; p < npix; ++p) {
                const int t = getv<int>(got, ot, p);
                if (t < 0 || t >= nc) { msg = " token out of range"; return 99; }
                const double d = dist(p, t) - (*dmin)[p];
                worst = std::max(worst, d / bound);
                if ((*gap)[p] > bound) { if (t != (*amin)[p]) { msg = " unambiguous pixel off the fp64 argmin"; return 99; } } else ++na;
            }
            char s[64]; snprintf(s, sizeof s, " (%ld of %ld pixels ambiguous)", na, npix); msg = s;
            return worst;
        };
    }
    Case* self = &c; const AmOpt oo = o; if (cd > 16) pre_fail(c, "cd > 16");
    c.launch = [=]() { Case& c = *self; GO(car_launch_vq_argmin(oo.mode, need(c, bz, (size_t)npix * cd * es), (const float*)need(c, bc, (size_t)nc * cd * 4), (int*)need(c, bt, (size_t)npix * 4), npix, cd, nc, 0)); };
    return cp;
}
static void am_all() {
    for (int mode = 0; mode < 2; ++mode) for (int cd : {8, 16}) {
        for (int nc : {1, 5, 64, 255, 256, 257, 1000, 16384}) { AmOpt o; o.mode = mode; o.cd = cd; o.ncode = nc; o.seed = nc + cd; run(*am_case(o)); }
        AmOpt t; t.mode = mode; t.cd = cd; t.ncode = 1000; t.kind = 1; t.seed = 5; run(*am_case(t));
    }
    const int dn[][2] = {{16384, 8}, {1000, 8}, {257, 16}, {16384, 16}};
    for (auto& d : dn) { AmOpt o; o.kind = 2; o.ncode = d[0]; o.cd = d[1]; o.seed = 11; run(*am_case(o)); }
    { AmOpt o; o.kind = 2; o.mode = 1; o.ncode = 1000; o.cd = 8; o.seed = 12; run(*am_case(o)); }
}

// ================================================================================================================ vq_lookup
static void lookup_case(int mode, long npix, int cd, int zc, int ncode, int kind) {      // kind 0: dyadic (memcmp), 1: rows of norm 5, 2: dense
    Case c; char nm[160]; snprintf(nm, sizeof nm, "vq_lookup %s npix %ld cd %d zc %d ncode %d %s", mode ? "bf16" : "fp32", npix, cd, zc, ncode, kind == 0 ? "dyadic, clamped tokens" : kind == 1 ? "norm-5 rows" : "dense vs fp64"); c.name = nm;
    const int es = esz(mode);
    const int bt = c.A.add(npix * 4), bc = c.A.add((size_t)ncode * cd * 4), bw = c.A.add((size_t)zc * cd * 4), bb = c.A.add((size_t)zc * 4), bz = c.A.add((size_t)npix * zc * es);
    std::vector<float> cb((size_t)ncode * cd, 0.f), w((size_t)zc * cd), b(zc); std::vector<int> tok(npix);
    for (int j = 0; j < ncode; ++j) {
        if (kind == 0) cb[(size_t)j * cd + hint(j, 0, 3, 0, cd - 1)] = std::ldexp((hsh(j, 1, 3) & 1) ? -1.f : 1.f, hint(j, 2, 3, -3, 3));
        else if (kind == 1) { const int k0 = hint(j, 0, 4, 0, cd - 1), k1 = (k0 + 1 + hint(j, 1, 4, 0, cd - 2)) % cd; cb[(size_t)j * cd + k0] = (hsh(j, 2, 4) & 1) ? -3.f : 3.f; cb[(size_t)j * cd + k1] = (hsh(j, 3, 4) & 1) ? -4.f : 4.f; }
        else for (int k = 0; k < cd; ++k) cb[(size_t)j * cd + k] = (float)gauss(j, k, 5);
    }
    for (int i = 0; i < zc * cd; ++i) w[i] = kind == 2 ? (float)gauss(i, 1, 6) : (float)hint(i, 0, 6, -4, 4);
    for (int i = 0; i < zc; ++i) b[i] = kind == 2 ? (float)gauss(i, 2, 6) : (float)hint(i, 1, 6, -8, 8);
    const int special[] = {-1, 0, ncode - 1, ncode, INT_MAX, INT_MIN};
    for (long p = 0; p < npix; ++p) tok[p] = p < 6 ? special[p] : hint((unsigned)p, 0, 7, 0, ncode - 1);
    for (long p = 0; p < npix; ++p) putv<int>(c.A.init, c.A.off[bt], p, tok[p]);
    for (size_t i = 0; i < cb.size(); ++i) putv<float>(c.A.init, c.A.off[bc], i, cb[i]);
    for (size_t i = 0; i < w.size(); ++i) putv<float>(c.A.init, c.A.off[bw], i, w[i]);
    for (int i = 0; i < zc; ++i) putv<float>(c.A.init, c.A.off[bb], i, b[i]);
    c.A.seal();
    auto ref = std::make_shared<std::vector<double>>((size_t)npix * zc), bnd = std::make_shared<std::vector<double>>((size_t)npix * zc);
    for (long p = 0; p < npix; ++p) {
        const int t = tok[p] < 0 ? 0 : (tok[p] >= ncode ? ncode - 1 : tok[p]); const float* e = &cb[(size_t)t * cd];
        double nn = 0; for (int k = 0; k < cd; ++k) nn += (double)e[k] * e[k]; const double nrm = std::max(std::sqrt(nn), 1e-12);
        for (int ch = 0; ch < zc; ++ch) {
            double a = 0, m = 0; for (int k = 0; k < cd; ++k) { a += w[ch * cd + k] * (e[k] / nrm); m += std::fabs(w[ch * cd + k] * (e[k] / nrm)); }
            const double v = a + b[ch]; (*ref)[p * zc + ch] = v; (*bnd)[p * zc + ch] = (cd + 5) * std::ldexp(1.0, -24) * (m + std::fabs(b[ch])) + (mode == 1 ? 0.5 * ulp_bf16(v) * 1.0000001 : 0.0);
            if (kind == 0) { if (rT(mode, (float)v) != v) pre_fail(c, "dyadic result not exact"); put(c.A.exp, c.A.off[bz], p * zc + ch, mode, (float)v); }
        }
    }
    if (kind != 0) {
        c.A.mark_soft(bz); const size_t oz = c.A.off[bz];
        c.soft = [=](const u8* got, std::string&) -> double { double worst = 0; for (size_t i = 0; i < ref->size(); ++i) worst = std::max(worst, std::fabs(get(got, oz, i, mode) - (*ref)[i]) / (*bnd)[i]); return worst; };
    }
    Case* self = &c;
    c.launch = [=]() { Case& c = *self; GO(car_launch_vq_lookup(mode, (const int*)need(c, bt, npix * 4), (const float*)need(c, bc, (size_t)ncode * cd * 4), (const float*)need(c, bw, (size_t)zc * cd * 4), (const float*)need(c, bb, (size_t)zc * 4), need(c, bz, (size_t)npix * zc * es), npix, cd, zc, ncode, 0)); };
    run(c);
}
static void lookup_all() {
    for (int mode = 0; mode < 2; ++mode) {
        for (int cd : {8, 16}) { lookup_case(mode, 70, cd, 24, 100, 0); lookup_case(mode, 70, cd, 24, 100, 1); lookup_case(mode, 70, cd, 24, 100, 2); }
        lookup_case(mode, 4100, 8, 256, 16384, 0);      // 4100 * 256 > 4096 * 256: the stride loop runs twice
    }
}

// ================================================================================================================ conv_out, conv_in3
static void conv_out_case(int mode, int C, int H, int W, bool direct_scalar) {
    Case c; char nm[160]; snprintf(nm, sizeof nm, "conv_out %s C %d %dx%d%s", mode ? "bf16" : "fp32", C, H, W, direct_scalar ? " conv_out_kernel<bf16> direct (== MFMA form)" : (mode == 1 && C % 32 == 0 && C <= 256 ? " (MFMA form)" : " (scalar form)")); c.name = nm;
    const int B = 2, es = esz(mode); const long npix = (long)B * H * W;
    if (C % (mode == 1 ? 8 : 4)) pre_fail(c, "C outside the documented domain");
    const int bx = c.A.add(npix * C * es), bw = c.A.add((size_t)27 * C * es), bb = c.A.add(12), bo = c.A.add(npix * 3 * 4);
    std::vector<int> x(npix * C), w(27 * C); const int bias[3] = {5, -7, 11};
    for (long i = 0; i < npix * C; ++i) x[i] = hint((unsigned)(i / C), (unsigned)(i % C), 21, -2, 2);
    for (int i = 0; i < 27 * C; ++i) w[i] = hint(i / C, i % C, 22 + C, -2, 2);
    for (long i = 0; i < npix * C; ++i) put(c.A.init, c.A.off[bx], i, mode, (float)x[i]);
    for (int i = 0; i < 27 * C; ++i) put(c.A.init, c.A.off[bw], i, mode, (float)w[i]);
    for (int o = 0; o < 3; ++o) putv<float>(c.A.init, c.A.off[bb], o, (float)bias[o]);
    c.A.seal();
    for (int b = 0; b < B; ++b) for (int y = 0; y < H; ++y) for (int xx = 0; xx < W; ++xx) for (int o = 0; o < 3; ++o) {
        long acc = 0, mag = 0;
        for (int tap = 0; tap < 9; ++tap) { const int yy = y + tap / 3 - 1, xq = xx + tap % 3 - 1; if (yy < 0 || yy >= H || xq < 0 || xq >= W) continue;
            const int* px = &x[(((long)b * H + yy) * W + xq) * C]; const int* ww = &w[(o * 9 + tap) * C]; for (int ch = 0; ch < C; ++ch) { acc += px[ch] * ww[ch]; mag += std::abs(px[ch] * ww[ch]); } }
        if (mag + 16 >= (1 << 24)) pre_fail(c, "sum beyond 2^24");
        putv<float>(c.A.exp, c.A.off[bo], ((long)b * 3 + o) * H * W + (long)y * W + xx, (float)(acc + bias[o]));
    }
    Case* self = &c;
    c.launch = [=]() { Case& c = *self; void* x = need(c, bx, npix * C * es); void* w = need(c, bw, (size_t)27 * C * es); const float* bi = (const float*)need(c, bb, 12); float* out = (float*)need(c, bo, npix * 3 * 4);
        if (direct_scalar) GO(hipLaunchKernelGGL(conv_out_kernel<bf16_t>, dim3((npix + 255) / 256), dim3(256), (size_t)27 * C * 4, 0, x, w, bi, out, B, H, W, C));
        else GO(car_launch_conv_out(mode, x, w, bi, out, B, H, W, C, 0)); };
    run(c);
}
static void conv_in3_case(int mode, int Co, int H, int W) {
    Case c; char nm[120]; snprintf(nm, sizeof nm, "conv_in3 %s Co %d %dx%d (257 -> 256, 259 -> 260 in bf16)", mode ? "bf16" : "fp32", Co, H, W); c.name = nm;
    const int B = 2, es = esz(mode); const long npix = (long)B * H * W;
    const int bi = c.A.add(npix * 3 * 4), bw = c.A.add((size_t)Co * 27 * es), bb = c.A.add((size_t)Co * es), bo = c.A.add(npix * Co * es);
    std::vector<float> img(npix * 3); std::vector<int> w(Co * 27), bs(Co);
    for (long i = 0; i < npix * 3; ++i) { const unsigned h = hsh((unsigned)i, 0, 31); img[i] = h % 37 == 0 ? 257.f : h % 37 == 1 ? 259.f : h % 37 == 2 ? -257.f : (float)((int)(h % 9) - 4); }
    for (int i = 0; i < Co * 27; ++i) w[i] = hint(i / 27, i % 27, 32, -2, 2);
    for (int i = 0; i < Co; ++i) bs[i] = hint(i, 0, 33, -6, 6);
    for (long i = 0; i < npix * 3; ++i) putv<float>(c.A.init, c.A.off[bi], i, img[i]);
    for (int i = 0; i < Co * 27; ++i) put(c.A.init, c.A.off[bw], i, mode, (float)w[i]);
    for (int i = 0; i < Co; ++i) put(c.A.init, c.A.off[bb], i, mode, (float)bs[i]);
    c.A.seal();
    for (int b = 0; b < B; ++b) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) for (int co = 0; co < Co; ++co) {
        long acc = 0;
        for (int ci = 0; ci < 3; ++ci) for (int t = 0; t < 9; ++t) { const int yy = y + t / 3 - 1, xx = x + t % 3 - 1; if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            acc += (long)rT(mode, img[(((long)b * 3 + ci) * H + yy) * W + xx]) * w[co * 27 + ci * 9 + t]; }
        put(c.A.exp, c.A.off[bo], (((long)b * H + y) * W + x) * Co + co, mode, (float)(acc + bs[co]));      // |sum| < 2^24: exact; one rounding at the store
    }
    Case* self = &c;
    c.launch = [=]() { Case& c = *self; GO(car_launch_conv_in3(mode, (const float*)need(c, bi, npix * 3 * 4), need(c, bw, (size_t)Co * 27 * es), need(c, bb, (size_t)Co * es), need(c, bo, npix * Co * es), B, H, W, Co, 0)); };
    run(c);
}
static void conv_all() {
    const int shp[][2] = {{1, 1}, {5, 7}, {16, 16}, {17, 33}, {31, 16}};
    for (auto& s : shp) { for (int C : {32, 64, 128, 256, 8, 288, 512}) conv_out_case(1, C, s[0], s[1], false); for (int C : {4, 128}) conv_out_case(0, C, s[0], s[1], false); }
    conv_out_case(1, 32, 17, 33, true); conv_out_case(1, 256, 17, 33, true);
    for (int mode = 0; mode < 2; ++mode) for (int Co : {1, 5, 128}) { conv_in3_case(mode, Co, 5, 7); conv_in3_case(mode, Co, 17, 19); }
}

// ================================================================================================================ rmsnorm_kernel
struct RmOpt { int mode = 1, D = 64, rows = 3; bool gather = false, hout = true, xn = true, sign = false; int add_mode = 0; float cs = 1.f; int ks = 0; float eps = 1e-5f; };
static void rms_case(const RmOpt& o) {
    Case c; char nm[200]; snprintf(nm, sizeof nm, "rmsnorm %s D %d rows %d%s%s%s%s add_mode %d cs %g parts_ks %d eps %g", o.mode ? "bf16" : "fp32", o.D, o.rows, o.sign ? " sign rows" : " integer rows", o.gather ? " gather" : "",
                                    o.hout ? "" : " no h_out", o.xn ? "" : " xn == nullptr", o.add_mode, o.cs, o.ks, o.eps); c.name = nm;
    const int D = o.D, rows = o.rows, es = esz(o.mode), T = 3, n_tok = 5, row0 = 1, pos = 6, nemb = 7;
    if (D % 4 || D > 16 * 1024) pre_fail(c, "D outside the documented domain");
    if (o.add_mode >= 2 && rows % T) pre_fail(c, "rows % T");
    const long pstride = (long)rows * D + 64;
    long nctrl = 0;
    if (o.add_mode == 1) nctrl = ((long)(rows - 1) * n_tok + (pos - T + 1) + 1) * D; else if (o.add_mode == 2) nctrl = ((long)((rows - 1) / T) * n_tok + 1) * D; else if (o.add_mode == 3) nctrl = ((long)((rows - 1) / T) * n_tok + (T - 1 - row0) + 1) * D;
    const int bh = c.A.add((size_t)(o.gather ? nemb : rows) * D * es), bi = o.gather ? c.A.add(rows * 4) : -1, bw = c.A.add((size_t)D * es), bho = o.hout ? c.A.add((size_t)rows * D * es) : -1, bxn = o.xn ? c.A.add((size_t)rows * D * es) : -1;
    const int bc = o.add_mode ? c.A.add((size_t)nctrl * es) : -1, bp = o.add_mode == 1 ? c.A.add(4) : -1, bpa = o.ks ? c.A.add((size_t)((o.ks - 1) * pstride + (long)rows * D) * 4) : -1;
    std::vector<int> idx(rows); for (int r = 0; r < rows; ++r) idx[r] = o.gather ? (r * 3 + 5) % nemb : r;
    const int nsrc = o.gather ? nemb : rows;
    std::vector<float> src((size_t)nsrc * D), w(D), ctrl(nctrl), parts;
    for (int r = 0; r < nsrc; ++r) for (int d = 0; d < D; ++d) src[(size_t)r * D + d] = o.sign ? std::ldexp((hsh(r, d, 41) & 1) ? -1.f : 1.f, hint(r, 0, 42, 0, 3)) : (float)hint(r, d, 43, -8, 8);
    for (int d = 0; d < D; ++d) w[d] = (float)hint(d, 0, 44, -5, 5);
    const bool dyadic = o.cs == 0.5f || o.cs == 1.f || o.cs == 2.f;
    for (long i = 0; i < nctrl; ++i) ctrl[i] = dyadic ? (float)hint((unsigned)i, 0, 45, -4, 4) : ((hsh((unsigned)i, 1, 45) & 1) ? -4.f : 4.f);
    if (o.ks) { parts.assign((size_t)((o.ks - 1) * pstride + (long)rows * D), 0.f); for (int s = 0; s < o.ks; ++s) for (long i = 0; i < (long)rows * D; ++i) parts[s * pstride + i] = (float)hint((unsigned)i, s, 46, -2, 2); }
    if (o.mode == 0 && o.add_mode && !dyadic) pre_fail(c, "fp32 mode takes dyadic cs only");
    for (size_t i = 0; i < src.size(); ++i) put(c.A.init, c.A.off[bh], i, o.mode, src[i]);
    for (int d = 0; d < D; ++d) put(c.A.init, c.A.off[bw], d, o.mode, w[d]);
    if (o.gather) for (int r = 0; r < rows; ++r) putv<int>(c.A.init, c.A.off[bi], r, idx[r]);
    for (long i = 0; i < nctrl; ++i) put(c.A.init, c.A.off[bc], i, o.mode, ctrl[i]);
    if (bp >= 0) putv<int>(c.A.init, c.A.off[bp], 0, pos);
    if (o.ks) { for (size_t i = 0; i < parts.size(); ++i) putv<float>(c.A.init, c.A.off[bpa], i, 1e30f); for (int s = 0; s < o.ks; ++s) for (long i = 0; i < (long)rows * D; ++i) putv<float>(c.A.init, c.A.off[bpa], s * pstride + i, parts[s * pstride + i]); }      // the gap between slices holds 1e30
    c.A.seal();
    auto cand = std::make_shared<std::vector<float>>((size_t)rows * 3 * D);      // the three candidate xn rows
    for (int r = 0; r < rows; ++r) {
        std::vector<float> v(D); std::vector<double> sq(D);
        long arow = -1;
        if (o.add_mode == 1) arow = (long)r * n_tok + (pos - T + 1); else if (o.add_mode == 2 && r % T == T - 1) arow = (long)(r / T) * n_tok; else if (o.add_mode == 3 && r % T >= row0) arow = (long)(r / T) * n_tok + (r % T - row0);
        for (int d = 0; d < D; ++d) {
            float x = src[(size_t)idx[r] * D + d];
            if (o.ks) { float a = 0.f; for (int s = 0; s < o.ks; ++s) a = fadd(a, parts[s * pstride + (long)r * D + d]); x = rT(o.mode, fadd(x, rT(o.mode, a))); }      // integers: every order gives this sum
            if (arow >= 0) x = rT(o.mode, fadd(x, rT(o.mode, fmul(o.cs, rT(o.mode, ctrl[arow * D + d])))));
            v[d] = x; sq[d] = (double)x * x;
            if (o.hout) put(c.A.exp, c.A.off[bho], (size_t)r * D + d, o.mode, x);
        }
        if (!exact_sum_ok(sq)) pre_fail(c, "sum of squares not exact in fp32");
        double ss = 0; for (double t : sq) ss += t;
        const float m2 = fadd(fdiv((float)ss, (float)D), o.eps), rc = (float)(1.0 / std::sqrt((double)m2));
        const float rs[3] = {nextafterf(rc, 0.f), rc, nextafterf(rc, INFINITY)};
        for (int k = 0; k < 3; ++k) for (int d = 0; d < D; ++d) (*cand)[((size_t)r * 3 + k) * D + d] = rT(o.mode, fmul(rT(o.mode, fmul(v[d], rs[k])), w[d]));
        if (o.sign && o.mode == 1 && !o.ks && !o.add_mode) {      // the sign-row claim: rnd(v rstd) = +-1 within 2 ulp of rstd
            const float r2[2] = {nextafterf(rs[0], 0.f), nextafterf(rs[2], INFINITY)};
            for (float q : r2) for (int d = 0; d < D; ++d) if (std::fabs(rT(1, fmul(v[d], q))) != 1.f) pre_fail(c, "sign row: rnd(v rstd) != +-1");
            for (int k = 0; k < 3; k += 2) if (memcmp(&(*cand)[((size_t)r * 3 + k) * D], &(*cand)[((size_t)r * 3 + 1) * D], D * 4) != 0) pre_fail(c, "sign row: candidates differ");
        }
    }
    if (o.xn) {
        c.A.mark_soft(bxn); const size_t ox = c.A.off[bxn]; const int mode = o.mode;
        c.soft = [=](const u8* got, std::string& msg) -> double {
            for (int r = 0; r < rows; ++r) { bool any = false;
                for (int k = 0; k < 3 && !any; ++k) { bool eq = true; for (int d = 0; d < D && eq; ++d) { const float e = (*cand)[((size_t)r * 3 + k) * D + d], g = get(got, ox, (size_t)r * D + d, mode); eq = memcmp(&e, &g, 4) == 0; } any = eq; }
                if (!any) { char t[64]; snprintf(t, sizeof t, " row %d equals none of the three candidates", r); msg = t; return 99; } }
            return 0;
        };
    }
    Case* self = &c; const RmOpt oo = o;
    c.launch = [=]() { Case& c = *self; NormP p; memset(&p, 0, sizeof p);
        const size_t rb = (size_t)rows * D * es;
        if (oo.gather) { int mx = 0; for (int r = 0; r < rows; ++r) mx = std::max(mx, idx[r]); p.emb = need(c, bh, (size_t)(mx + 1) * D * es); p.idx = (const int*)need(c, bi, rows * 4); } else p.h_in = need(c, bh, rb);
        p.h_out = oo.hout ? need(c, bho, rb) : nullptr; p.xn = oo.xn ? need(c, bxn, rb) : nullptr; p.w = need(c, bw, (size_t)D * es);
        if (oo.add_mode) p.ctrl = need(c, bc, (size_t)nctrl * es); if (oo.add_mode == 1) p.pos = (const int*)need(c, bp, 4);
        p.add_mode = oo.add_mode; p.T = T; p.n_tok = n_tok; p.cs = oo.cs; p.D = D; p.eps = oo.eps; p.row0 = row0;
        if (oo.ks) { p.parts = (const float*)need(c, bpa, (size_t)((oo.ks - 1) * pstride + (long)rows * D) * 4); p.parts_ks = oo.ks; p.parts_stride = pstride; }
        GO(car_launch_rmsnorm(oo.mode, &p, rows, 0)); };
    run(c);
}
static void rms_all() {
    for (int D : {64, 252, 260, 768, 1280, 2048, 4096, 4100, 8192}) {
        for (float eps : {1e-5f, 0.f}) { RmOpt o; o.D = D; o.sign = true; o.eps = eps; o.gather = D == 260 || D == 4100; o.hout = D != 768; rms_case(o); }
        for (int mode = 0; mode < 2; ++mode) { RmOpt o; o.mode = mode; o.D = D; o.gather = D == 252 || D == 8192; rms_case(o); }
    }
    for (int mode = 0; mode < 2; ++mode) for (int D : {260, 4100}) {
        for (int am = 1; am <= 3; ++am) { RmOpt o; o.mode = mode; o.D = D; o.rows = 6; o.add_mode = am; o.cs = 0.5f; o.hout = am != 2; rms_case(o); }
        if (mode == 1 && D == 260) for (int am = 1; am <= 3; ++am) { RmOpt o; o.D = 64; o.rows = 6; o.add_mode = am; o.cs = 0.7f; rms_case(o); }      // non-dyadic cs: rnd(cs c) and rnd(v + .) really round; D = 64 keeps the squares exact
        for (int ks : {1, 3, 4, 5, 8, 9}) { RmOpt o; o.mode = mode; o.D = D; o.ks = ks; o.add_mode = ks == 5 ? 3 : 0; o.rows = ks == 5 ? 6 : 3; o.cs = 0.5f; o.gather = ks == 9; rms_case(o); }
        { RmOpt o; o.mode = mode; o.D = D; o.rows = 6; o.xn = false; o.add_mode = 3; o.cs = 0.5f; o.ks = 3; o.gather = true; rms_case(o); }
    }
}

// ================================================================================================================ layernorm_kernel
static void ln_case(int mode, int D, int rows, bool sign) {
    Case c; char nm[120]; snprintf(nm, sizeof nm, "layernorm %s D %d rows %d %s", mode ? "bf16" : "fp32", D, rows, sign ? "sign rows around an integer centre" : "dense vs fp64"); c.name = nm;
    const int es = esz(mode); const float eps = 1e-6f;
    if (sign && D != 1 && D % 2) pre_fail(c, "sign rows need an even D");
    const int bx = c.A.add((size_t)rows * D * es), bw = c.A.add((size_t)D * es), bb = c.A.add((size_t)D * es), by = c.A.add((size_t)rows * D * es);
    std::vector<float> x((size_t)rows * D), w(D), b(D);
    for (int r = 0; r < rows; ++r) { const int ce = hint(r, 0, 51 + D, -4, 4), a = hint(r, 1, 51 + D, 0, 2);
        for (int d = 0; d < D; ++d) x[(size_t)r * D + d] = sign ? (D == 1 ? (float)ce : (float)ce + std::ldexp(((hsh(r, d >> 1, 52) & 1) ^ (d & 1)) ? -1.f : 1.f, a)) : rT(mode, (float)(0.5 * r + gauss(r, d, 53))); }
    for (int d = 0; d < D; ++d) { w[d] = sign ? (float)hint(d, 0, 54, -3, 3) : rT(mode, (float)(1 + 0.3 * gauss(d, 0, 55))); b[d] = sign ? (float)(hint(d, 1, 54, 4, 8) * ((hsh(d, 2, 54) & 1) ? -1 : 1)) : rT(mode, (float)(0.3 * gauss(d, 1, 55))); }
    for (size_t i = 0; i < x.size(); ++i) put(c.A.init, c.A.off[bx], i, mode, x[i]);
    for (int d = 0; d < D; ++d) { put(c.A.init, c.A.off[bw], d, mode, w[d]); put(c.A.init, c.A.off[bb], d, mode, b[d]); }
    c.A.seal();
    auto ref = std::make_shared<std::vector<double>>((size_t)rows * D), bnd = std::make_shared<std::vector<double>>((size_t)rows * D);
    const double L = (D + 127) / 128 + 8, u = std::ldexp(1.0, -24);
    for (int r = 0; r < rows; ++r) {
        double mean = 0, var = 0, ma = 0; for (int d = 0; d < D; ++d) { mean += x[(size_t)r * D + d]; ma += std::fabs(x[(size_t)r * D + d]); } mean /= D; ma /= D;
        for (int d = 0; d < D; ++d) { const double t = x[(size_t)r * D + d] - mean; var += t * t; } var /= D; const double rstd = 1.0 / std::sqrt(var + eps);
        for (int d = 0; d < D; ++d) {
            const double dd = x[(size_t)r * D + d] - mean, y = dd * rstd * w[d] + b[d]; (*ref)[(size_t)r * D + d] = y;
            (*bnd)[(size_t)r * D + d] = sign ? 4 * u * std::fabs(w[d]) + u * std::fabs(y) + 1e-30 : (L + 8) * u * std::fabs(w[d]) * rstd * (std::fabs(dd) + ma) + u * std::fabs(y) + (mode == 1 ? 0.5 * ulp_bf16(y) * 1.0000001 : 0.0) + 1e-30;
            if (sign && mode == 1) { const double yi = D == 1 ? b[d] : (dd > 0 ? 1 : -1) * w[d] + b[d]; put(c.A.exp, c.A.off[by], (size_t)r * D + d, 1, (float)yi); }
        }
    }
    if (!(sign && mode == 1)) { c.A.mark_soft(by); const size_t oy = c.A.off[by];
        c.soft = [=](const u8* got, std::string&) -> double { double worst = 0; for (size_t i = 0; i < ref->size(); ++i) worst = std::max(worst, std::fabs(get(got, oy, i, mode) - (*ref)[i]) / (*bnd)[i]); return worst; }; }
    Case* self = &c;
    c.launch = [=]() { Case& c = *self; GO(car_launch_layernorm(mode, need(c, bx, (size_t)rows * D * es), need(c, bw, (size_t)D * es), need(c, bb, (size_t)D * es), need(c, by, (size_t)rows * D * es), rows, D, eps, 0)); };
    run(c);
}
static void ln_all() {
    for (int mode = 0; mode < 2; ++mode) for (int rows : {1, 3}) for (int D : {1, 64, 127, 128, 129, 384, 1024, 1280}) { if (D == 1 || D % 2 == 0) ln_case(mode, D, rows, true); if (D > 1) ln_case(mode, D, rows, false); }
}

// ================================================================================================================ swiglu, swiglu_parts, t5_gated_act
// which 0: swiglu, 1: t5_gated_act, 2: swiglu_parts (bf16 output)
static void glu_case(int which, int mode, long rows, int hidden, int ks, bool dense) {
    Case c; char nm[160]; snprintf(nm, sizeof nm, "%s %s rows %ld hidden %d%s %s", which == 0 ? "swiglu" : which == 1 ? "t5_gated_act" : "swiglu_parts", mode ? "bf16" : "fp32", rows, hidden, which == 2 ? (" ks " + std::to_string(ks)).c_str() : "",
                                    dense ? "dense pre-activations" : "integer gates in [24, 60] (layout, no tolerance)"); c.name = nm;
    const bool gelu = which == 1; const int es = esz(mode); const long nin = rows * 2 * hidden, nout = rows * hidden, stride = nin + 32;
    if (which == 2 && (hidden % 8 || mode != 1)) pre_fail(c, "swiglu_parts domain"); if (hidden % 16) pre_fail(c, "hidden % 16");
    const int bi = which == 2 ? c.A.add((size_t)((ks - 1) * stride + nin) * 4) : c.A.add((size_t)nin * es), bo = c.A.add((size_t)nout * es);
    std::vector<float> a(nout), g(nout);
    for (long i = 0; i < nout; ++i) {
        if (!dense) { a[i] = (float)(24 + (int)(hsh((unsigned)i, 0, 61) % 37u)); g[i] = (float)hint((unsigned)i, 1, 61, -4, 4); }
        else { const int lo = gelu ? -28 : -244; a[i] = (float)hint((unsigned)i, 0, 62, lo, 244) / 8.f; g[i] = (float)hint((unsigned)i, 1, 62, -64, 64) / 16.f; }
    }
    auto col = [&](long i) { const long r = i / hidden; const int ch = (int)(i % hidden); return r * 2 * hidden + (ch >> 4) * 32 + (ch & 15); };
    if (which == 2) {
        for (size_t i = 0; i < (size_t)((ks - 1) * stride + nin); ++i) putv<float>(c.A.init, c.A.off[bi], i, 1e30f);
        for (long i = 0; i < nout; ++i) {      // split a and g into ks addends of the same unit (integers, or eighths / sixteenths): every partial sum is exact
            const float ua = dense ? 0.125f : 1.f, ug = dense ? 0.0625f : 1.f; int ra = (int)(a[i] / ua), rg = (int)(g[i] / ug);
            for (int s = 0; s < ks; ++s) { const int pa = s == ks - 1 ? ra : hint((unsigned)i, s, 63, -3, 3), pg = s == ks - 1 ? rg : hint((unsigned)i, s, 64, -3, 3); ra -= pa; rg -= pg;
                putv<float>(c.A.init, c.A.off[bi], s * stride + col(i), pa * ua); putv<float>(c.A.init, c.A.off[bi], s * stride + col(i) + 16, pg * ug); }
        }
    } else for (long i = 0; i < nout; ++i) { put(c.A.init, c.A.off[bi], col(i), mode, a[i]); put(c.A.init, c.A.off[bi], col(i) + 16, mode, g[i]); }
    c.A.seal();
    auto ref = std::make_shared<std::vector<double>>(), bnd = std::make_shared<std::vector<double>>(); auto expb = std::make_shared<std::vector<float>>();
    for (long i = 0; i < nout; ++i) {
        const double f = gelu ? gelu64(a[i]) : silu64(a[i]);
        if (!dense) { if (std::fabs(f / a[i] - 1.0) >= std::ldexp(1.0, -30)) pre_fail(c, "gate not saturated"); const float v = a[i] * g[i]; if (rT(mode, v) != v) pre_fail(c, "a g not exact"); put(c.A.exp, c.A.off[bo], i, mode, v); continue; }
        if (mode == 1) { const float gt = bfv(r_bf((float)f)); const float o = bfv(r_bf(gt * g[i])); expb->push_back(o); bnd->push_back(ulp_bf16(f) * std::fabs(g[i]) + ulp_bf16(o)); ref->push_back(o); }
        else { const double r = f * g[i]; ref->push_back(r); bnd->push_back(gelu ? 10 * std::ldexp(1.0, -24) * std::fabs(0.5 * a[i] * g[i]) + 4 * std::ldexp(1.0, -24) * std::fabs(r) + 1e-30 : 5 * std::ldexp(1.0, -24) * std::fabs(r) + 1e-30); }
    }
    if (dense) { c.A.mark_soft(bo); const size_t oo = c.A.off[bo];
        c.soft = [=](const u8* got, std::string& msg) -> double { double worst = 0; long nd = 0;
            for (long i = 0; i < nout; ++i) { const double gv = get(got, oo, i, mode), d = std::fabs(gv - (*ref)[i]); if (mode == 1) { if (d != 0) { ++nd; worst = std::max(worst, d / (*bnd)[i]); } } else worst = std::max(worst, d / (*bnd)[i]); }
            if (mode == 1) { char t[64]; snprintf(t, sizeof t, " (%ld of %ld off the rounded fp64 value)", nd, nout); msg = t; if (nd * 100 > nout) worst = std::max(worst, 9.0); }
            return worst; }; }
    Case* self = &c;
    c.launch = [=]() { Case& c = *self;
        if (which == 2) GO(car_launch_swiglu_parts((const float*)need(c, bi, (size_t)((ks - 1) * stride + nin) * 4), ks, stride, need(c, bo, (size_t)nout * 2), (int)rows, hidden, 0));
        else if (which == 1) GO(car_launch_t5_gated_act(mode, need(c, bi, (size_t)nin * es), need(c, bo, (size_t)nout * es), rows, hidden, 0));
        else GO(car_launch_swiglu(mode, need(c, bi, (size_t)nin * es), need(c, bo, (size_t)nout * es), rows, hidden, 0)); };
    run(c);
}
static void glu_all() {
    for (int which = 0; which < 2; ++which) for (int mode = 0; mode < 2; ++mode) { for (int h : {16, 48, 4096}) glu_case(which, mode, 3, h, 0, false); glu_case(which, mode, 3, 4096, 0, true); }
    glu_case(0, 1, 257, 4096, 0, false); glu_case(1, 0, 257, 4096, 0, false);      // 257 * 4096 > 4096 * 256: past the grid cap
    for (int ks : {1, 2, 5}) for (int h : {16, 48, 4096}) glu_case(2, 1, 3, h, ks, false);
    glu_case(2, 1, 3, 4096, 5, true); glu_case(2, 1, 40, 4096, 2, false);
}

// ================================================================================================================ copies and index kernels
static void convert_case(int mode, int src_dtype) {
    Case c; char nm[120]; snprintf(nm, sizeof nm, "convert %s -> %s, every bf16 pattern%s", src_dtype ? "bf16" : "fp32", mode ? "bf16" : "fp32", src_dtype ? "" : " x 17 low halves: ties, NaN, inf, 3.4e38, denormals; past the grid cap"); c.name = nm;
    const unsigned lows[17] = {0, 1, 0x7fff, 0x8000, 0x8001, 0xffff, 0x4000, 0xc000, 0x7ffe, 0x8002, 0x1234, 0xfedc, 0x00ff, 0xff00, 0x5555, 0xaaaa, 0x8080};
    const long n = src_dtype ? 65536 : 65536L * 17;
    const int bs = c.A.add((size_t)n * (src_dtype ? 2 : 4)), bd = c.A.add((size_t)n * esz(mode));
    for (long i = 0; i < n; ++i) { if (src_dtype) putv<uint16_t>(c.A.init, c.A.off[bs], i, (uint16_t)i); else putv<uint32_t>(c.A.init, c.A.off[bs], i, ((uint32_t)(i & 0xffff) << 16) | lows[i >> 16]); }
    c.A.seal();
    for (long i = 0; i < n; ++i) {
        const float v = src_dtype ? bfv((uint16_t)i) : getv<float>(c.A.init.data(), c.A.off[bs], i);
        if (mode == 1) putv<uint16_t>(c.A.exp, c.A.off[bd], i, r_bf(v)); else putv<float>(c.A.exp, c.A.off[bd], i, v);
    }
    Case* self = &c;
    c.launch = [=]() { Case& c = *self; GO(car_launch_convert(mode, need(c, bs, (size_t)n * (src_dtype ? 2 : 4)), src_dtype, need(c, bd, (size_t)n * esz(mode)), n, 0)); };
    run(c);
}
static void build_text_case(int mode, int src_dtype, int B, long per, long per_src, long src_off, int cfg) {
    Case c; char nm[160]; snprintf(nm, sizeof nm, "build_text %s cond %s B %d per %ld of %ld at %ld cfg %d", mode ? "bf16" : "fp32", src_dtype ? "bf16" : "fp32", B, per, per_src, src_off, cfg); c.name = nm;
    const int es = esz(mode), ss = src_dtype ? 2 : 4; const long nd = (long)(cfg ? 2 * B : B) * per;
    const int bc = c.A.add((size_t)B * per_src * ss), bu = c.A.add((size_t)(src_off + per) * es), bd = c.A.add((size_t)nd * es);
    auto val = [](unsigned i, unsigned s) { const unsigned h = hsh(i, 0, s); return h % 11 == 0 ? -0.f : h % 11 == 1 ? 257.f : h % 11 == 2 ? 1.00390625f : (float)((int)(h % 2001) - 1000) / 64.f; };
    for (long i = 0; i < B * per_src; ++i) put(c.A.init, c.A.off[bc], i, src_dtype, val((unsigned)i, 71));
    for (long i = 0; i < src_off + per; ++i) put(c.A.init, c.A.off[bu], i, mode, val((unsigned)i, 72));
    c.A.seal();
    for (long i = 0; i < nd; ++i) { const long b = i / per, r = i - b * per; float v;
        if (b < B) v = get(c.A.init.data(), c.A.off[bc], b * per_src + src_off + r, src_dtype); else { v = get(c.A.init.data(), c.A.off[bu], src_off + r, mode); if (v == 0.f) v = 0.f; }      // 0 + (-0) = +0
        put(c.A.exp, c.A.off[bd], i, mode, v); }
    Case* self = &c;
    c.launch = [=]() { Case& c = *self; GO(car_launch_build_text(mode, need(c, bc, (size_t)((B - 1) * per_src + src_off + per) * ss), src_dtype, need(c, bu, (size_t)(src_off + per) * es), need(c, bd, (size_t)nd * es), B, per, per_src, src_off, cfg, 0)); };
    run(c);
}
static void gather_case(int mode, long rows, int D) {
    Case c; char nm[120]; snprintf(nm, sizeof nm, "gather_rows %s rows %ld D %d (raw patterns, NaN payloads)", mode ? "bf16" : "fp32", rows, D); c.name = nm;
    const int es = esz(mode), nt = 37; const int bt = c.A.add((size_t)nt * D * es), bi = c.A.add(rows * 4), bo = c.A.add((size_t)rows * D * es);
    for (long i = 0; i < (long)nt * D; ++i) { const unsigned h = hsh((unsigned)i, 0, 81); if (mode) putv<uint16_t>(c.A.init, c.A.off[bt], i, (uint16_t)(i % 5 == 0 ? 0x7f81 + (h & 0x7e) : h)); else putv<uint32_t>(c.A.init, c.A.off[bt], i, i % 5 == 0 ? 0x7f800001u + (h & 0x3ffffe) : h); }
    std::vector<int> idx(rows); for (long r = 0; r < rows; ++r) { idx[r] = r == 0 ? nt - 1 : r == 1 ? 0 : hint((unsigned)r, 0, 82, 0, nt - 1); putv<int>(c.A.init, c.A.off[bi], r, idx[r]); }
    c.A.seal();
    for (long r = 0; r < rows; ++r) memcpy(&c.A.exp[c.A.off[bo] + (size_t)r * D * es], &c.A.init[c.A.off[bt] + (size_t)idx[r] * D * es], (size_t)D * es);
    Case* self = &c;
    c.launch = [=]() { Case& c = *self; GO(car_launch_gather_rows(mode, need(c, bt, (size_t)nt * D * es), (const int*)need(c, bi, rows * 4), need(c, bo, (size_t)rows * D * es), rows, D, 0)); };
    run(c);
}
static void label_case(int bad) {      // bad 0: every conditional row in range (bad labels only behind unconditional rows); 1..3: one conditional row with -1 / nc + 1 / 2^40
    Case c; const int nc = 1000, b = 300, nimg = 150; const long long bads[] = {0, -1, nc + 1, 1LL << 40};
    char nm[120]; snprintf(nm, sizeof nm, "label_index labels {0, nc - 1, nc%s}, unconditional rows, flag %s", bad == 1 ? ", -1" : bad == 2 ? ", nc + 1" : bad == 3 ? ", 2^40" : "", bad ? "set" : "untouched"); c.name = nm;
    const int bl = c.A.add(nimg * 8), bri = c.A.add(b * 4), bru = c.A.add(b * 4), bi = c.A.add(b * 4), bf = c.A.add(4);
    std::vector<long long> lab(nimg); for (int i = 0; i < nimg; ++i) lab[i] = i == 0 ? 0 : i == 1 ? nc - 1 : i == 2 ? nc : i == 3 ? -1 : i == 4 ? nc + 1 : i == 5 ? (1LL << 40) : i == 6 ? (1LL << 32) + 5 : hint(i, 0, 91, 0, nc);
    std::vector<int> ri(b), ru(b);
    for (int r = 0; r < b; ++r) { ri[r] = r % nimg; ru[r] = r >= nimg; if (r == 3 || r == 4 || r == 5 || r == 6) ri[r] = 7; }      // images 3..6 (bad labels) only through unconditional rows
    if (bad) { ri[260] = 7; ru[260] = 0; lab[7] = bads[bad]; ri[299] = 3; }      // row 299 unconditional, on a bad image: ignored
    for (int i = 0; i < nimg; ++i) putv<long long>(c.A.init, c.A.off[bl], i, lab[i]);
    for (int r = 0; r < b; ++r) { putv<int>(c.A.init, c.A.off[bri], r, ri[r]); putv<int>(c.A.init, c.A.off[bru], r, ru[r]); }
    putv<int>(c.A.init, c.A.off[bf], 0, 0);
    c.A.seal();
    bool flag = false;
    for (int r = 0; r < b; ++r) { long long l = ru[r] ? nc : lab[ri[r]]; if (l < 0 || l > nc) { flag = true; l = nc; } putv<int>(c.A.exp, c.A.off[bi], r, (int)l); }
    if (flag != (bad != 0)) pre_fail(c, "flag expectation");
    putv<int>(c.A.exp, c.A.off[bf], 0, flag ? 1 : 0);
    Case* self = &c;
    c.launch = [=]() { Case& c = *self; GO(car_launch_label_index((const int64_t*)need(c, bl, nimg * 8), (const int*)need(c, bri, b * 4), (const int*)need(c, bru, b * 4), nc, (int*)need(c, bi, b * 4), (int*)need(c, bf, 4), b, 0)); };
    run(c);
}
static void t5_prep_case(bool with_mask) {
    Case c; c.name = std::string("t5_prep ids {-1, 0, vocab - 1, vocab, 2^40, 2^32 + 7}, ") + (with_mask ? "mask {0, 1, 2, -1, 2^32}" : "mask == nullptr");
    const long n = 300; const int vocab = 32128; const int bi = c.A.add(n * 8), bm = with_mask ? c.A.add(n * 8) : -1, bo = c.A.add(n * 4), bk = c.A.add(n);
    const long long sp[] = {-1, 0, vocab - 1, vocab, 1LL << 40, (1LL << 32) + 7, -(1LL << 40), LLONG_MIN}, ms[] = {0, 1, 2, -1, 1LL << 32};
    std::vector<long long> ids(n), mk(n);
    for (long i = 0; i < n; ++i) { ids[i] = i < 8 ? sp[i] : hint((unsigned)i, 0, 95, 0, vocab - 1); mk[i] = ms[hsh((unsigned)i, 1, 95) % 5]; putv<long long>(c.A.init, c.A.off[bi], i, ids[i]); if (with_mask) putv<long long>(c.A.init, c.A.off[bm], i, mk[i]); }
    c.A.seal();
    for (long i = 0; i < n; ++i) { long long v = ids[i]; if (v < 0) v = 0; if (v >= vocab) v = vocab - 1; putv<int>(c.A.exp, c.A.off[bo], i, (int)v); c.A.exp[c.A.off[bk] + i] = with_mask ? (mk[i] != 0) : 1; }
    Case* self = &c;
    c.launch = [=]() { Case& c = *self; GO(car_launch_t5_prep((const long long*)need(c, bi, n * 8), with_mask ? (const long long*)need(c, bm, n * 8) : nullptr, (int*)need(c, bo, n * 4), (unsigned char*)need(c, bk, n), n, vocab, 0)); };
    run(c);
}
// bicubic: weights are dyadic, (-1/8, 5/8, 5/8, -1/8) or (0, 1, 0, 0) or (0, 1/2, 1/2, 0) per output index, indices clamped at the border; on an integer image the row
// sums are multiples of 1/8 and the column sum a multiple of 1/64, all exact in fp32 in the kernel's x-then-y order, so the interpolated value has one result (and one
// bf16 rounding where the image is bf16)
static void patchify_case(int mode, int img_dtype, int bicubic, bool big) {
    Case c; const int B = 2, H = big ? 40 : 9, W = big ? 44 : 11, p = big ? 14 : 2, gh = big ? 37 : 3, gw = big ? 37 : 4, Kpad = big ? 608 : 16, OH = gh * p, OW = gw * p;
    char nm[160]; snprintf(nm, sizeof nm, "patchify %s image %s %s %dx%d -> %dx%d patches of %d, Kpad %d", mode ? "bf16" : "fp32", img_dtype ? "bf16" : "fp32", bicubic ? "bicubic (dyadic weights)" : "nearest", H, W, gh, gw, p, Kpad); c.name = nm;
    const int es = esz(mode), is = img_dtype ? 2 : 4, nt = bicubic ? 4 : 1; const long nimg = (long)B * 3 * H * W, nout = (long)B * gh * gw * Kpad;
    const int bi = c.A.add(nimg * is), bo = c.A.add(nout * es), biy = c.A.add(OH * nt * 4), bix = c.A.add(OW * nt * 4), bwy = c.A.add(OH * 4 * 4), bwx = c.A.add(OW * 4 * 4);
    std::vector<float> img(nimg); for (long i = 0; i < nimg; ++i) img[i] = (float)hint((unsigned)i, 0, 101, 0, 255);
    const float ws[3][4] = {{-0.125f, 0.625f, 0.625f, -0.125f}, {0.f, 1.f, 0.f, 0.f}, {0.f, 0.5f, 0.5f, 0.f}};
    std::vector<int> iy(OH * nt), ix(OW * nt); std::vector<float> wy(OH * 4), wx(OW * 4);
    for (int o = 0; o < OH; ++o) { const int s = o * H / OH; for (int a = 0; a < nt; ++a) iy[o * nt + a] = bicubic ? std::min(std::max(s - 1 + a, 0), H - 1) : (o * 7 + 3) % H; for (int a = 0; a < 4; ++a) wy[o * 4 + a] = ws[hsh(o, 0, 102) % 3][a]; }
    for (int o = 0; o < OW; ++o) { const int s = o * W / OW; for (int a = 0; a < nt; ++a) ix[o * nt + a] = bicubic ? std::min(std::max(s - 1 + a, 0), W - 1) : (o * 5 + 1) % W; for (int a = 0; a < 4; ++a) wx[o * 4 + a] = ws[hsh(o, 1, 102) % 3][a]; }
    for (long i = 0; i < nimg; ++i) put(c.A.init, c.A.off[bi], i, img_dtype, img[i]);
    for (size_t i = 0; i < iy.size(); ++i) putv<int>(c.A.init, c.A.off[biy], i, iy[i]); for (size_t i = 0; i < ix.size(); ++i) putv<int>(c.A.init, c.A.off[bix], i, ix[i]);
    for (size_t i = 0; i < wy.size(); ++i) putv<float>(c.A.init, c.A.off[bwy], i, wy[i]); for (size_t i = 0; i < wx.size(); ++i) putv<float>(c.A.init, c.A.off[bwx], i, wx[i]);
    c.A.seal();
    for (long i = 0; i < nout; ++i) {
        const int k = (int)(i % Kpad); const long t = i / Kpad; double v = 0;
        if (k < 3 * p * p) {
            const int ch = k / (p * p), py = (k % (p * p)) / p, pxx = k % p, gx = (int)(t % gw), gy = (int)((t / gw) % gh), b = (int)(t / ((long)gw * gh)), oy = gy * p + py, ox = gx * p + pxx;
            const float* im = &img[((long)b * 3 + ch) * H * W];
            if (!bicubic) v = im[(long)iy[oy] * W + ix[ox]];
            else { for (int a = 0; a < 4; ++a) { double row = 0; for (int q = 0; q < 4; ++q) row += (double)im[(long)iy[oy * 4 + a] * W + ix[ox * 4 + q]] * wx[ox * 4 + q]; v += row * wy[oy * 4 + a]; }
                if (v * 64 != std::floor(v * 64) || std::fabs(v) > 1024) pre_fail(c, "bicubic value not a small multiple of 1/64"); if (img_dtype == 1) v = bfv(r_bf((float)v)); }
        }
        put(c.A.exp, c.A.off[bo], i, mode, (float)v);
    }
    Case* self = &c;
    c.launch = [=]() { Case& c = *self; GO(car_launch_patchify(mode, need(c, bi, nimg * is), img_dtype, need(c, bo, nout * es), B, H, W, gh, gw, p, Kpad, bicubic, (const int*)need(c, biy, OH * nt * 4), (const int*)need(c, bix, OW * nt * 4),
                                                               (const float*)need(c, bwy, OH * 4 * 4), (const float*)need(c, bwx, OW * 4 * 4), 0)); };
    run(c);
}
static void vit_assemble_case(int mode, int B, int n, int D) {
    Case c; char nm[100]; snprintf(nm, sizeof nm, "vit_assemble %s B %d n %d D %d", mode ? "bf16" : "fp32", B, n, D); c.name = nm;
    const int es = esz(mode); const long nt = (long)B * n * D, np = (long)(n + 1) * D, nh = (long)B * (n + 1) * D;
    const int bt = c.A.add(nt * es), bc = c.A.add((size_t)D * es), bp = c.A.add(np * es), bh = c.A.add(nh * es);
    auto tv = [](long i) { return (float)hint((unsigned)i, 0, 111, -60, 60); }; auto cv = [](long i) { return (float)hint((unsigned)i, 1, 111, -60, 60); }; auto pv = [](long i) { return (float)hint((unsigned)i, 2, 111, -60, 60); };
    for (long i = 0; i < nt; ++i) put(c.A.init, c.A.off[bt], i, mode, tv(i)); for (int i = 0; i < D; ++i) put(c.A.init, c.A.off[bc], i, mode, cv(i)); for (long i = 0; i < np; ++i) put(c.A.init, c.A.off[bp], i, mode, pv(i));
    c.A.seal();
    for (long i = 0; i < nh; ++i) { const int d = (int)(i % D); const long r = i / D; const int t = (int)(r % (n + 1)); const long b = r / (n + 1); put(c.A.exp, c.A.off[bh], i, mode, (t == 0 ? cv(d) : tv((b * n + t - 1) * D + d)) + pv((long)t * D + d)); }
    Case* self = &c;
    c.launch = [=]() { Case& c = *self; GO(car_launch_vit_assemble(mode, need(c, bt, nt * es), need(c, bc, (size_t)D * es), need(c, bp, np * es), need(c, bh, nh * es), B, n, D, 0)); };
    run(c);
}
static void put_row(std::vector<u8>& im, size_t off, int i, const SampleRow& r) { memcpy(&im[off + (size_t)i * sizeof(SampleRow)], &r, sizeof r); }
static void ctrl_scale_case(int mode, long per) {
    Case c; char nm[100]; snprintf(nm, sizeof nm, "ctrl_scale_rows %s per %ld (cs 0.7, 1.3: one IEEE product)", mode ? "bf16" : "fp32", per); c.name = nm;
    const int es = esz(mode), n_img = 2; const float cs[2] = {0.7f, 1.3f};
    const int bc = c.A.add((size_t)n_img * per * es), br = c.A.add(n_img * sizeof(SampleRow));
    for (long i = 0; i < n_img * per; ++i) put(c.A.init, c.A.off[bc], i, mode, (float)gauss((unsigned)i, 0, 121));
    for (int i = 0; i < n_img; ++i) { SampleRow r; memset(&r, 0, sizeof r); r.control_strength = cs[i]; r.cfg_scale = 99.f; r.temperature = 77.f; put_row(c.A.init, c.A.off[br], i, r); }
    c.A.seal();
    for (long i = 0; i < n_img * per; ++i) put(c.A.exp, c.A.off[bc], i, mode, fmul(cs[i / per], get(c.A.init.data(), c.A.off[bc], i, mode)));
    if (per % 4) pre_fail(c, "per % 4");
    Case* self = &c;
    c.launch = [=]() { Case& c = *self; GO(car_launch_ctrl_scale_rows(mode, need(c, bc, (size_t)n_img * per * es), (const SampleRow*)need(c, br, n_img * sizeof(SampleRow)), n_img, per, 0)); };
    run(c);
}
static void row_mix_case() {
    Case c; c.name = "row_mix_scale cfg_interval {-1, 0, n_new - 2, n_new}";
    const int n_img = 4, n_new = 130; const int ci[4] = {-1, 0, n_new - 2, n_new}; const float sc[4] = {7.5f, 1.3f, 4.f, 2.7f};
    const int br = c.A.add(n_img * sizeof(SampleRow)), bo = c.A.add((size_t)n_img * n_new * 4);
    for (int i = 0; i < n_img; ++i) { SampleRow r; memset(&r, 0, sizeof r); r.cfg_scale = sc[i]; r.cfg_interval = ci[i]; r.control_strength = 55.f; put_row(c.A.init, c.A.off[br], i, r); }
    c.A.seal();
    for (int i = 0; i < n_img; ++i) for (int j = 0; j < n_new; ++j) putv<float>(c.A.exp, c.A.off[bo], (size_t)i * n_new + j, (ci[i] > -1 && j - 1 > ci[i]) ? 1.f : sc[i]);
    Case* self = &c;
    c.launch = [=]() { Case& c = *self; GO(car_launch_row_mix_scale((const SampleRow*)need(c, br, n_img * sizeof(SampleRow)), (float*)need(c, bo, (size_t)n_img * n_new * 4), n_img, n_new, 0)); };
    run(c);
}
static void pos_step_cases() {
    { Case c; c.name = "set_pos_step: 16 ints and the guard behind them"; const int b = c.A.add(64); c.A.seal(); for (int i = 0; i < 16; ++i) putv<int>(c.A.exp, c.A.off[b], i, (i & 1) ? 1234567 : -89);
      Case* self = &c; c.launch = [=]() { GO(car_launch_set_pos_step((int*)need(*self, b, 64), -89, 1234567, 0)); }; run(c); }
    { Case c; c.name = "advance: pos += 1, step += 1"; const int bp = c.A.add(4), bs = c.A.add(4); putv<int>(c.A.init, c.A.off[bp], 0, 41); putv<int>(c.A.init, c.A.off[bs], 0, -1); c.A.seal();
      putv<int>(c.A.exp, c.A.off[bp], 0, 42); putv<int>(c.A.exp, c.A.off[bs], 0, 0);
      Case* self = &c; c.launch = [=]() { GO(car_launch_advance((int*)need(*self, bp, 4), (int*)need(*self, bs, 4), 0)); }; run(c); }
}
static void copies_all() {
    for (int mode = 0; mode < 2; ++mode) for (int sd = 0; sd < 2; ++sd) convert_case(mode, sd);
    for (int mode = 0; mode < 2; ++mode) for (int sd = 0; sd < 2; ++sd) for (int cfg = 0; cfg < 2; ++cfg) { build_text_case(mode, sd, 2, 520, 1000, 480, cfg); build_text_case(mode, sd, 2, 1000, 1000, 0, cfg); }
    build_text_case(1, 0, 2, 140000, 150000, 10000, 1);      // 4 * 140000 > 2048 * 256: the stride loop runs twice
    for (int mode = 0; mode < 2; ++mode) { gather_case(mode, 5, 24); gather_case(mode, 600, 1000); }
    for (int bad = 0; bad < 4; ++bad) label_case(bad);
    t5_prep_case(true); t5_prep_case(false);
    for (int mode = 0; mode < 2; ++mode) for (int id = 0; id < 2; ++id) for (int bc = 0; bc < 2; ++bc) patchify_case(mode, id, bc, false);
    patchify_case(1, 0, 1, true);      // 2 * 37 * 37 * 608 > 4096 * 256
    for (int mode = 0; mode < 2; ++mode) { vit_assemble_case(mode, 2, 5, 24); vit_assemble_case(mode, 2, 256, 1024); }
    for (int mode = 0; mode < 2; ++mode) for (long per : {4L, 1020L, 65540L}) ctrl_scale_case(mode, per);
    row_mix_case(); pos_step_cases();
}

int main(int argc, char** argv) {
    const std::string m = argc > 1 ? argv[1] : "quick";
    if (m != "quick" && m != "selftest") { printf("usage: ops_check [quick | selftest]\n"); return 2; }
    g_selftest = m == "selftest";
    // the reference's bf16 on its own corner cases
    if (r_bf(257.f) != 0x4380 || r_bf(259.f) != 0x4382 || r_bf(3.4e38f) != 0x7f80 || r_bf(-0.f) != 0x8000 || (r_bf(NAN) & 0x7fc0) != 0x7fc0 || r_bf(1.00390625f) != 0x3f80 || r_bf(1.01171875f) != 0x3f82) { printf("reference bf16 rounding FAIL\n"); return 1; }
    unsetenv("CAR_GN_SCALAR");
    const auto t0 = std::chrono::steady_clock::now();
    gn_all(); am_all(); lookup_all(); conv_all(); rms_all(); ln_all(); glu_all(); copies_all();
    if (g_dev) CK(hipFree(g_dev));
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%d cases, %d failed, %.1f s\n", g_cases, g_fail, sec);
    if (g_fail) { printf("%d case(s) FAILED\n", g_fail); return 1; }
    printf("all checks passed\n");
    return 0;
}
