// experiments/gemm_check.hip — every kernel family behind car_launch_gemm (controlar_amd/csrc/gemm.hip) against EXACT integer references, through the real launcher:
// gemm_bf16_kernel, gemm_bf16_glds_kernel, conv3_halo64_kernel, conv3_halo_kernel, gemm_f32_mfma_kernel, gemm_f32_kernel (gemm_f32s_kernel stays with
// split_gemm_check.hip).  Compiled with -DCAR_DEV_KNOBS, so that CAR_CONV_HALO128 / CAR_GEMM_V1 / CAR_NO_HALO / CAR_CONV_LINEAR / CAR_GN_UNFUSED really select
// the alternate routes; every case asserts its car_gemm_route value before it launches.
//
// Operands are small integers taken from a hash of (row, column, seed) — a swapped row, tap, channel chunk or batch reads another pattern — so every product and
// sum is exact in fp32 and the expected output has NO tolerance: the whole output allocation (values, the ldc > N gap columns, the gaps between batches and 4096
// guard elements past the end, all poisoned with 0xff bytes before each launch) is compared with memcmp.  In units u = alpha * ascale (a power of two) a case is
//     out = u * ((acc + bias_i) * scale_i + R_i),   acc = sum_k a_i w_i   (integers)
// and the host verifies for EVERY output element the condition that makes each rounding point of the epilogue the identity:
//     (sum |a w| + |bias_i|) * |scale_i| + |R_i|  <=  256   in bf16 mode (8 significant bits: the bf16 store is exact, a wrong addend cannot hide in a rounding)
//                                                 <  2^24   in fp32 mode
// A violated condition is a HARNESS error ("PRECONDITION"), not a kernel failure.  A is sparse (one non-zero per `dens` consecutive k, at a hashed position) to
// keep that sum and the host reference small; W is dense in {-2..2}.
// Three "big" bf16 cases (one per epilogue path: EP_VEC, EP_SCALAR, EP_SWIGLU) use dense, wider operands: the sum only has to stay below 2^24 (the fp32 accumulator
// is exact) and the reference replays the documented rounding points in float —  rnd(alpha acc + bias) -> act -> rnd(. scale) -> rnd(+ R),  still ==;  for SwiGLU
// rnd(acc) of gate and linear column (accumulators far beyond 8 bits, so that rounding is NOT the identity) -> gate -> rnd -> * c -> rnd,  under the SwiGLU bound.
// This pins the ORDER of the roundings.
// The only non-exact cases are the activations (GELU-erf, GELU-tanh, SiLU) and SwiGLU.  Their pre-activations are exact multiples of 1/8; the reference is the fp64
// function rounded to bf16; the bound is DERIVED, not measured: one bf16 ulp of the reference (activations), ulp(gate) |c| + ulp(out) (SwiGLU), and at most 1 % of
// the elements may differ at all.  fp32 erff / tanhf / expf are within a few 2^-23 of the true value against a bf16 half-ulp of 2^-9 relative, so the device lands
// on the reference or its neighbour — as long as 1 + erf(x / sqrt 2) and 1 + tanh(..) do not cancel: below x ~ -4.3 the fp32 formula (the reference model's own)
// loses all relative accuracy (it returns -0 where the true value is -1e-9).  So the two GELU forms are checked on x in [-3.5, 30.5] and SiLU, which has no such
// cancellation, on the whole [-30.5, 30.5] (the "wide" cases spread x with a large bias; the harness checks the range), inside the [-31, 31] in which
// multiples of 1/8 are exact.
// Every case runs twice (equal bits).  Refused calls (negative route) must return non-zero and leave the whole allocation untouched.
//   quick      all checks, no timing; prints "all checks passed"
//   selftest   host only, no HIP call: builds every case's data and reference, checks every precondition, and shows with the host's fp32 libm in place of the device
//              that the derived activation bounds and the 1 % cap hold for the reference alone
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -DCAR_DEV_KNOBS -I controlar_amd/csrc experiments/gemm_check.hip -o experiments/gemm_check && experiments/gemm_check quick
#ifndef CAR_DEV_KNOBS
#error "gemm_check needs -DCAR_DEV_KNOBS: without it CAR_KNOB() is a null constant and the cases that select conv3_halo_kernel, the register kernel at a halo shape, ... would silently run the default route"
#endif
#include "../controlar_amd/csrc/gemm.hip"
#include "../controlar_amd/csrc/gemm_split.hip"
#include "../controlar_amd/csrc/ops.hip"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

extern "C" { int g_car_knob_hits = 0; }        // the development build's counter lives in engine.hip, which is not part of this program

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)

static int g_fail = 0, g_cases = 0;
static unsigned hsh(unsigned a, unsigned b, unsigned seed) {
    unsigned x = a * 2654435761u + b * 0x85ebca6bu + seed * 0x9e3779b9u; x ^= x >> 15; x *= 2246822519u; x ^= x >> 13; x *= 3266489917u; x ^= x >> 16; return x;
}

struct Case {
    std::string name; int mode = 1, amode = AMODE_PLAIN, route = CAR_ROUTE_BF16_REG;
    int M = 0, N = 0, K = 0, nb0 = 1, nb1 = 1;
    long lda = 0, ldw = 0, ldc = 0;                 // 0: dense (K, K, output columns); R has the layout of C
    long padA = 0, padW = 0, padC = 0;              // batch strides: s1 = dense + pad, s0 = nb1 * s1 + 2 * pad (so s0 != nb1 * s1 when pad != 0)
    int B = 0, Ho = 0, Wo = 0, Cin = 0, ups = 0, patch = 0;      // convolutions: M = B * Ho * Wo, K = 9 * Cin
    int bias_mode = BIAS_NONE; bool bias_ptr = false, scale = false, resid = false, gn = false;
    float alpha = 1.f, ascale = 1.f; int act = ACT_NONE, out_f32 = 0, swiglu = 0;
    int dens = 0, brange = 8, xmax = 0, xneg = -1; bool big = false, bpos = false;         // dens 0: chosen from the precondition; xmax: bound on |pre-activation| in units (approximate cases), xneg: on its negative side (-1: xmax); bpos: bias >= 0
    const char* knob = nullptr;
    unsigned seed = 1;
};

// ---------------------------------------------------------------------------------------------------------------- operand values (integers, in units)
static int a_val(const Case& c, unsigned row, int col) {
    const int blk = col / c.dens;
    if (col % c.dens != (int)(hsh(row, (unsigned)blk, c.seed * 16u + 1u) % (unsigned)c.dens)) return 0;
    const unsigned h = hsh(row, (unsigned)col, c.seed * 16u + 2u);
    const int mag = c.big ? 1 + (int)(h % 4u) : 1 + (int)(h & 1u);
    return (h & 0x100u) ? -mag : mag;
}
static int w_val(const Case& c, unsigned row, int col) { const unsigned h = hsh(row, (unsigned)col, c.seed * 16u + 3u); return c.big ? (int)(h % 17u) - 8 : (int)(h % 5u) - 2; }
static int b_val(const Case& c, int i) {
    if (!c.brange) return 0;
    const unsigned h = hsh((unsigned)i, 0u, c.seed * 16u + 4u);
    return c.bpos ? (int)(h % (unsigned)(c.brange + 1)) : (int)(h % (unsigned)(2 * c.brange + 1)) - c.brange;
}
static int s_val(const Case& c, int n) { const unsigned h = hsh((unsigned)n, 0u, c.seed * 16u + 5u); const int m = c.big ? 1 + (int)(h % 3u) : 1 + (int)(h & 1u); return (h & 0x100u) ? -m : m; }
static int r_val(const Case& c, unsigned row, int n) { return (int)(hsh(row, (unsigned)n, c.seed * 16u + 6u) % 17u) - 8; }

static double ulp_bf16(double v) { if (v == 0 || !(std::fabs(v) < 1e300)) return 0; int e; (void)std::frexp(std::fabs(v), &e); return std::ldexp(1.0, e - 8); }
static float rbf(float v) { return bf2f(f2bf(v)); }
static double act64(int act, double x) {
    if (act == ACT_GELU_ERF) return 0.5 * x * (1.0 + std::erf(x * 0.70710678118654752440));
    if (act == ACT_GELU_TANH) return 0.5 * x * (1.0 + std::tanh(0.79788456080286535588 * (x + 0.044715 * x * x * x)));
    if (act == ACT_SILU) return x / (1.0 + std::exp(-x));
    return x;
}
// the kernels' fp32 formulas (car_common.h) on the host's libm: what selftest puts in the device's place
static float act32(int act, float x) {
    if (act == ACT_GELU_ERF) return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
    if (act == ACT_GELU_TANH) return 0.5f * x * (1.0f + tanhf(0.79788456080286535588f * (x + 0.044715f * x * x * x)));
    if (act == ACT_SILU) return x / (1.0f + expf(-x));
    return x;
}
static int gate_kind(int swiglu) { return swiglu == 2 ? ACT_GELU_TANH : ACT_SILU; }

// ---------------------------------------------------------------------------------------------------------------- one prepared case (host side)
struct Prep {
    bool conv = false, approx = false; int rows = 0, ocols = 0, Hin = 0, Win = 0, nz = 1, esz = 2, osz = 2;
    long lda = 0, ldw = 0, ldc = 0, sA0 = 0, sA1 = 0, sW0 = 0, sW1 = 0, sC0 = 0, sC1 = 0;
    size_t nA = 0, nW = 0, nC = 0, nCv = 0, nPart = 0;               // allocation sizes in elements (nC includes the guard; nCv without it)
    std::vector<unsigned char> A, W, bias, scl, R, expC;             // device images (raw bytes)
    std::vector<float> ref, tol, host32, expPart;                    // approximate cases: reference, bound, host-libm stand-in per element of the C allocation
    std::vector<unsigned char> isout;
    double worst = 0, xworst = 0; bool pre_ok = true; std::string why;
};
static const size_t GUARD = 4096;

static void put(std::vector<unsigned char>& buf, size_t i, int esz, float v) {
    if (esz == 2) { const bf16_t b = f2bf(v); memcpy(&buf[i * 2], &b, 2); } else memcpy(&buf[i * 4], &v, 4);
}

static void prepare(Case& c, Prep& P) {
    P.conv = c.amode != AMODE_PLAIN; P.esz = c.mode == 1 ? 2 : 4; P.osz = (c.mode == 0 || c.out_f32) ? 4 : 2;
    if (P.conv) { c.M = c.B * c.Ho * c.Wo; c.K = 9 * c.Cin; P.Hin = c.amode == AMODE_CONV3S2 ? c.Ho * 2 : c.Ho >> c.ups; P.Win = c.amode == AMODE_CONV3S2 ? c.Wo * 2 : c.Wo >> c.ups; }
    P.rows = c.M; P.ocols = c.swiglu ? c.N / 2 : c.N; P.nz = c.nb0 * c.nb1;
    P.approx = c.act != ACT_NONE || c.swiglu;
    const float unit = c.alpha * c.ascale;
    const int smax = c.scale ? (c.big ? 3 : 2) : 1, br = (c.bias_mode != BIAS_NONE) ? c.brange : 0;
    const int nterms = P.conv ? c.Cin : c.K;                          // per gathered A row; a conv output sums 9 of them
    if (c.big) c.dens = 1;
    if (!c.dens) { c.dens = 1; while (c.dens < nterms && ((long)((nterms + c.dens - 1) / c.dens) * (P.conv ? 9 : 1) * 4 + br) * smax + (c.resid ? 8 : 0) > 256) c.dens *= 2; }
    const long arows = P.conv ? (long)c.B * P.Hin * P.Win : c.M, acols = P.conv ? c.Cin : c.K;
    P.lda = P.conv ? acols : (c.lda ? c.lda : c.K); P.ldw = c.ldw ? c.ldw : c.K; P.ldc = c.ldc ? c.ldc : P.ocols;
    P.sA1 = arows * P.lda + c.padA; P.sA0 = c.nb1 * P.sA1 + 2 * c.padA;
    P.sW1 = (long)c.N * P.ldw + c.padW; P.sW0 = c.nb1 * P.sW1 + 2 * c.padW;
    P.sC1 = (long)P.rows * P.ldc + c.padC; P.sC0 = c.nb1 * P.sC1 + 2 * c.padC;
    auto zoff = [&](int z, long s0, long s1) { return (long)(z / c.nb1) * s0 + (long)(z % c.nb1) * s1; };
    P.nA = (size_t)(zoff(P.nz - 1, P.sA0, P.sA1) + (arows - 1) * P.lda + acols);
    P.nW = (size_t)(zoff(P.nz - 1, P.sW0, P.sW1) + (long)(c.N - 1) * P.ldw + c.K);
    P.nCv = (size_t)(zoff(P.nz - 1, P.sC0, P.sC1) + (long)(P.rows - 1) * P.ldc + P.ocols); P.nC = P.nCv + GUARD;
    // ---- device images
    P.A.assign(P.nA * P.esz, 0); P.W.assign(P.nW * P.esz, 0);
    std::vector<signed char> Wt((size_t)P.nz * c.K * c.N);            // [z][k][n]: the reference walks n innermost
    for (int z = 0; z < P.nz; ++z) {
        for (long r = 0; r < arows; ++r) for (int k = 0; k < acols; ++k) { const int v = a_val(c, (unsigned)(z * arows + r), k); if (v) put(P.A, (size_t)(zoff(z, P.sA0, P.sA1) + r * P.lda + k), P.esz, v * c.ascale); }
        for (int n = 0; n < c.N; ++n) for (int k = 0; k < c.K; ++k) { const int v = w_val(c, (unsigned)(z * c.N + n), k); Wt[((size_t)z * c.K + k) * c.N + n] = (signed char)v; put(P.W, (size_t)(zoff(z, P.sW0, P.sW1) + (long)n * P.ldw + k), P.esz, (float)v); }
    }
    const int nbias = c.bias_mode == BIAS_M ? c.M : c.N;
    if (c.bias_mode != BIAS_NONE) { P.bias.assign((size_t)nbias * P.esz, 0); for (int i = 0; i < nbias; ++i) put(P.bias, i, P.esz, b_val(c, i) * unit); }
    else if (c.bias_ptr) { P.bias.assign((size_t)c.N * P.esz, 0); for (int i = 0; i < c.N; ++i) put(P.bias, i, P.esz, 3.f + (float)(i & 3)); }      // must NOT be added
    if (c.scale) { P.scl.assign((size_t)c.N * P.esz, 0); for (int n = 0; n < c.N; ++n) put(P.scl, n, P.esz, (float)s_val(c, n)); }
    if (c.resid) { P.R.assign(P.nCv * P.esz, 0); }
    P.expC.assign(P.nC * P.osz, 0xff);
    if (P.approx) { P.ref.assign(P.nC, 0.f); P.tol.assign(P.nC, 0.f); P.host32.assign(P.nC, 0.f); P.isout.assign(P.nC, 0); }
    const int tw = c.Wo >> 4, th = c.Ho >> 4;
    std::vector<double> gsum, gsq;
    if (c.gn) { P.nPart = (size_t)c.B * tw * th * 2 * c.N; gsum.assign(P.nPart / 2, 0.0); gsq.assign(P.nPart / 2, 0.0); }
    // ---- reference, rows dealt to at most 16 threads
    unsigned nthr = std::thread::hardware_concurrency(); if (nthr < 1) nthr = 1; if (nthr > 16) nthr = 16;
    const long total = (long)P.nz * P.rows;
    std::vector<double> tworst(nthr, 0.0), txw(nthr, 0.0); std::vector<int> tbad(nthr, 0);
    auto work = [&](unsigned t) {
        std::vector<int> acc(c.N), sab(c.N); std::vector<std::pair<int, int>> nzs;
        for (long zr = t; zr < total; zr += nthr) {
            const int z = (int)(zr / P.rows), m = (int)(zr % P.rows);
            nzs.clear();
            auto gather = [&](long arow, int kbase) {
                for (int blk = 0; blk * c.dens < acols; ++blk) {
                    const int col = blk * c.dens + (int)(hsh((unsigned)(z * arows + arow), (unsigned)blk, c.seed * 16u + 1u) % (unsigned)c.dens);
                    if (col < acols) { const int v = a_val(c, (unsigned)(z * arows + arow), col); if (v) nzs.push_back({kbase + col, v}); }
                }
            };
            if (!P.conv) gather(m, 0);
            else {
                const int hw = c.Ho * c.Wo, b = m / hw, y = (m % hw) / c.Wo, x = m % c.Wo;
                for (int tap = 0; tap < 9; ++tap) {
                    int iy, ix;
                    if (c.amode == AMODE_CONV3S2) { iy = 2 * y + tap / 3; ix = 2 * x + tap % 3; if (iy >= P.Hin || ix >= P.Win) continue; }
                    else { const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1; if (yy < 0 || yy >= c.Ho || xx < 0 || xx >= c.Wo) continue; iy = yy >> c.ups; ix = xx >> c.ups; }
                    gather(((long)b * P.Hin + iy) * P.Win + ix, tap * c.Cin);
                }
            }
            for (int n = 0; n < c.N; ++n) { acc[n] = 0; sab[n] = 0; }
            for (auto& kv : nzs) {
                const signed char* w = &Wt[((size_t)z * c.K + kv.first) * c.N]; const int a = kv.second, aa = std::abs(a);
                for (int n = 0; n < c.N; ++n) { acc[n] += a * w[n]; sab[n] += aa * std::abs((int)w[n]); }
            }
            const long cbase = zoff(z, P.sC0, P.sC1) + (long)m * P.ldc;
            const unsigned rrow = (unsigned)(z * P.rows + m);
            for (int j = 0; j < P.ocols; ++j) {
                const size_t ci = (size_t)(cbase + j);
                if (c.swiglu) {
                    const int na = (j >> 4) * 32 + (j & 15), nc2 = na + 16;
                    const double lim = c.big ? 16777216.0 : 256.0, s = std::max(sab[na], sab[nc2]);
                    if (s > tworst[t]) tworst[t] = s;
                    if (!(s <= lim)) tbad[t] = 1;
                    if (c.xmax && (std::abs(acc[na]) > c.xmax || std::abs(acc[nc2]) > c.xmax)) tbad[t] = 1;
                    if (std::abs(acc[na]) > txw[t]) txw[t] = std::abs(acc[na]);
                    const float av = rbf((float)acc[na] * c.ascale), cv = rbf((float)acc[nc2] * c.ascale);
                    const float g = rbf((float)act64(gate_kind(c.swiglu), av)), o = rbf(g * cv);
                    P.ref[ci] = o; P.tol[ci] = (float)(ulp_bf16(g) * std::fabs(cv) + ulp_bf16(o)); P.isout[ci] = 1;
                    P.host32[ci] = rbf(rbf(act32(gate_kind(c.swiglu), av)) * cv);
                    put(P.expC, ci, P.osz, o);
                    continue;
                }
                const int bi = c.bias_mode == BIAS_N ? b_val(c, j) : c.bias_mode == BIAS_M ? b_val(c, m) : 0, si = c.scale ? s_val(c, j) : 1, ri = c.resid ? r_val(c, rrow, j) : 0;
                if (c.resid) put(P.R, ci, P.esz, ri * unit);
                const double cond = ((double)sab[j] + std::abs(bi)) * std::abs(si) + std::abs(ri);
                if (cond > tworst[t]) tworst[t] = cond;
                const double lim = (c.mode == 0 || c.big) ? 16777216.0 - 1.0 : 256.0;
                if (!(cond <= lim)) tbad[t] = 1;
                float out;
                if (c.act != ACT_NONE) {
                    const int xi = acc[j] + bi;
                    if (xi > c.xmax || -xi > (c.xneg >= 0 ? c.xneg : c.xmax)) tbad[t] = 1;
                    if (std::abs(xi) > txw[t]) txw[t] = std::abs(xi);
                    const float x = (float)xi * unit;                                 // exact, and exact in bf16
                    out = c.mode == 1 ? rbf((float)act64(c.act, x)) : (float)act64(c.act, x);
                    P.ref[ci] = out; P.tol[ci] = (float)ulp_bf16(out); P.isout[ci] = 1;
                    P.host32[ci] = c.mode == 1 ? rbf(act32(c.act, x)) : act32(c.act, x);
                } else if (c.big) {                                                   // replay of the rounding points (bf16 mode)
                    float x = (float)acc[j] * c.alpha; x += (float)bi * unit; x = rbf(x);
                    if (c.scale) x = rbf(x * (float)si);
                    if (c.resid) x = rbf(x + (float)ri * unit);
                    out = x;
                } else out = unit * (float)((acc[j] + bi) * si + ri);
                put(P.expC, ci, P.osz, out);
            }
        }
    };
    std::vector<std::thread> th_;
    for (unsigned t = 0; t < nthr; ++t) th_.emplace_back(work, t);
    for (auto& t : th_) t.join();
    for (unsigned t = 0; t < nthr; ++t) { if (tworst[t] > P.worst) P.worst = tworst[t]; if (txw[t] > P.xworst) P.xworst = txw[t]; if (tbad[t]) P.pre_ok = false; }
    if (c.gn) {
        // GroupNorm stage-1 partials of the STORED values per (image, 16x16 tile, channel): integers, |v| <= 256 over 256 pixels, so both sums are exact in fp32
        // in any order (the harness checks < 2^24 + 1).  Layout [B][tiles][2][N] (GemmP::gn_part).
        for (int m = 0; m < c.M; ++m) {
            const int hw = c.Ho * c.Wo, b = m / hw, y = (m % hw) / c.Wo, x = m % c.Wo;
            const size_t t2 = (size_t)b * tw * th + (size_t)(y >> 4) * tw + (x >> 4);
            for (int j = 0; j < c.N; ++j) { bf16_t v; memcpy(&v, &P.expC[((size_t)m * P.ldc + j) * 2], 2); const double f = bf2f(v); gsum[t2 * c.N + j] += f; gsq[t2 * c.N + j] += f * f; }
        }
        P.expPart.assign(P.nPart + 256, 0.f); memset(P.expPart.data(), 0xff, (P.nPart + 256) * 4);
        for (size_t t2 = 0; t2 < (size_t)c.B * tw * th; ++t2)
            for (int j = 0; j < c.N; ++j) {
                if (std::fabs(gsum[t2 * c.N + j]) > 16777216.0 || gsq[t2 * c.N + j] > 16777216.0) P.pre_ok = false;
                P.expPart[t2 * 2 * c.N + j] = (float)gsum[t2 * c.N + j]; P.expPart[(t2 * 2 + 1) * c.N + j] = (float)gsq[t2 * c.N + j];
            }
    }
}

static const char* route_name(int r) {
    switch (r) {
    case CAR_ROUTE_BF16_REG: return "BF16_REG"; case CAR_ROUTE_BF16_GLDS: return "BF16_GLDS"; case CAR_ROUTE_HALO64: return "HALO64"; case CAR_ROUTE_HALO128: return "HALO128";
    case CAR_ROUTE_F32_SPLIT: return "F32_SPLIT"; case CAR_ROUTE_F32_MFMA: return "F32_MFMA"; case CAR_ROUTE_F32_VALU: return "F32_VALU";
    case CAR_ROUTE_REFUSE_GN: return "refused(gn_part)"; case CAR_ROUTE_REFUSE_K: return "refused(K)"; default: return "?";
    }
}
static float ld_out(const std::vector<unsigned char>& buf, size_t i, int osz) { if (osz == 2) { bf16_t b; memcpy(&b, &buf[i * 2], 2); return bf2f(b); } float f; memcpy(&f, &buf[i * 4], 4); return f; }
template <typename T> static T* upload(const std::vector<unsigned char>& h) { if (h.empty()) return nullptr; T* d; CK(hipMalloc(&d, h.size())); CK(hipMemcpy(d, h.data(), h.size(), hipMemcpyHostToDevice)); return d; }

static void run(Case c, bool device) {
    c.seed = (unsigned)++g_cases;
    Prep P; prepare(c, P);
    char shape[160];
    if (P.conv) snprintf(shape, sizeof shape, "B %d %dx%d Cin %d N %d ups %d nb %dx%d dens %d", c.B, c.Ho, c.Wo, c.Cin, c.N, c.ups, c.nb0, c.nb1, c.dens);
    else snprintf(shape, sizeof shape, "M %d N %d K %d nb %dx%d dens %d", c.M, c.N, c.K, c.nb0, c.nb1, c.dens);
    if (!P.pre_ok) { printf("%-46s %-17s %s: PRECONDITION FAIL (harness): worst sum %.0f, worst |pre-activation| %.0f units\n", c.name.c_str(), route_name(c.route), shape, P.worst, P.xworst); ++g_fail; return; }
    // the derived bound and the 1 % cap on the reference alone: the host's fp32 libm in the device's place
    size_t hdiff = 0, hbad = 0, nout = 0;
    if (P.approx) {
        for (size_t i = 0; i < P.nCv; ++i) if (P.isout[i]) {
            ++nout; const float d = P.host32[i], r = P.ref[i];
            if (memcmp(&d, &r, 4) != 0) { ++hdiff; if (!(std::fabs((double)d - r) <= P.tol[i])) ++hbad; }
        }
        if (hbad || hdiff * 100 > nout) { printf("%-46s %-17s %s: PRECONDITION FAIL (harness): host fp32 libm vs fp64: %zu of %zu differ, %zu beyond the bound\n", c.name.c_str(), route_name(c.route), shape, hdiff, nout, hbad); ++g_fail; return; }
    }
    if (!device) {
        if (P.approx) printf("%-46s %-17s %s: worst sum %.0f, |x| <= %.3f; host libm differs on %zu of %zu (%.3f %%), none beyond the bound  ok\n", c.name.c_str(), route_name(c.route), shape, P.worst, P.xworst * c.alpha * c.ascale, hdiff, nout, 100.0 * hdiff / nout);
        else printf("%-46s %-17s %s: worst sum %.0f  ok\n", c.name.c_str(), route_name(c.route), shape, P.worst);
        return;
    }
    if (c.knob) setenv(c.knob, "1", 1);
    void* dA = upload<void>(P.A); void* dW = upload<void>(P.W); void* dB = upload<void>(P.bias); void* dS = upload<void>(P.scl); void* dR = upload<void>(P.R);
    void* dC; CK(hipMalloc(&dC, P.nC * P.osz));
    float* dP = nullptr; if (c.gn) CK(hipMalloc(&dP, (P.nPart + 256) * 4));
    GemmP p; memset(&p, 0, sizeof(p));
    p.A = dA; p.W = dW; p.C = dC; p.bias = dB; p.scale = dS; p.R = dR; p.M = c.M; p.N = c.N; p.K = c.K;
    p.lda = P.conv ? 0 : P.lda; p.ldw = P.ldw; p.ldc = P.ldc; p.ldr = P.ldc;
    p.sA0 = P.sA0; p.sA1 = P.sA1; p.sW0 = P.sW0; p.sW1 = P.sW1; p.sC0 = P.sC0; p.sC1 = P.sC1; p.sR0 = P.sC0; p.sR1 = P.sC1;
    p.nb0 = c.nb0; p.nb1 = c.nb1; p.alpha = c.alpha; p.bias_mode = c.bias_mode; p.act = c.act; p.out_f32 = c.out_f32; p.swiglu = c.swiglu;
    if (P.conv) { p.Ho = c.Ho; p.Wo = c.Wo; p.Cin = c.Cin; p.ups = c.ups; p.patch = c.patch; }
    p.gn_part = dP;
    const int route = car_gemm_route(c.mode, c.amode, &p);
    if (route != c.route) {                      // asserted FIRST: a misrouted descriptor is not launched
        printf("%-46s %-17s %s: FAIL (route %s, expected %s; not launched)\n", c.name.c_str(), route_name(route), shape, route_name(route), route_name(c.route)); fflush(stdout);
        ++g_fail; if (c.knob) unsetenv(c.knob);
        for (void* q : {dA, dW, dB, dS, dR, dC, (void*)dP}) if (q) CK(hipFree(q));
        return;
    }
    std::vector<unsigned char> h[2]; std::vector<float> hp(P.nPart + 256);
    int rc = 0;
    for (int rep = 0; rep < 2; ++rep) {
        CK(hipMemset(dC, 0xff, P.nC * P.osz)); if (dP) CK(hipMemset(dP, 0xff, (P.nPart + 256) * 4));
        rc = car_launch_gemm(c.mode, c.amode, &p, 0);
        CK(hipDeviceSynchronize()); CK(hipGetLastError());
        h[rep].resize(P.nC * P.osz); CK(hipMemcpy(h[rep].data(), dC, P.nC * P.osz, hipMemcpyDeviceToHost));
    }
    std::string verdict; bool ok = true;
    auto failv = [&](const std::string& s) { if (ok) verdict = s; ok = false; };
    if (memcmp(h[0].data(), h[1].data(), h[0].size()) != 0) failv("BITS DIFFER between two runs");
    if (c.route < 0) {
        if (rc != c.route) failv("FAIL (return code " + std::to_string(rc) + ")");
        for (unsigned char b : h[0]) if (b != 0xff) { failv("FAIL (a refused call wrote to the output)"); break; }
        if (dP) { CK(hipMemcpy(hp.data(), dP, hp.size() * 4, hipMemcpyDeviceToHost)); const unsigned char* q = (const unsigned char*)hp.data(); for (size_t i = 0; i < hp.size() * 4; ++i) if (q[i] != 0xff) { failv("FAIL (a refused call wrote partials)"); break; } }
    } else {
        if (rc != 0) failv("FAIL (return code " + std::to_string(rc) + ")");
        size_t bad = 0, first = 0, ndiff = 0, gbad = 0;
        if (!P.approx) {
            if (memcmp(h[0].data(), P.expC.data(), h[0].size()) != 0)
                for (size_t i = 0; i < P.nC; ++i) if (memcmp(&h[0][i * P.osz], &P.expC[i * P.osz], P.osz) != 0) { if (!bad) first = i; ++bad; }
        } else {
            for (size_t i = 0; i < P.nC; ++i) {
                if (i < P.nCv && P.isout[i]) {
                    if (memcmp(&h[0][i * P.osz], &P.expC[i * P.osz], P.osz) == 0) continue;
                    ++ndiff; const float d = ld_out(h[0], i, P.osz);
                    if (!(std::fabs((double)d - P.ref[i]) <= P.tol[i])) { if (!bad) first = i; ++bad; }
                } else for (int b = 0; b < P.osz; ++b) if (h[0][i * P.osz + b] != 0xff) { ++gbad; break; }
            }
            if (ndiff * 100 > nout) failv("FAIL (" + std::to_string(ndiff) + " of " + std::to_string(nout) + " elements differ from the rounded fp64 reference: more than 1 %)");
            if (gbad) failv("FAIL (" + std::to_string(gbad) + " guard / gap elements written)");
        }
        if (bad) {
            char buf[256]; unsigned long long eb = 0, gb = 0; memcpy(&eb, &P.expC[first * P.osz], P.osz); memcpy(&gb, &h[0][first * P.osz], P.osz);
            snprintf(buf, sizeof buf, "FAIL (%zu elements wrong; first at element %zu of the allocation [%zu values + guard]: got %g (bits %llx) expected %g (bits %llx))", bad, first, P.nCv,
                     (double)ld_out(h[0], first, P.osz), gb, (double)ld_out(P.expC, first, P.osz), eb);
            failv(buf);
        }
        if (c.gn) {
            CK(hipMemcpy(hp.data(), dP, hp.size() * 4, hipMemcpyDeviceToHost));
            if (memcmp(hp.data(), P.expPart.data(), hp.size() * 4) != 0) failv("FAIL (GroupNorm partials differ from the integer sums of the stored values)");
            // ... and against gn_partial_vec_kernel's pass over the stored output (chunks of 256 pixels in row order, not tiles): per (image, channel) totals, exact in double
            const int HW = c.Ho * c.Wo, nchunk = HW / GN_CHUNK; float* dP2; CK(hipMalloc(&dP2, P.nPart * 4));
            hipLaunchKernelGGL(gn_partial_vec_kernel, dim3(nchunk, c.B), dim3(256), (size_t)256 * 16 * 4, 0, (const bf16_t*)dC, dP2, HW, c.N);
            CK(hipDeviceSynchronize()); CK(hipGetLastError());
            std::vector<float> hp2(P.nPart); CK(hipMemcpy(hp2.data(), dP2, P.nPart * 4, hipMemcpyDeviceToHost)); CK(hipFree(dP2));
            for (int b = 0; b < c.B && ok; ++b) for (int j = 0; j < 2 * c.N; ++j) {
                double s1 = 0, s2 = 0; for (int k = 0; k < nchunk; ++k) { s1 += hp[((size_t)b * nchunk + k) * 2 * c.N + j]; s2 += hp2[((size_t)b * nchunk + k) * 2 * c.N + j]; }
                if (s1 != s2) { failv("FAIL (GroupNorm partials: totals differ from gn_partial_vec_kernel's)"); break; }
            }
        }
        if (ok && P.approx) { char buf[96]; snprintf(buf, sizeof buf, "OK (%zu of %zu differ by one ulp: %.3f %%)", ndiff, nout, 100.0 * ndiff / nout); verdict = buf; }
    }
    if (ok && verdict.empty()) verdict = "OK";
    printf("%-46s %-17s %s: worst sum %.0f  %s\n", c.name.c_str(), route_name(route), shape, P.worst, verdict.c_str());
    fflush(stdout);
    if (!ok) ++g_fail;
    if (c.knob) unsetenv(c.knob);
    for (void* q : {dA, dW, dB, dS, dR, dC, (void*)dP}) if (q) CK(hipFree(q));
}

static Case plain(const char* name, int mode, int route, int M, int N, int K) { Case c; c.name = name; c.mode = mode; c.route = route; c.M = M; c.N = N; c.K = K; return c; }
static Case conv(const char* name, int mode, int amode, int route, int B, int Ho, int Wo, int Cin, int N, int ups) {
    Case c; c.name = name; c.mode = mode; c.amode = amode; c.route = route; c.B = B; c.Ho = Ho; c.Wo = Wo; c.Cin = Cin; c.N = N; c.ups = ups; return c;
}

int main(int argc, char** argv) {
    const std::string md = argc > 1 ? argv[1] : "quick";
    if (md != "quick" && md != "selftest") { printf("usage: gemm_check [quick | selftest]\n"); return 2; }
    const bool device = md == "quick";
    const auto t0 = std::chrono::steady_clock::now();
    for (const char* k : {"CAR_CONV_HALO128", "CAR_GEMM_V1", "CAR_NO_HALO", "CAR_CONV_LINEAR", "CAR_GN_UNFUSED"}) unsetenv(k);
    const int REG = CAR_ROUTE_BF16_REG, GLDS = CAR_ROUTE_BF16_GLDS, MFMA = CAR_ROUTE_F32_MFMA, VALU = CAR_ROUTE_F32_VALU;
    std::vector<Case> L;
    Case c;
    // ================================================================= gemm_bf16_kernel (128 x 128 x 32): ragged second m- and n-tiles
    L.push_back(plain("reg plain K32 (one step, no prefetch)", 1, REG, 130, 136, 32));
    L.push_back(plain("reg plain K96 (double buffer wraps)", 1, REG, 130, 136, 96));
    c = plain("reg EP_VEC bias_n + R, alpha 2", 1, REG, 130, 136, 96); c.bias_mode = BIAS_N; c.resid = true; c.alpha = 2.f; L.push_back(c);
    c.name = "reg EP_VEC bias_n + R, alpha 2, out_f32"; c.out_f32 = 1; L.push_back(c);
    c = plain("reg EP_SCALAR N 133 bias_m + scale + R", 1, REG, 130, 133, 96); c.bias_mode = BIAS_M; c.scale = true; c.resid = true; L.push_back(c);
    c.name = "reg EP_SCALAR N 133 bias_m + scale + R, out_f32"; c.out_f32 = 1; L.push_back(c);
    c = plain("reg batched 2x3, sC % 8 != 0 (scalar per batch)", 1, REG, 70, 72, 64); c.nb0 = 2; c.nb1 = 3; c.padA = 8; c.padW = 16; c.padC = 3; c.bias_mode = BIAS_N; c.resid = true; L.push_back(c);
    c.name = "reg batched 2x3, aligned strides"; c.padC = 8; L.push_back(c);
    c = conv("reg conv3 linear row order", 1, AMODE_CONV3, REG, 2, 16, 32, 32, 40, 0); c.bias_mode = BIAS_N; c.resid = true; L.push_back(c);
    c.name = "reg conv3 patch row order"; c.patch = 1; L.push_back(c);
    c.name = "reg conv3 patch asked, CAR_CONV_LINEAR"; c.knob = "CAR_CONV_LINEAR"; L.push_back(c);
    c = conv("reg conv3 ups 6x5 -> 12x10", 1, AMODE_CONV3, REG, 2, 12, 10, 32, 40, 1); c.bias_mode = BIAS_N; c.resid = true; L.push_back(c);
    c = conv("reg conv3s2 10x14 -> 5x7 (odd output map)", 1, AMODE_CONV3S2, REG, 2, 5, 7, 32, 40, 0); c.bias_mode = BIAS_N; L.push_back(c);
    c = conv("reg conv3s2 8x12 -> 4x6 (even output map)", 1, AMODE_CONV3S2, REG, 2, 4, 6, 32, 40, 0); c.bias_mode = BIAS_N; L.push_back(c);
    c = conv("reg conv3 at a halo shape, CAR_NO_HALO", 1, AMODE_CONV3, REG, 1, 16, 16, 128, 128, 0); c.bias_mode = BIAS_N; c.resid = true; c.patch = 1; c.knob = "CAR_NO_HALO"; L.push_back(c);
    c.name = "reg conv3 at a halo shape, CAR_GEMM_V1"; c.knob = "CAR_GEMM_V1"; L.push_back(c);
    c = conv("reg conv3 ups at a halo shape, CAR_NO_HALO", 1, AMODE_CONV3, REG, 2, 32, 16, 128, 128, 1); c.bias_mode = BIAS_N; c.patch = 1; c.knob = "CAR_NO_HALO"; L.push_back(c);
    // ================================================================= EP_SWIGLU: N = 256 weight rows = two n-tiles -> 128 outputs, ragged M
    for (int kind = 1; kind <= 2; ++kind)
        for (int el = 0; el < 2; ++el) {
            c = plain("", 1, REG, 130, 256, 96); c.name = std::string("swiglu ") + (kind == 1 ? "1 (SiLU)" : "2 (tanh-GELU)") + (el ? ", ldc 131: element branch" : ", 16-byte branch");
            c.swiglu = kind; c.ascale = 0.125f; c.dens = 16; c.xmax = 24; if (el) c.ldc = 131; L.push_back(c);
        }
    // dense operands: gate pre-activations are integers (the reached maximum is 69; beyond +-88 expf overflows where the true SiLU is still a normal number)
    c = plain("swiglu 1 dense operands, integer gate <= 69", 1, REG, 130, 256, 64); c.swiglu = 1; c.dens = 1; c.xmax = 80; L.push_back(c);
    // ================================================================= activations: x = (acc + bias_i) / 8, |x| <= 3.5
    for (int act = ACT_GELU_ERF; act <= ACT_SILU; ++act)
        for (int sc = 0; sc < 2; ++sc) {
            c = plain("", 1, REG, 130, sc ? 133 : 136, 96); c.name = std::string(act == ACT_GELU_ERF ? "GELU-erf" : act == ACT_GELU_TANH ? "GELU-tanh" : "SiLU") + (sc ? " EP_SCALAR N 133, out_f32" : " EP_VEC");
            c.act = act; c.alpha = 0.125f; c.dens = 16; c.brange = 4; c.bias_mode = BIAS_N; c.xmax = 28; c.out_f32 = sc; L.push_back(c);
        }
    // the saturated sides: x = (acc + bias_i) / 8 spread by a large bias over [-30.5, 30.5] (SiLU) or [-3, 30.5] (the GELU forms: no cancellation for x > 0)
    for (int act = ACT_GELU_ERF; act <= ACT_SILU; ++act)
        for (int sc = 0; sc < 2; ++sc) {
            c = plain("", 1, REG, 130, sc ? 133 : 136, 96); c.name = std::string(act == ACT_GELU_ERF ? "GELU-erf" : act == ACT_GELU_TANH ? "GELU-tanh" : "SiLU") + (act == ACT_SILU ? " wide |x| <= 30.5" : " wide -3 <= x <= 30.5") + (sc ? " EP_SCALAR bias_m, out_f32" : " EP_VEC bias_n");
            c.act = act; c.alpha = 0.125f; c.dens = 16; c.brange = 220; c.bpos = act != ACT_SILU; c.bias_mode = sc ? BIAS_M : BIAS_N; c.xmax = 244; c.xneg = act != ACT_SILU ? 24 : 244; c.out_f32 = sc; L.push_back(c);
        }
    // ================================================================= the order of the rounding points: sums far beyond 8 bits, replayed in float
    c = plain("big EP_VEC bias_n, scale, R, alpha 2", 1, REG, 130, 136, 96); c.big = true; c.bias_mode = BIAS_N; c.scale = true; c.resid = true; c.alpha = 2.f; L.push_back(c);
    c = plain("big EP_SCALAR bias_m, scale, R, alpha 1/2", 1, REG, 130, 133, 96); c.big = true; c.bias_mode = BIAS_M; c.scale = true; c.resid = true; c.alpha = 0.5f; L.push_back(c);
    // SwiGLU: accumulators up to about +-1000 in units of 1/16 (about a fifth beyond 256 units: rnd(acc) of gate and linear column is not the identity), |gate| < 88
    c = plain("big swiglu 1, |acc| far beyond 8 bits, 16-byte branch", 1, REG, 130, 256, 256); c.big = true; c.swiglu = 1; c.ascale = 0.0625f; c.xmax = 1400; L.push_back(c);
    c.name = "big swiglu 1, |acc| far beyond 8 bits, element branch"; c.ldc = 131; L.push_back(c);
    // ================================================================= gemm_bf16_glds_kernel (256 x 128 x 64, three-stage ring): tiles == 512 exactly
    c = plain("glds plain K512 (8 stages) 16x8 batches", 1, GLDS, 257, 129, 512); c.nb0 = 16; c.nb1 = 8; c.bias_mode = BIAS_N; L.push_back(c);
    c = plain("glds plain K576 (9 stages) 16x8 batches", 1, GLDS, 257, 129, 576); c.nb0 = 16; c.nb1 = 8; c.bias_mode = BIAS_N; L.push_back(c);
    c = plain("one batch fewer (tiles 508): register kernel", 1, REG, 257, 129, 512); c.nb0 = 127; c.nb1 = 1; c.bias_mode = BIAS_N; L.push_back(c);
    c = plain("glds plain K512 N136 EP_VEC + R", 1, GLDS, 257, 136, 512); c.nb0 = 16; c.nb1 = 8; c.bias_mode = BIAS_N; c.resid = true; L.push_back(c);
    c = conv("glds conv3 Cin64 12x20, 256 batches", 1, AMODE_CONV3, GLDS, 1, 12, 20, 64, 136, 0); c.nb0 = 256; c.bias_mode = BIAS_N; c.resid = true; L.push_back(c);
    c = conv("glds conv3 Cin64 ups 6x10 -> 12x20, 256 batches", 1, AMODE_CONV3, GLDS, 1, 12, 20, 64, 136, 1); c.nb0 = 256; c.bias_mode = BIAS_N; L.push_back(c);
    // ================================================================= the LDS-halo convolutions: conv3_halo64_kernel, and conv3_halo_kernel through CAR_CONV_HALO128
    for (int old = 0; old < 2; ++old) {
        const int rt = old ? CAR_ROUTE_HALO128 : CAR_ROUTE_HALO64; const char* kn = old ? "CAR_CONV_HALO128" : nullptr; const std::string pf = old ? "halo128 " : "halo64 ";
        c = conv("", 1, AMODE_CONV3, rt, 2, 48, 32, 128, 128, 0); c.name = pf + "2 x 48x32 128->128 bias + R"; c.bias_mode = BIAS_N; c.resid = true; c.patch = 1; c.knob = kn; L.push_back(c);
        c = conv("", 1, AMODE_CONV3, rt, 2, 48, 32, 256, 256, 1); c.name = pf + "2 x 48x32 256->256 ups, bias pointer with BIAS_NONE"; c.bias_ptr = true; c.patch = 1; c.knob = kn; L.push_back(c);
        c = conv("", 1, AMODE_CONV3, rt, 2, 48, 32, 256, 128, 0); c.name = pf + "2 x 48x32 256->128 bias"; c.bias_mode = BIAS_N; c.patch = 1; c.knob = kn; L.push_back(c);
        c = conv("", 1, AMODE_CONV3, rt, 1, 16, 16, 128, 256, 0); c.name = pf + "one 16x16 image (ring all padding) 128->256 bias + R"; c.bias_mode = BIAS_N; c.resid = true; c.patch = 1; c.knob = kn; L.push_back(c);
        c = conv("", 1, AMODE_CONV3, rt, 1, 16, 16, 256, 128, 1); c.name = pf + "one 16x16 image ups 256->128 R, BIAS_NONE + pointer"; c.bias_ptr = true; c.resid = true; c.patch = 1; c.knob = kn; L.push_back(c);
    }
    c = conv("halo64 gn_part 2 x 48x32 128->128 bias + R", 1, AMODE_CONV3, CAR_ROUTE_HALO64, 2, 48, 32, 128, 128, 0); c.bias_mode = BIAS_N; c.resid = true; c.patch = 1; c.gn = true; L.push_back(c);
    c = conv("halo64 gn_part 2 x 48x32 256->256 ups bias", 1, AMODE_CONV3, CAR_ROUTE_HALO64, 2, 48, 32, 256, 256, 1); c.bias_mode = BIAS_N; c.patch = 1; c.gn = true; L.push_back(c);
    // ================================================================= refusals: negative route, non-zero return, nothing written
    c = conv("refusal: gn_part with CAR_GN_UNFUSED", 1, AMODE_CONV3, CAR_ROUTE_REFUSE_GN, 1, 16, 16, 128, 128, 0); c.bias_mode = BIAS_N; c.gn = true; c.knob = "CAR_GN_UNFUSED"; L.push_back(c);
    c.name = "refusal: gn_part with CAR_CONV_HALO128"; c.knob = "CAR_CONV_HALO128"; L.push_back(c);
    c = conv("refusal: gn_part on an ineligible shape (Cin 32)", 1, AMODE_CONV3, CAR_ROUTE_REFUSE_GN, 1, 16, 16, 32, 128, 0); c.bias_mode = BIAS_N; c.gn = true; L.push_back(c);
    L.push_back(plain("refusal: bf16 K 48 (K % 32 != 0)", 1, CAR_ROUTE_REFUSE_K, 130, 136, 48));
    L.push_back(conv("refusal: bf16 conv Cin 16 (K 144)", 1, AMODE_CONV3, CAR_ROUTE_REFUSE_K, 1, 6, 5, 16, 40, 0));
    L.push_back(plain("refusal: fp32 K 24 (K % 16 != 0)", 0, CAR_ROUTE_REFUSE_K, 66, 70, 24));
    // ================================================================= fp32: gemm_f32_mfma_kernel (128 x 128 x 16) and gemm_f32_kernel (64 x 64 x 16)
    L.push_back(plain("f32 mfma plain K16", 0, MFMA, 130, 136, 16));
    c = plain("f32 mfma plain K48 bias_n, scale, R, alpha 2", 0, MFMA, 130, 136, 48); c.bias_mode = BIAS_N; c.scale = true; c.resid = true; c.alpha = 2.f; L.push_back(c);
    c = plain("f32 mfma plain K48 ldc 137 (scalar stores) bias_m", 0, MFMA, 130, 136, 48); c.ldc = 137; c.bias_mode = BIAS_M; c.resid = true; L.push_back(c);
    c = plain("f32 mfma batched 2x3, odd zC (scalar stores)", 0, MFMA, 70, 72, 48); c.nb0 = 2; c.nb1 = 3; c.padA = 4; c.padW = 8; c.padC = 1; c.bias_mode = BIAS_N; c.resid = true; L.push_back(c);
    c.name = "f32 mfma batched 2x3, aligned strides"; c.padC = 4; L.push_back(c);
    L.push_back(conv("f32 mfma conv3 12x11 Cin16", 0, AMODE_CONV3, MFMA, 1, 12, 11, 16, 136, 0));
    c = conv("f32 mfma conv3 ups 6x5 -> 12x10", 0, AMODE_CONV3, MFMA, 2, 12, 10, 16, 40, 1); c.bias_mode = BIAS_N; c.resid = true; L.push_back(c);
    c = conv("f32 mfma conv3s2 10x14 -> 5x7", 0, AMODE_CONV3S2, MFMA, 2, 5, 7, 16, 40, 0); c.bias_mode = BIAS_N; L.push_back(c);
    L.push_back(conv("f32 mfma conv3s2 8x12 -> 4x6", 0, AMODE_CONV3S2, MFMA, 2, 4, 6, 16, 40, 0));
    c = plain("f32 valu plain K16 via lda 17", 0, VALU, 66, 70, 16); c.lda = 17; L.push_back(c);
    c = plain("f32 valu plain K48 via lda 49 bias_n, scale, R", 0, VALU, 66, 70, 48); c.lda = 49; c.bias_mode = BIAS_N; c.scale = true; c.resid = true; c.alpha = 2.f; L.push_back(c);
    c = plain("f32 valu plain M130 N136 K48 via lda 50 bias_m", 0, VALU, 130, 136, 48); c.lda = 50; c.bias_mode = BIAS_M; L.push_back(c);
    c = plain("f32 valu batched 2x3 via lda 49", 0, VALU, 70, 72, 48); c.lda = 49; c.nb0 = 2; c.nb1 = 3; c.padA = 4; c.padW = 8; c.padC = 1; c.bias_mode = BIAS_N; c.resid = true; L.push_back(c);
    // a convolution cannot reach the VALU kernel through Cin % 4 != 0 any more (K = 9 Cin must be a multiple of 16): it gets there through ldw % 4 != 0
    c = conv("f32 valu conv3 12x11 Cin16 via ldw 145", 0, AMODE_CONV3, VALU, 1, 12, 11, 16, 136, 0); c.ldw = 145; L.push_back(c);
    c = conv("f32 valu conv3 ups via ldw 146", 0, AMODE_CONV3, VALU, 2, 12, 10, 16, 40, 1); c.ldw = 146; c.bias_mode = BIAS_N; c.resid = true; L.push_back(c);
    c = conv("f32 valu conv3s2 10x14 -> 5x7 via ldw 147", 0, AMODE_CONV3S2, VALU, 2, 5, 7, 16, 40, 0); c.ldw = 147; c.bias_mode = BIAS_N; L.push_back(c);

    for (const Case& cs : L) run(cs, device);
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%d cases (%s), wall %.1f s\n", g_cases, md.c_str(), wall);
    if (g_fail) { printf("%d check(s) FAILED\n", g_fail); return 1; }
    printf(device ? "all checks passed\n" : "selftest passed\n");
    return 0;
}
