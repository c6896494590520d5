// experiments/decode_check.hip — the bf16 decode-step kernels of controlar_amd/csrc/decode2.hip against EXACT integer references, through the real launchers:
// dec_gemm_kernel (every tile shape x epilogue x weight format x norm form the launcher accepts), rmsnorm2_kernel, and the two writers of the packed KV cache
// (the EPI_QKV epilogue and prefill_rope_kv2_kernel).  Every dec_gemm case asserts its car_dec_gemm_route value (I, J, WAVES, F8, NORM) before it launches.
//
// Method (that of gemm_check.hip).  Activations, weights, residuals and control tokens are small hashed integers (times a power of two), wscale rows are powers
// of two, RoPE tables hold dyadic (cos, sin) pairs — so every product and every partial sum is exact in fp32 in ANY order (the harness checks, per output element,
// sum |x w| < 2^24, and the same for the sums of squares behind ssq_out) and the K-split, the fold order and FMA contraction cannot matter.  The reference then
// replays the documented rounding points (bf16 RNE; e4m3fn RNE with the +-448 clamp for W8A8 activations and e4m3 KV rows) and has ONE possible result.
// All buffers of a case live in one arena that is poisoned with 0xff bytes (256 guard bytes between buffers); after the launch the WHOLE arena is compared with
// the expected image: the inputs must be unchanged, the guards, the cache rows at positions other than *pos, rows >= M of the last 16-row block of every output
// and of ssq_out must still be poison.  Rows >= M of a packed X hold NaN patterns.
// RMSNorm forms: rsqrtf is not exact, so the rows are "sign rows" v[m][k] = +-2^a(m): rnd(v * rstd) = +-1 for every float within 2 ulp of the correctly rounded
// rstd (checked by the harness for eps = 1e-5 and 0), x = +-w[k] is an integer again and the GEMM behind it is exact.  The per-row exponent makes a row that used
// another row's statistics visible.  The partials of NORM 2 / 3 come from a preceding EPI_RESID launch with ssq_out, as in the engine.
// The only bound is SwiGLU's, taken from gemm_check.hip: expected = rounded fp64 function, a difference of at most ulp(gate) |c| + ulp(out) on at most 1 % of the
// elements, pre-activations within 30.5 (the dense case, whose sums are far beyond 8 bits so that the pre-gate rounding matters: within 80).
// Before each launch the byte extents the launch may touch (layout formulas of decode2.hip's header) are asserted to lie inside the case's buffers: a wrong case
// fails on the host.  Every HIP call is checked; the process exits on the first HIP error.
//   quick      all device checks; one line per case; ends with "all checks passed"
//   selftest   host only, no HIP call: every case's data, reference and preconditions, the SwiGLU bound and the 1 % cap with the host's fp32 libm in the
//              device's place, the e4m3 encoder against all 256 codes, the layout formulas against the attn2_edge_* lane maps, and car_pick_gemm_cfg followed by
//              car_dec_gemm_route over the engine's linears (nothing the engine would ask for may be refused)
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I controlar_amd/csrc experiments/decode_check.hip -o experiments/decode_check && experiments/decode_check quick
#include "../controlar_amd/csrc/decode2.hip"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)
#define HOSTCHECK(c, ...) do { if (!(c)) { printf("PRECONDITION FAIL (harness) %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(3); } } while (0)

static bool g_dev = false;
static int g_fail = 0, g_cases = 0, g_launches = 0;
static char* g_arena = nullptr;
static const size_t ARENA = (size_t)48 << 20, GUARD = 256;

static unsigned hsh(unsigned a, unsigned b, unsigned seed) {
    unsigned x = a * 2654435761u + b * 0x85ebca6bu + seed * 0x9e3779b9u; x ^= x >> 15; x *= 2246822519u; x ^= x >> 13; x *= 3266489917u; x ^= x >> 16; return x;
}
static float rbf(float v) { return bf2f(f2bf(v)); }
static double ulp_bf16(double v) { if (v == 0 || !(std::fabs(v) < 1e300)) return 0; int e; (void)std::frexp(std::fabs(v), &e); return std::ldexp(1.0, e - 8); }

// ---------------------------------------------------------------------------------------------------------------- OCP e4m3fn (reference encoder, f8_check.hip)
static float e4m3_decode(unsigned char v) {
    const int e = (v >> 3) & 15, m = v & 7; const float s = (v & 0x80) ? -1.f : 1.f;
    if (e == 15 && m == 7) return NAN;
    return s * (e == 0 ? (float)m * 0.001953125f : ldexpf(1.0f + (float)m / 8.0f, e - 7));
}
static float e4m3_round(float f) {        // round-to-nearest-even, saturating at 448: the value the code stands for
    if (f != f) return NAN;
    const float s = std::signbit(f) ? -1.f : 1.f; float a = fabsf(f);
    if (a >= 448.f) return s * 448.f;
    if (a < 0.015625f) return s * nearbyintf(a * 512.0f) / 512.0f;
    int e; const float m = frexpf(a, &e);
    const float r = ldexpf(nearbyintf(m * 16.0f) / 16.0f, e);
    return s * (r > 448.f ? 448.f : r);
}
static unsigned char e4m3_encode(float f) {
    if (f != f) return 0x7f;
    const unsigned char sg = std::signbit(f) ? 0x80 : 0;
    const float r = fabsf(e4m3_round(f));
    if (r < 0.015625f) return sg | (unsigned char)(int)(r * 512.0f);
    int e; const float m = frexpf(r, &e);                // r = m 2^e, m in [0.5, 1)
    return sg | (unsigned char)(((e + 6) << 3) | ((int)(m * 16.0f) - 8));
}

// ---------------------------------------------------------------------------------------------------------------- layouts (decode2.hip header)
static size_t xp_off(int m, int k, int K) { return ((((size_t)(m >> 4) * (K >> 5) + (k >> 5)) * 64 + ((k & 31) >> 3) * 16 + (m & 15)) << 3) + (k & 7); }
static size_t w8_off(int n, int k, int K) { return ((((((size_t)(n >> 4) * (K >> 6) + (k >> 6)) * 64 + (((k & 31) >> 3) * 16 + (n & 15))) * 2 + ((k >> 5) & 1)) << 3) + (k & 7)); }
static void v_code(int p, int& qv, int& ev) { const int w = p & 31; qv = w < 16 ? (w >> 2) : ((w - 16) >> 2); ev = w < 16 ? (w & 3) : (4 + ((w - 16) & 3)); }
static size_t k_off(int p, int d) { return ((size_t)(p >> 4) * 2 + (d >> 5)) * 512 + ((((d & 31) >> 3) * 16 + (p & 15)) << 3) + (d & 7); }
static size_t v_off(int p, int d) { int qv, ev; v_code(p, qv, ev); return ((size_t)(p >> 5) * 4 + (d >> 4)) * 512 + ((qv * 16 + (d & 15)) << 3) + ev; }
static size_t k8_off(int p, int d) { return (size_t)(p >> 4) * 1024 + ((((d & 31) >> 3) * 16 + (p & 15)) << 4) + (d >> 5) * 8 + (d & 7); }
static size_t v8_off(int p, int d) { int qv, ev; v_code(p, qv, ev); return (size_t)(p >> 5) * 2048 + (d >> 5) * 1024 + ((qv * 16 + (d & 15)) << 4) + ((d >> 4) & 1) * 8 + ev; }

// dyadic (cos, sin) pairs: not rotations, the kernels do not care
static void rope_pair(int pos, int pr, float& c, float& s) {
    static const float T[4][2] = {{1.f, 0.f}, {0.f, -1.f}, {0.5f, 0.5f}, {0.75f, -0.25f}};
    const unsigned h = hsh((unsigned)pos, (unsigned)pr, 77u) & 3u; c = T[h][0]; s = T[h][1];
}

// ---------------------------------------------------------------------------------------------------------------- one arena image per case
struct Sess {
    std::vector<unsigned char> img; std::vector<std::pair<size_t, size_t>> reg;
    size_t alloc(size_t bytes) { const size_t off = (img.size() + 255) & ~(size_t)255; img.resize(off + bytes + GUARD, 0xff); reg.push_back({off, bytes}); HOSTCHECK(img.size() <= ARENA, "arena too small"); return off; }
    size_t size_of(size_t off) const { for (auto& r : reg) if (r.first == off) return r.second; return 0; }
    // the launch may touch `need` bytes from `off`: inside the buffer allocated there
    void extent(const char* what, size_t off, size_t need) const { HOSTCHECK(need <= size_of(off), "extent of %s: needs %zu bytes, the buffer has %zu", what, need, size_of(off)); }
    template <typename T> T* dp(size_t off) const { return (T*)((g_dev ? g_arena : (char*)0x100000000ull) + off); }
    void upload() const { CK(hipMemcpy(g_arena, img.data(), img.size(), hipMemcpyHostToDevice)); }
    void download(std::vector<unsigned char>& got) const { got.resize(img.size()); CK(hipDeviceSynchronize()); CK(hipGetLastError()); CK(hipMemcpy(got.data(), g_arena, img.size(), hipMemcpyDeviceToHost)); }
};
static void put_bf(std::vector<unsigned char>& im, size_t off, size_t i, float v) { const bf16_t b = f2bf(v); HOSTCHECK(bf2f(b) == v || v != v, "value %g is not a bf16 number", (double)v); memcpy(&im[off + i * 2], &b, 2); }
static void put_f32(std::vector<unsigned char>& im, size_t off, size_t i, float v) { memcpy(&im[off + i * 4], &v, 4); }
static void put_i32(std::vector<unsigned char>& im, size_t off, size_t i, int v) { memcpy(&im[off + i * 4], &v, 4); }

struct Approx { size_t off = 0; std::vector<float> ref, tol, host32; std::vector<unsigned char> isout; };   // per bf16 element of the buffer at `off`

// compares the arena with the expected image; elements of the approximate buffer (SwiGLU) under the derived bound
static std::string compare(const std::vector<unsigned char>& got, const std::vector<unsigned char>& exp, const Sess& S, const Approx* ap, const std::vector<std::pair<size_t, const char*>>& names) {
    size_t ndiff = 0, nout = 0, bad = 0;
    std::vector<unsigned char> g2;
    const std::vector<unsigned char>* g = &got;
    if (ap) {
        g2 = got;
        for (size_t i = 0; i < ap->isout.size(); ++i) if (ap->isout[i]) {
            ++nout;
            if (memcmp(&got[ap->off + i * 2], &exp[ap->off + i * 2], 2) == 0) continue;
            ++ndiff; bf16_t b; memcpy(&b, &got[ap->off + i * 2], 2);
            if (!(std::fabs((double)bf2f(b) - ap->ref[i]) <= ap->tol[i])) ++bad; else memcpy(&g2[ap->off + i * 2], &exp[ap->off + i * 2], 2);
        }
        g = &g2;
    }
    char buf[320];
    if (memcmp(g->data(), exp.data(), exp.size()) != 0) {
        size_t first = 0, n = 0; for (size_t i = 0; i < exp.size(); ++i) if ((*g)[i] != exp[i]) { if (!n) first = i; ++n; }
        const char* nm = "?"; size_t base = 0, sz = 0; for (size_t r = 0; r < S.reg.size(); ++r) if (first >= S.reg[r].first) { base = S.reg[r].first; sz = S.reg[r].second; for (auto& q : names) if (q.first == base) nm = q.second; }
        snprintf(buf, sizeof buf, "FAIL (%zu bytes differ; first at byte %zu of %s [%zu bytes + guard]: got %02x expected %02x)", n, first - base, nm, sz, (*g)[first], exp[first]);
        return buf;
    }
    if (ap && ndiff * 100 > nout) { snprintf(buf, sizeof buf, "FAIL (%zu of %zu elements differ from the rounded fp64 reference: more than 1 %%)", ndiff, nout); return buf; }
    if (ap) { snprintf(buf, sizeof buf, "OK (%zu of %zu within the SwiGLU bound: %.3f %%)", ndiff, nout, 100.0 * ndiff / (nout ? nout : 1)); return buf; }
    return "OK";
}

// ---------------------------------------------------------------------------------------------------------------- dec_gemm cases
struct GC {
    std::string name; int cfg = 111, epi = EPI_LOGITS, f8 = 0, M = 1, N = 64, K = 64;
    int norm = 0;                 // the NORM form the case must be routed to
    int src = 0;                  // 0: packed X of hashed integers; 1: sign rows through the norm path (norm 0: rmsnorm2_kernel -> packed xn -> NORM 0)
    int staged_ok = 1, w_nt = 1, pf = 0; bool ssq = false; int pos = 0, kv8 = 0; bool dense = false;
    bool tiny = false;            // EPI_QKV: wscale rows 2^-129 .. 2^-133, so that q lands in the bf16 subnormal range, the only place where rnd(r) / 8 and rnd(r / 8) differ
    bool gather = false, add = false, poslast = false, nhout = false; float eps = 1e-5f; int rI = 2;       // rI: I of the EPI_RESID producer of the partials (NORM 2 / 3)
};
static const int SA = 96, HH = 2, DIM = 128, NTOK = 3;

static void ref_gemm(const std::vector<int>& X, const std::vector<signed char>& W, int M, int N, int K, std::vector<long>& acc, std::vector<long>& sab) {
    acc.assign((size_t)M * N, 0); sab.assign((size_t)M * N, 0);
    unsigned nthr = std::thread::hardware_concurrency(); if (nthr < 1) nthr = 1; if (nthr > 16) nthr = 16; if ((long)M * N * K < (4L << 20)) nthr = 1;
    auto work = [&](unsigned t) {
        for (long i = t; i < (long)M * N; i += nthr) {
            const int* x = &X[(size_t)(i / N) * K]; const signed char* w = &W[(size_t)(i % N) * K];
            int a = 0, s = 0; for (int k = 0; k < K; ++k) { const int p = x[k] * w[k]; a += p; s += p < 0 ? -p : p; }
            acc[i] = a; sab[i] = s;
        }
    };
    if (nthr == 1) { work(0); return; }
    std::vector<std::thread> th; for (unsigned t = 0; t < nthr; ++t) th.emplace_back(work, t); for (auto& t : th) t.join();
}

static void fill_w(Sess& S, size_t offW, size_t offS, const std::vector<signed char>& W, const std::vector<float>& sc, int N, int K, int f8) {
    for (int n = 0; n < N; ++n) for (int k = 0; k < K; ++k) {
        if (f8) { const unsigned char b = e4m3_encode((float)W[(size_t)n * K + k]); HOSTCHECK(e4m3_decode(b) == (float)W[(size_t)n * K + k], "weight not an e4m3 number"); S.img[offW + w8_off(n, k, K)] = b; }
        else put_bf(S.img, offW, xp_off(n, k, K), (float)W[(size_t)n * K + k]);
    }
    if (f8) for (int n = 0; n < N; ++n) put_f32(S.img, offS, n, sc[n]);
}
static void route_str(char* b, size_t n, int rc, const DecGemmRoute& r) { if (rc) snprintf(b, n, "refused"); else snprintf(b, n, "I%d J%d W%-2d F8 %d NORM %d", r.I, r.J, r.WAVES, r.F8, r.NORM); }

static int launch(const GemmDP& p, int epi, int cfg, int staged_ok) { ++g_launches; return car_launch_dec_gemm_cfg_ex(&p, epi, cfg, staged_ok, 0); }

// extents of one dec_gemm launch (bytes from each pointer), asserted inside the buffers of the session
static void gemm_extents(const Sess& S, const GemmDP& p, int epi, const DecGemmRoute& r, int pos, int n_idx_rows) {
    auto off = [&](const void* q) { return (size_t)((const char*)q - S.dp<char>(0)); };
    const int Mb = (p.M + 15) / 16, IW = r.I >= 2 ? 2 : 1;
    S.extent("W", off(p.W), (size_t)p.N * p.K * (r.F8 ? 1 : 2));
    if (r.F8) S.extent("wscale", off(p.wscale), (size_t)p.N * 4);
    if (r.NORM == 0) S.extent("X", off(p.X), (size_t)Mb * 16 * p.K * 2);
    if (r.NORM) S.extent("nw", off(p.nw), (size_t)p.K * 2);
    if (r.NORM == 1) {
        if (p.nidx) { S.extent("nidx", off(p.nidx), (size_t)p.M * 4); S.extent("nemb", off(p.nemb), (size_t)n_idx_rows * p.K * 2); } else S.extent("nh_in", off(p.nh_in), (size_t)p.M * p.K * 2);
        if (p.nadd) { const int tk = pos - p.nT + 1; HOSTCHECK(tk >= 0 && tk < p.n_tok, "control token index"); S.extent("nctrl", off(p.nctrl), (size_t)p.M * p.n_tok * p.K * 2); }
        if (p.nh_out) S.extent("nh_out", off(p.nh_out), (size_t)p.M * p.K * 2);
    }
    if (r.NORM >= 2) { S.extent("nh_in", off(p.nh_in), (size_t)p.M * p.K * 2); S.extent("ssq_in", off(p.ssq_in), (size_t)p.M * p.ssq_np * 4); }
    if (epi == EPI_LOGITS) S.extent("outf", off(p.outf), (size_t)p.M * p.N * 4);
    if (epi == EPI_RESID) { S.extent("h", off(p.h), (size_t)p.M * p.N * 2); if (p.ssq_out) { HOSTCHECK(p.N / (16 * IW) <= p.ssq_ld, "ssq_ld"); S.extent("ssq_out", off(p.ssq_out), (size_t)p.M * p.ssq_ld * 4); } }
    if (epi == EPI_SWIGLU) { HOSTCHECK(p.N % 64 == 0, "SwiGLU packs N/2 in 32-column chunks"); S.extent("outp", off(p.outp), (size_t)Mb * 16 * (p.N / 2) * 2); }
    if (epi == EPI_QKV) {
        HOSTCHECK(p.N == 3 * p.dim && p.dim == p.H * 64 && pos >= 0 && pos < p.SA && p.SA % 32 == 0, "QKV geometry");
        S.extent("pos", off(p.pos), 4); S.extent("rope", off(p.rope), (size_t)(pos + 1) * 64 * 4); S.extent("qout", off(p.qout), (size_t)p.M * p.H * 64 * 2);
        S.extent("kc", off(p.kc), (size_t)p.M * p.H * p.SA * 64 * (p.kv8 ? 1 : 2)); S.extent("vc", off(p.vc), (size_t)p.M * p.H * p.SA * 64 * (p.kv8 ? 1 : 2));
    }
    if (p.pf_wgs > 0) { S.extent("pf_p0", off(p.pf_p0), p.pf_b0); HOSTCHECK(!p.pf_p1 && !p.pf_kc && p.pf_wgs % 8 == 0, "helper jobs"); }
    // LDS: fold buffer + NORM 1 rows / NORM 3 staging (launch_gemm_ij), within the 160 KiB of a CU
    const int nku = p.K / (r.F8 ? 64 : 32), xr = (p.M * ((nku + r.WAVES - 1) / r.WAVES) * (r.F8 ? 2 : 1) * 4 + 63) / 64, sr = (p.M * (p.ssq_np / 4) + 63) / 64;
    const size_t sh = (size_t)r.WAVES * r.I * r.J * 1024 + (r.NORM == 1 ? (size_t)16 * (p.K + 8) * 2 : 0) + (r.NORM == 3 ? (size_t)r.WAVES * (xr + 1 + sr) * 1024 : 0);
    HOSTCHECK(sh <= 160 * 1024, "LDS %zu bytes", sh);
}

static int kv8_ties = 0, kv8_clamps = 0, x8_ties = 0, x8_clamps = 0;

static void run_gemm(GC c) {
    const unsigned seed = (unsigned)++g_cases;
    const int I = c.cfg / 100, J = (c.cfg / 10) % 10, WAVES = c.cfg == 112 ? 16 : (c.cfg % 10 ? 8 : 4), IW = I >= 2 ? 2 : 1;
    const int M = c.M, N = c.N, K = c.K, Mb = (M + 15) / 16, f8 = c.f8;
    const bool swi = c.epi == EPI_SWIGLU;
    float xs = swi ? (c.dense ? 0.0625f : 0.125f) : 1.f;      // activations (norm forms: norm weights) are integers times xs; SwiGLU halves it until the pre-activations fit
    char shape[200]; snprintf(shape, sizeof shape, "cfg %d %s f8 %d M %d N %d K %d", c.cfg, c.epi == EPI_LOGITS ? "LOGITS" : c.epi == EPI_RESID ? (c.ssq ? "RESID+ssq" : "RESID") : swi ? "SWIGLU" : (c.kv8 ? "QKV kv8" : "QKV"), f8, M, N, K);
    std::string extra;
    if (c.epi == EPI_QKV) extra += " pos " + std::to_string(c.pos);
    if (c.pf) extra += " pf_wgs " + std::to_string(c.pf);
    if (c.w_nt != 1) extra += " w_nt " + std::to_string(c.w_nt);
    // ---------------- operands
    std::vector<int> X((size_t)M * K); std::vector<signed char> W((size_t)N * K); std::vector<float> sc(N, 1.f);
    std::vector<long> acc, sab;
    int amp = 0; bool pre_ok = false; long worst = 0; double aworst = 0;
    std::vector<int> am(M), nwv(K); std::vector<signed char> sg;
    if (c.src == 1) { sg.resize((size_t)M * K); for (int m = 0; m < M; ++m) am[m] = (int)((m * 5u + seed) & 3u); for (int k = 0; k < K; ++k) nwv[k] = (int)(hsh((unsigned)k, 1u, seed) % 9u) - 4; }
    for (int n = 0; n < N; ++n) if (f8) sc[n] = c.tiny ? ldexpf(1.f, -129 - (int)(hsh((unsigned)n, 2u, seed) % 5u)) : ldexpf(1.f, (int)(hsh((unsigned)n, 2u, seed) % 3u) - 1);
    // activation (m, k) in units of xs: hashed integers in [-a, a]; at a = 8 (no SwiGLU, no sums of squares) a few e4m3 ties (17 -> 16, 19 -> 20) and values beyond 448
    auto xval = [&](int m, int k, int a) {
        const unsigned h = hsh((unsigned)m, (unsigned)k, seed * 8u + 1u);
        if (c.src == 1) return sg[(size_t)m * K + k] * nwv[k];
        if (!swi && !c.ssq && a == 8 && (h >> 8) % 53u == 0) { static const int sp[8] = {17, 19, -17, -19, 500, -500, 16, 20}; return sp[(h >> 16) & 7]; }
        return (int)(h % (unsigned)(2 * a + 1)) - a;
    };
    if (c.src == 1) for (int m = 0; m < M; ++m) for (int k = 0; k < K; ++k) sg[(size_t)m * K + k] = (hsh((unsigned)m, (unsigned)k, seed * 8u + 1u) & 1u) ? -1 : 1;
    for (int a : {8, 4, 2, 1}) {
        amp = a; if (swi && !c.dense && a > 1) continue;
        for (int m = 0; m < M; ++m) for (int k = 0; k < K; ++k) {
            int v = xval(m, k, a);
            if (f8 == 2 && !swi) { const float q = e4m3_round((float)v); if (q != (float)v) { if (std::abs(v) > 448) ++x8_clamps; else ++x8_ties; } v = (int)q; HOSTCHECK((float)v == q && (c.src == 0 || q == (float)xval(m, k, a)), "quantised activation"); }
            X[(size_t)m * K + k] = v;
        }
        for (int n = 0; n < N; ++n) for (int k = 0; k < K; ++k) W[(size_t)n * K + k] = (signed char)((int)(hsh((unsigned)n, (unsigned)k, seed * 8u + 2u) % (unsigned)(2 * a + 1)) - a);
        ref_gemm(X, W, M, N, K, acc, sab);
        pre_ok = true; worst = 0; aworst = 0;
        for (size_t i = 0; i < acc.size(); ++i) { if (sab[i] > worst) worst = sab[i]; const double v = std::fabs((double)acc[i] * sc[i % N]); if (v > aworst) aworst = v; }
        if (swi) { const double lim = c.dense ? 80.0 : 30.5; while (!c.dense && aworst * xs > lim && xs > 1.f / 256.f) xs *= 0.5f; aworst *= xs; if (aworst > lim) pre_ok = false; }
        if (worst >= (1L << 24)) pre_ok = false;
        if (c.ssq && (aworst + 8) * (aworst + 8) * 4 * 16 * IW >= 16777216.0) pre_ok = false;      // the sums of squares of the stored values (checked on the real values below)
        if (pre_ok) break;
    }
    if (swi && f8 == 2) for (int m = 0; m < M; ++m) for (int k = 0; k < K; ++k) HOSTCHECK(e4m3_round((float)X[(size_t)m * K + k] * xs) == (float)X[(size_t)m * K + k] * xs, "SwiGLU activations are e4m3 numbers");
    // ---------------- the arena
    Sess S; std::vector<std::pair<size_t, const char*>> names;
    auto A = [&](const char* nm, size_t bytes) { const size_t o = S.alloc(bytes); names.push_back({o, nm}); return o; };
    const size_t oW = A("W", (size_t)N * K * (f8 ? 1 : 2)), oS = f8 ? A("wscale", (size_t)N * 4) : 0;
    fill_w(S, oW, oS, W, sc, N, K, f8);
    GemmDP p; memset(&p, 0, sizeof p);
    p.W = S.dp<bf16_t>(oW); p.M = M; p.N = N; p.K = K; p.w_nt = c.w_nt; p.f8_mfma = f8 == 2; p.wscale = f8 ? S.dp<float>(oS) : nullptr;
    const size_t oPos = A("pos", 4); put_i32(S.img, oPos, 0, c.pos); p.pos = S.dp<int>(oPos);
    // X source
    size_t oX = 0, oHin = 0, oNw = 0, oEmb = 0, oIdx = 0, oCtl = 0, oHout = 0, oSsq = 0, oXr = 0, oWr = 0;
    int n_emb = 0, np = 0; const int tk = c.poslast ? NTOK - 1 : 0;
    Norm2P np2; memset(&np2, 0, sizeof np2); GemmDP pr; memset(&pr, 0, sizeof pr);
    std::vector<int> Xr; std::vector<signed char> Wr; std::vector<long> accr, sabr;
    if (c.src == 0) {
        oX = A("X", (size_t)Mb * 16 * K * 2);
        // (the packed X holds the UNQUANTISED values: W8A8 quantises in registers); rows >= M of the last block: NaN patterns
        for (int m = 0; m < Mb * 16; ++m) for (int k = 0; k < K; ++k) {
            if (m < M) put_bf(S.img, oX, xp_off(m, k, K), (float)xval(m, k, amp) * xs);
            else { const bf16_t nanv = (bf16_t)(((m + k) & 1 ? 0x7fc0 : 0xffc0) | ((m * 7 + k) & 0x3f)); memcpy(&S.img[oX + xp_off(m, k, K) * 2], &nanv, 2); }
        }
        p.X = S.dp<bf16_t>(oX);
    } else {
        oNw = A("nw", (size_t)K * 2); for (int k = 0; k < K; ++k) put_bf(S.img, oNw, k, (float)nwv[k] * xs);
        auto vrow = [&](int m, int k) { return (float)sg[(size_t)m * K + k] * ldexpf(1.f, am[m]); };
        if (c.norm <= 1) {       // rmsnorm2_kernel or the prologue norm: rows / gathered rows, control add
            auto cval = [&](int m, int t, int k) { return 2 * ((int)(hsh((unsigned)(m * NTOK + t), (unsigned)k, seed * 8u + 5u) % 9u) - 4); };
            if (c.gather) {
                n_emb = 2 * M + 4; oEmb = A("nemb", (size_t)n_emb * K * 2); oIdx = A("nidx", (size_t)M * 4);
                for (int r = 0; r < n_emb; ++r) for (int k = 0; k < K; ++k) put_bf(S.img, oEmb, (size_t)r * K + k, (float)((int)(hsh((unsigned)r, (unsigned)k, seed * 8u + 6u) % 7u) - 3));
                for (int m = 0; m < M; ++m) { const int r = 3 + (M - 1 - m) * 2; put_i32(S.img, oIdx, m, r); for (int k = 0; k < K; ++k) put_bf(S.img, oEmb, (size_t)r * K + k, vrow(m, k) - (c.add ? 0.5f * cval(m, tk, k) : 0.f)); }
            } else {
                oHin = A("nh_in", (size_t)M * K * 2);
                for (int m = 0; m < M; ++m) for (int k = 0; k < K; ++k) put_bf(S.img, oHin, (size_t)m * K + k, vrow(m, k) - (c.add ? 0.5f * cval(m, tk, k) : 0.f));
            }
            if (c.add) { oCtl = A("nctrl", (size_t)M * NTOK * K * 2); for (int m = 0; m < M; ++m) for (int t = 0; t < NTOK; ++t) for (int k = 0; k < K; ++k) put_bf(S.img, oCtl, ((size_t)m * NTOK + t) * K + k, (float)cval(m, t, k)); }
            if (c.nhout) oHout = A("nh_out", (size_t)Mb * 16 * K * 2);
            if (c.norm == 1) {
                p.nh_in = c.gather ? nullptr : S.dp<bf16_t>(oHin); p.nemb = c.gather ? S.dp<bf16_t>(oEmb) : nullptr; p.nidx = c.gather ? S.dp<int>(oIdx) : nullptr;
                p.nh_out = c.nhout ? S.dp<bf16_t>(oHout) : nullptr; p.nw = S.dp<bf16_t>(oNw); p.nctrl = c.add ? S.dp<bf16_t>(oCtl) : nullptr;
                p.nadd = c.add; p.nT = c.pos + 1 - tk; p.n_tok = NTOK; p.ncs = 0.5f; p.neps = c.eps;
            } else {
                oX = A("xn", (size_t)Mb * 16 * K * 2); p.X = S.dp<bf16_t>(oX);
                np2.h_in = c.gather ? nullptr : S.dp<bf16_t>(oHin); np2.emb = c.gather ? S.dp<bf16_t>(oEmb) : nullptr; np2.idx = c.gather ? S.dp<int>(oIdx) : nullptr;
                np2.h_out = c.nhout ? S.dp<bf16_t>(oHout) : nullptr; np2.xn = S.dp<bf16_t>(oX); np2.w = S.dp<bf16_t>(oNw); np2.ctrl = c.add ? S.dp<bf16_t>(oCtl) : nullptr;
                np2.pos = S.dp<int>(oPos); np2.add = c.add ? 1 : 0; np2.T = c.pos + 1 - tk; np2.n_tok = NTOK; np2.cs = 0.5f; np2.D = K; np2.eps = c.eps;
            }
        } else {                 // NORM 2 / 3: h and its partials come from an EPI_RESID launch (N = K of this linear, K = 32)
            const int rIW = c.rI >= 2 ? 2 : 1; np = K / (16 * rIW);
            extra += " ssq_np " + std::to_string(np);
            oHin = A("h (producer)", (size_t)Mb * 16 * K * 2); oSsq = A("ssq", (size_t)Mb * 16 * np * 4); oXr = A("X (producer)", (size_t)Mb * 16 * 32 * 2); oWr = A("W (producer)", (size_t)K * 32 * 2);
            Xr.resize((size_t)M * 32); Wr.resize((size_t)K * 32);
            for (int m = 0; m < M; ++m) for (int k = 0; k < 32; ++k) Xr[(size_t)m * 32 + k] = (int)(hsh((unsigned)m, (unsigned)k, seed * 8u + 3u) % 3u) - 1;
            for (int n = 0; n < K; ++n) for (int k = 0; k < 32; ++k) Wr[(size_t)n * 32 + k] = (signed char)((int)(hsh((unsigned)n, (unsigned)k, seed * 8u + 4u) % 5u) - 2);
            ref_gemm(Xr, Wr, M, K, 32, accr, sabr);
            for (int m = 0; m < Mb * 16; ++m) for (int k = 0; k < 32; ++k) { if (m < M) put_bf(S.img, oXr, xp_off(m, k, 32), (float)Xr[(size_t)m * 32 + k]); else { const bf16_t nanv = 0x7fc1; memcpy(&S.img[oXr + xp_off(m, k, 32) * 2], &nanv, 2); } }
            for (int n = 0; n < K; ++n) for (int k = 0; k < 32; ++k) put_bf(S.img, oWr, xp_off(n, k, 32), (float)Wr[(size_t)n * 32 + k]);
            for (int m = 0; m < M; ++m) for (int k = 0; k < K; ++k) put_bf(S.img, oHin, (size_t)m * K + k, vrow(m, k) - (float)accr[(size_t)m * K + k]);      // h + acc = +-2^a
            pr.W = S.dp<bf16_t>(oWr); pr.X = S.dp<bf16_t>(oXr); pr.M = M; pr.N = K; pr.K = 32; pr.w_nt = 1; pr.h = S.dp<bf16_t>(oHin); pr.ssq_out = S.dp<float>(oSsq); pr.ssq_ld = np;
            p.nh_in = S.dp<bf16_t>(oHin); p.nw = S.dp<bf16_t>(oNw); p.ssq_in = S.dp<float>(oSsq); p.ssq_np = np; p.neps = c.eps;
        }
    }
    // outputs
    size_t oOut = 0, oH = 0, oSo = 0, oQ = 0, oKc = 0, oVc = 0, oRope = 0, oPf = 0;
    const int kvb = c.kv8 ? 1 : 2;
    if (c.epi == EPI_LOGITS) { oOut = A("outf", (size_t)Mb * 16 * N * 4); p.outf = S.dp<float>(oOut); }
    if (c.epi == EPI_RESID) {
        oH = A("h", (size_t)Mb * 16 * N * 2); p.h = S.dp<bf16_t>(oH);
        for (int m = 0; m < M; ++m) for (int n = 0; n < N; ++n) put_bf(S.img, oH, (size_t)m * N + n, (float)((int)(hsh((unsigned)m, (unsigned)n, seed * 8u + 7u) % 17u) - 8));
        if (c.ssq) { p.ssq_ld = N / (16 * IW); oSo = A("ssq_out", (size_t)Mb * 16 * p.ssq_ld * 4); p.ssq_out = S.dp<float>(oSo); }
    }
    if (swi) { oOut = A("outp", (size_t)Mb * 16 * (N / 2) * 2); p.outp = S.dp<bf16_t>(oOut); }
    if (c.epi == EPI_QKV) {
        oQ = A("qout", (size_t)Mb * 16 * HH * 64 * 2); oKc = A("kc", (size_t)M * HH * SA * 64 * kvb); oVc = A("vc", (size_t)M * HH * SA * 64 * kvb); oRope = A("rope", (size_t)SA * 64 * 4);
        for (int t = 0; t < SA; ++t) for (int pr_ = 0; pr_ < 32; ++pr_) { float cc, ss; rope_pair(t, pr_, cc, ss); put_f32(S.img, oRope, ((size_t)t * 32 + pr_) * 2, cc); put_f32(S.img, oRope, ((size_t)t * 32 + pr_) * 2 + 1, ss); }
        p.qout = S.dp<bf16_t>(oQ); p.kc = S.dp<bf16_t>(oKc); p.vc = S.dp<bf16_t>(oVc); p.rope = S.dp<float>(oRope); p.H = HH; p.SA = SA; p.dim = DIM; p.kv8 = c.kv8;
    }
    if (c.pf) { oPf = A("helper scratch", 64 * 1024); memset(&S.img[oPf], 0x5a, 64 * 1024); p.pf_p0 = S.dp<char>(oPf); p.pf_b0 = 64 * 1024; p.pf_wgs = c.pf; }
    // ---------------- expected image
    std::vector<unsigned char> E = S.img, E0;       // E0: after the producer launch (rmsnorm2 / EPI_RESID)
    Approx ap; bool use_ap = false;
    if (c.src == 1) {
        if (c.norm <= 1 && c.nhout) for (int m = 0; m < M; ++m) for (int k = 0; k < K; ++k) put_bf(E, oHout, (size_t)m * K + k, (float)sg[(size_t)m * K + k] * ldexpf(1.f, am[m]));
        if (c.norm == 0) for (int m = 0; m < M; ++m) for (int k = 0; k < K; ++k) put_bf(E, oX, xp_off(m, k, K), (float)sg[(size_t)m * K + k] * ((float)nwv[k] * xs));      // (-1 x 0 = -0: the sign of a zero is part of the bits)
        if (c.norm >= 2) {
            const int rIW = c.rI >= 2 ? 2 : 1;
            for (int m = 0; m < M; ++m) { for (int k = 0; k < K; ++k) put_bf(E, oHin, (size_t)m * K + k, (float)sg[(size_t)m * K + k] * ldexpf(1.f, am[m])); for (int j = 0; j < np; ++j) put_f32(E, oSsq, (size_t)m * np + j, (float)(16 * rIW) * ldexpf(1.f, 2 * am[m])); }
        }
        E0 = E;
    }
    long tie8 = 0, clamp8 = 0, n_scale_order = 0;
    for (int m = 0; m < M; ++m) {
        std::vector<float> v(N);
        for (int n = 0; n < N; ++n) v[n] = (float)acc[(size_t)m * N + n] * xs * sc[n];
        if (c.epi == EPI_LOGITS) for (int n = 0; n < N; ++n) put_f32(E, oOut, (size_t)m * N + n, rbf(v[n]));
        else if (c.epi == EPI_RESID) {
            std::vector<double> sq(N / (16 * IW), 0.0);
            for (int n = 0; n < N; ++n) { bf16_t hb; memcpy(&hb, &S.img[oH + ((size_t)m * N + n) * 2], 2); const float o = rbf(bf2f(hb) + rbf(v[n])); put_bf(E, oH, (size_t)m * N + n, o); sq[n / (16 * IW)] += (double)o * o; if (c.ssq && 2 * o != std::floor(2 * o)) pre_ok = false; }      // stored values in units of 1/2 (wscale 1/2): squares in units of 1/4
            if (c.ssq) for (size_t j = 0; j < sq.size(); ++j) { if (4 * sq[j] >= 16777216.0) pre_ok = false; put_f32(E, oSo, (size_t)m * p.ssq_ld + j, (float)sq[j]); }
        } else if (swi) {
            if (m == 0) { const size_t ne = (size_t)Mb * 16 * (N / 2); ap.off = oOut; ap.ref.assign(ne, 0.f); ap.tol.assign(ne, 0.f); ap.host32.assign(ne, 0.f); ap.isout.assign(ne, 0); use_ap = true; }
            for (int j = 0; j < N / 2; ++j) {
                const int na = (j >> 4) * 32 + (j & 15), nc = na + 16;
                const float av = rbf(v[na]), cv = rbf(v[nc]);
                const float g = rbf((float)((double)av / (1.0 + std::exp(-(double)av)))), o = rbf(g * cv);
                const size_t ei = xp_off(m, j, N / 2);
                ap.ref[ei] = o; ap.tol[ei] = (float)(ulp_bf16(g) * std::fabs(cv) + ulp_bf16(o)); ap.isout[ei] = 1; ap.host32[ei] = rbf(rbf(av / (1.0f + expf(-av))) * cv);
                put_bf(E, oOut, ei, o);
            }
        } else {
            for (int n = 0; n < N; n += 2) {
                const int sec = n / DIM, within = n % DIM, hh = within >> 6, d = within & 63;
                const float x0 = rbf(v[n]), x1 = rbf(v[n + 1]);
                const size_t sb = ((size_t)m * HH + hh) * SA * 64;
                auto e8 = [&](float f) { const float q = e4m3_round(f); if (q != f) { if (std::fabs(f) > 448.f) ++clamp8; else ++tie8; } return e4m3_encode(f); };
                if (sec == 2) {
                    if (c.kv8) { E[oVc + sb + v8_off(c.pos, d)] = e8(x0); E[oVc + sb + v8_off(c.pos, d + 1)] = e8(x1); }
                    else { put_bf(E, oVc, sb + v_off(c.pos, d), x0); put_bf(E, oVc, sb + v_off(c.pos, d + 1), x1); }
                } else {
                    float cc, ss; rope_pair(c.pos, d >> 1, cc, ss);
                    const float r0u = x0 * cc - x1 * ss, r1u = x1 * cc + x0 * ss, r0 = rbf(r0u), r1 = rbf(r1u);
                    if (sec == 0 && (rbf(r0u * 0.125f) != rbf(r0 * 0.125f) || rbf(r1u * 0.125f) != rbf(r1 * 0.125f))) ++n_scale_order;
                    if (sec == 0) { put_bf(E, oQ, ((size_t)m * HH + hh) * 64 + d, rbf(r0 * 0.125f)); put_bf(E, oQ, ((size_t)m * HH + hh) * 64 + d + 1, rbf(r1 * 0.125f)); }
                    else if (c.kv8) { E[oKc + sb + k8_off(c.pos, d)] = e8(r0); E[oKc + sb + k8_off(c.pos, d + 1)] = e8(r1); }
                    else { put_bf(E, oKc, sb + k_off(c.pos, d), r0); put_bf(E, oKc, sb + k_off(c.pos, d + 1), r1); }
                }
            }
        }
    }
    kv8_ties += (int)tie8; kv8_clamps += (int)clamp8;
    if (c.tiny) { HOSTCHECK(f8 == 1 && c.epi == EPI_QKV && n_scale_order > 0, "the subnormal-q case holds no element on which the order of scale and rounding matters"); extra += " [" + std::to_string(n_scale_order) + " q elements where rnd(r) / 8 != rnd(r / 8)]"; }
    // ---------------- preconditions, route
    char rs[64], es[64];
    DecGemmRoute want = {I, J, WAVES, f8, c.norm}, r = {0, 0, 0, 0, 0};
    const int rc = car_dec_gemm_route(&p, c.epi, c.cfg, c.staged_ok, &r);
    route_str(rs, sizeof rs, rc, r); route_str(es, sizeof es, 0, want);
    const std::string head = c.name + " | " + shape + extra;
    if (!pre_ok) { printf("%-100s %-22s PRECONDITION FAIL (harness): worst sum %ld, worst |pre-activation| %.3f\n", head.c_str(), rs, worst, aworst); ++g_fail; return; }
    if (use_ap) {
        size_t nout = 0, hd = 0, hb = 0;
        for (size_t i = 0; i < ap.isout.size(); ++i) if (ap.isout[i]) { ++nout; if (memcmp(&ap.host32[i], &ap.ref[i], 4) != 0) { ++hd; if (!(std::fabs((double)ap.host32[i] - ap.ref[i]) <= ap.tol[i])) ++hb; } }
        if (hb || hd * 100 > nout) { printf("%-100s %-22s PRECONDITION FAIL (harness): host fp32 libm vs fp64: %zu of %zu differ, %zu beyond the bound\n", head.c_str(), rs, hd, nout, hb); ++g_fail; return; }
        if (!g_dev) extra += " [host libm differs on " + std::to_string(hd) + " of " + std::to_string(nout) + ", none beyond the bound]";
    }
    if (rc != 0 || memcmp(&r, &want, sizeof r) != 0) { printf("%-100s %-22s FAIL (route; expected %s; not launched)\n", head.c_str(), rs, es); ++g_fail; return; }
    gemm_extents(S, p, c.epi, r, c.pos, n_emb);
    DecGemmRoute rr = {0, 0, 0, 0, 0};
    if (c.src == 1 && c.norm >= 2) {
        const int pc = c.rI >= 2 ? 211 : 111;
        HOSTCHECK(car_dec_gemm_route(&pr, EPI_RESID, pc, 1, &rr) == 0 && rr.NORM == 0 && rr.I == c.rI, "producer route");
        gemm_extents(S, pr, EPI_RESID, rr, 0, 0);
        for (size_t i = 0; i < sabr.size(); ++i) HOSTCHECK(sabr[i] <= 128, "producer sum");
    }
    if (c.src == 1 && c.norm == 0) { S.extent("xn", oX, (size_t)Mb * 16 * K * 2); HOSTCHECK(K % 32 == 0 && K <= 4096, "rmsnorm2 D"); }
    if (!g_dev) { printf("%-100s %-22s worst sum %ld%s  ok\n", (c.name + " | " + shape + extra).c_str(), rs, worst, use_ap ? (", |a| <= " + std::to_string(aworst)).c_str() : ""); return; }
    // ---------------- device
    S.upload();
    std::vector<unsigned char> got; std::string verdict;
    if (c.src == 1 && c.norm != 1) {
        if (c.norm == 0) car_launch_rmsnorm2(&np2, M, 0); else if (launch(pr, EPI_RESID, c.rI >= 2 ? 211 : 111, 1)) verdict = "FAIL (producer refused)";
        S.download(got);
        if (verdict.empty()) { const std::string v0 = compare(got, E0, S, nullptr, names); if (v0 != "OK") verdict = std::string(c.norm == 0 ? "rmsnorm2: " : "EPI_RESID producer: ") + v0; }
    }
    if (verdict.empty()) {
        const int lrc = launch(p, c.epi, c.cfg, c.staged_ok);
        S.download(got);
        verdict = lrc ? "FAIL (return code " + std::to_string(lrc) + ")" : compare(got, E, S, use_ap ? &ap : nullptr, names);
    }
    printf("%-100s %-22s worst sum %ld  %s\n", head.c_str(), rs, worst, verdict.c_str()); fflush(stdout);
    if (verdict.compare(0, 2, "OK") != 0) ++g_fail;
}

// ---------------------------------------------------------------------------------------------------------------- refusals
static void run_refusal(const char* name, int epi, int cfg, int M, int N, int K, int f8, int normkind /* 0 none, 1 fused, 2 ssq_in */, int ssq_np) {
    ++g_cases;
    Sess S; const int Mb = (M + 15) / 16;
    const size_t oW = S.alloc((size_t)N * (K + 64) * 2), oX = S.alloc((size_t)Mb * 16 * (K + 64) * 2), oS = S.alloc((size_t)N * 4), oO = S.alloc((size_t)Mb * 16 * N * 4), oNw = S.alloc((size_t)(K + 64) * 2), oSs = S.alloc((size_t)Mb * 16 * 132 * 4), oPos = S.alloc(4);
    memset(&S.img[oW], 0, (size_t)N * K * 2); memset(&S.img[oX], 0, (size_t)Mb * 16 * K * 2); memset(&S.img[oNw], 0, (size_t)K * 2); memset(&S.img[oSs], 0, (size_t)Mb * 16 * 132 * 4); put_i32(S.img, oPos, 0, 0);
    for (int n = 0; n < N; ++n) put_f32(S.img, oS, n, 1.f);
    GemmDP p; memset(&p, 0, sizeof p);
    p.W = S.dp<bf16_t>(oW); p.X = S.dp<bf16_t>(oX); p.M = M; p.N = N; p.K = K; p.w_nt = 1; p.wscale = f8 ? S.dp<float>(oS) : nullptr; p.f8_mfma = f8 == 2;
    p.h = S.dp<bf16_t>(oO); p.outp = S.dp<bf16_t>(oO); p.outf = S.dp<float>(oO); p.pos = S.dp<int>(oPos);
    if (normkind) { p.nw = S.dp<bf16_t>(oNw); p.nh_in = S.dp<bf16_t>(oX); p.neps = 1e-5f; }
    if (normkind == 2) { p.ssq_in = S.dp<float>(oSs); p.ssq_np = ssq_np; }
    DecGemmRoute r; const int rc = car_dec_gemm_route(&p, epi, cfg, 1, &r);
    std::string verdict = "OK";
    if (rc == 0) verdict = "FAIL (the route function accepts the call; not launched)";
    else if (g_dev) {
        S.upload();
        const int lrc = launch(p, epi, cfg, 1);
        std::vector<unsigned char> got; S.download(got);
        if (lrc == 0) verdict = "FAIL (the launcher returned 0)"; else if (got != S.img) verdict = "FAIL (a refused call wrote to memory)";
    }
    printf("%-100s %-22s %s\n", (std::string("refusal: ") + name).c_str(), rc ? "refused" : "accepted", verdict.c_str());
    if (verdict != "OK") ++g_fail;
}

// ---------------------------------------------------------------------------------------------------------------- prefill_rope_kv2_kernel (+ a decode-time row behind it)
static void run_prefill(int Tn, int t0, int kv8) {
    const unsigned seed = (unsigned)++g_cases;
    const int b = 2, kvb = kv8 ? 1 : 2, K = 3 * DIM;
    Sess S; std::vector<std::pair<size_t, const char*>> names;
    auto A = [&](const char* nm, size_t bytes) { const size_t o = S.alloc(bytes); names.push_back({o, nm}); return o; };
    const size_t oQkv = A("qkv", (size_t)b * Tn * K * 2), oKc = A("kc", (size_t)b * HH * SA * 64 * kvb), oVc = A("vc", (size_t)b * HH * SA * 64 * kvb), oRope = A("rope", (size_t)SA * 64 * 4);
    const size_t oW = A("W (identity)", (size_t)K * K * 2), oX = A("X", (size_t)16 * K * 2), oQ = A("qout", (size_t)16 * HH * 64 * 2), oPos = A("pos", 4);
    HOSTCHECK(t0 + Tn < SA, "prefill window and the decode row inside the stream");
    // values: integers, some beyond 448 and e4m3 ties
    auto qv = [&](int bb, int t, int n) { const unsigned h = hsh((unsigned)(bb * 64 + t), (unsigned)n, seed); if (h % 29u == 0) { static const int sp[6] = {17, 19, -19, 500, -500, 34}; return sp[(h >> 8) % 6u]; } return (int)((h >> 4) % 33u) - 16; };
    for (int t = 0; t < SA; ++t) for (int pr = 0; pr < 32; ++pr) { float cc, ss; rope_pair(t, pr, cc, ss); put_f32(S.img, oRope, ((size_t)t * 32 + pr) * 2, cc); put_f32(S.img, oRope, ((size_t)t * 32 + pr) * 2 + 1, ss); }
    for (int bb = 0; bb < b; ++bb) for (int t = 0; t < Tn; ++t) for (int n = 0; n < K; ++n) put_bf(S.img, oQkv, ((size_t)bb * Tn + t) * K + n, (float)qv(bb, t, n));
    for (int n = 0; n < K; ++n) for (int k = 0; k < K; ++k) put_bf(S.img, oW, xp_off(n, k, K), n == k ? 1.f : 0.f);
    for (int m = 0; m < 16; ++m) for (int k = 0; k < K; ++k) { if (m < b) put_bf(S.img, oX, xp_off(m, k, K), (float)qv(m, Tn, k)); else { const bf16_t nanv = 0x7fc3; memcpy(&S.img[oX + xp_off(m, k, K) * 2], &nanv, 2); } }
    put_i32(S.img, oPos, 0, t0 + Tn);
    std::vector<unsigned char> E = S.img, E1;
    auto row = [&](std::vector<unsigned char>& Eo, int bb, int tw, bool decode) {
        const int t = t0 + tw;
        for (int h = 0; h < HH; ++h) for (int d = 0; d < 64; d += 2) {
            float cc, ss; rope_pair(t, d >> 1, cc, ss);
            const float q0 = (float)qv(bb, tw, h * 64 + d), q1 = (float)qv(bb, tw, h * 64 + d + 1), k0 = (float)qv(bb, tw, DIM + h * 64 + d), k1 = (float)qv(bb, tw, DIM + h * 64 + d + 1);
            const float v0 = (float)qv(bb, tw, 2 * DIM + h * 64 + d), v1 = (float)qv(bb, tw, 2 * DIM + h * 64 + d + 1);
            const float rq0 = rbf(q0 * cc - q1 * ss), rq1 = rbf(q1 * cc + q0 * ss), rk0 = rbf(k0 * cc - k1 * ss), rk1 = rbf(k1 * cc + k0 * ss);
            if (decode) { put_bf(Eo, oQ, ((size_t)bb * HH + h) * 64 + d, rbf(rq0 * 0.125f)); put_bf(Eo, oQ, ((size_t)bb * HH + h) * 64 + d + 1, rbf(rq1 * 0.125f)); }
            else { const size_t ro = ((size_t)bb * Tn + tw) * K; put_bf(Eo, oQkv, ro + h * 64 + d, rq0); put_bf(Eo, oQkv, ro + h * 64 + d + 1, rq1); put_bf(Eo, oQkv, ro + DIM + h * 64 + d, rk0); put_bf(Eo, oQkv, ro + DIM + h * 64 + d + 1, rk1); }
            const size_t sb = ((size_t)bb * HH + h) * SA * 64;
            if (kv8) { Eo[oKc + sb + k8_off(t, d)] = e4m3_encode(rk0); Eo[oKc + sb + k8_off(t, d + 1)] = e4m3_encode(rk1); Eo[oVc + sb + v8_off(t, d)] = e4m3_encode(v0); Eo[oVc + sb + v8_off(t, d + 1)] = e4m3_encode(v1); }
            else { put_bf(Eo, oKc, sb + k_off(t, d), rk0); put_bf(Eo, oKc, sb + k_off(t, d + 1), rk1); put_bf(Eo, oVc, sb + v_off(t, d), v0); put_bf(Eo, oVc, sb + v_off(t, d + 1), v1); }
        }
    };
    for (int bb = 0; bb < b; ++bb) for (int t = 0; t < Tn; ++t) row(E, bb, t, false);
    E1 = E; for (int bb = 0; bb < b; ++bb) row(E1, bb, Tn, true);
    GemmDP p; memset(&p, 0, sizeof p);
    p.W = S.dp<bf16_t>(oW); p.X = S.dp<bf16_t>(oX); p.M = b; p.N = K; p.K = K; p.w_nt = 1; p.qout = S.dp<bf16_t>(oQ); p.kc = S.dp<bf16_t>(oKc); p.vc = S.dp<bf16_t>(oVc); p.rope = S.dp<float>(oRope);
    p.pos = S.dp<int>(oPos); p.H = HH; p.SA = SA; p.dim = DIM; p.kv8 = kv8;
    DecGemmRoute r; HOSTCHECK(car_dec_gemm_route(&p, EPI_QKV, 211, 1, &r) == 0 && r.NORM == 0 && r.I == 2 && r.WAVES == 8, "decode row route");
    gemm_extents(S, p, EPI_QKV, r, t0 + Tn, 0);
    S.extent("qkv", oQkv, (size_t)b * Tn * K * 2); S.extent("rope", oRope, (size_t)(t0 + Tn) * 64 * 4); S.extent("kc", oKc, (size_t)b * HH * SA * 64 * kvb);
    char head[160]; snprintf(head, sizeof head, "prefill_rope_kv2 + decode row | b 2 H 2 Tn %d t0 %d %s", Tn, t0, kv8 ? "kv8" : "bf16");
    if (!g_dev) { printf("%-100s %-22s ok\n", head, ""); return; }
    S.upload();
    car_launch_prefill_rope_kv2(S.dp<void>(oQkv), S.dp<void>(oKc), S.dp<void>(oVc), S.dp<float>(oRope), b, Tn, HH, DIM, SA, kv8, t0, 0); ++g_launches;
    std::vector<unsigned char> got; S.download(got);
    std::string verdict = compare(got, E, S, nullptr, names);
    if (verdict == "OK") {
        if (launch(p, EPI_QKV, 211, 1)) verdict = "FAIL (decode row refused)";
        else { S.download(got); verdict = compare(got, E1, S, nullptr, names); if (verdict != "OK") verdict = "decode row at pos t0 + Tn: " + verdict; }
    } else verdict = "prefill: " + verdict;
    printf("%-100s %-22s %s\n", head, "", verdict.c_str()); fflush(stdout);
    if (verdict != "OK") ++g_fail;
}

// ---------------------------------------------------------------------------------------------------------------- general integer rows through the norm forms
// Rows of integers in [-8, 8]: rstd is not a power of two, so (a) rmsnorm2's packed row must equal, in every element, the row computed with ONE of the candidate
// rstd values — the correctly rounded 1/sqrt(mean + eps) and its two neighbours (rsqrtf: 1 ulp, HIP math API documentation) — and (b) every fused form must be
// bit-equal to rmsnorm2 followed by the NORM 0 launch of the same tile shape: the integer residuals make the sums of squares exact, so the three kernels evaluate
// the same expression on the same number, and the same tile shape splits and folds K in the same order.
static void run_general(int cfg, int f8, int M, int K, int rI) {
    const unsigned seed = (unsigned)++g_cases;
    const int I = cfg / 100, J = (cfg / 10) % 10, Mb = (M + 15) / 16, N = 16 * I * 3, rIW = rI >= 2 ? 2 : 1, np = K / (16 * rIW);
    const bool do1 = M <= 16 && J == 1 && K <= 2048;
    const float eps = 1e-5f;
    Sess S; std::vector<std::pair<size_t, const char*>> names;
    auto A = [&](const char* nm, size_t bytes) { const size_t o = S.alloc(bytes); names.push_back({o, nm}); return o; };
    const size_t oW = A("W", (size_t)N * K * (f8 ? 1 : 2)), oS = f8 ? A("wscale", (size_t)N * 4) : 0, oNw = A("nw", (size_t)K * 2), oH0 = A("h rows", (size_t)M * K * 2), oXn = A("xn", (size_t)Mb * 16 * K * 2);
    const size_t oA = A("outf (rmsnorm2 + NORM 0)", (size_t)Mb * 16 * N * 4), oB = A("outf (NORM 1)", (size_t)Mb * 16 * N * 4), oC = A("outf (NORM 2 / 3)", (size_t)Mb * 16 * N * 4);
    const size_t oHp = A("h (producer)", (size_t)Mb * 16 * K * 2), oSsq = A("ssq", (size_t)Mb * 16 * np * 4), oXr = A("X (producer)", (size_t)Mb * 16 * 32 * 2), oWr = A("W (producer)", (size_t)K * 32 * 2), oPos = A("pos", 4);
    put_i32(S.img, oPos, 0, 0);
    std::vector<signed char> W((size_t)N * K), Wr((size_t)K * 32); std::vector<float> sc(N, 1.f); std::vector<int> Xr((size_t)M * 32), hv((size_t)M * K), nwv(K);
    for (int n = 0; n < N; ++n) { if (f8) sc[n] = ldexpf(1.f, (int)(hsh((unsigned)n, 2u, seed) % 3u) - 1); for (int k = 0; k < K; ++k) W[(size_t)n * K + k] = (signed char)((int)(hsh((unsigned)n, (unsigned)k, seed * 8u + 2u) % 9u) - 4); }
    fill_w(S, oW, oS, W, sc, N, K, f8);
    for (int k = 0; k < K; ++k) { nwv[k] = (int)(hsh((unsigned)k, 1u, seed) % 9u) - 4; put_bf(S.img, oNw, k, (float)nwv[k]); }
    for (int m = 0; m < M; ++m) for (int k = 0; k < 32; ++k) Xr[(size_t)m * 32 + k] = (int)(hsh((unsigned)m, (unsigned)k, seed * 8u + 3u) % 3u) - 1;
    for (int n = 0; n < K; ++n) for (int k = 0; k < 32; ++k) Wr[(size_t)n * 32 + k] = (signed char)((int)(hsh((unsigned)n, (unsigned)k, seed * 8u + 4u) % 5u) - 2);
    std::vector<long> accr, sabr; ref_gemm(Xr, Wr, M, K, 32, accr, sabr);
    for (int m = 0; m < Mb * 16; ++m) for (int k = 0; k < 32; ++k) { if (m < M) put_bf(S.img, oXr, xp_off(m, k, 32), (float)Xr[(size_t)m * 32 + k]); else { const bf16_t nanv = 0x7fc1; memcpy(&S.img[oXr + xp_off(m, k, 32) * 2], &nanv, 2); } }
    for (int n = 0; n < K; ++n) for (int k = 0; k < 32; ++k) put_bf(S.img, oWr, xp_off(n, k, 32), (float)Wr[(size_t)n * 32 + k]);
    std::vector<unsigned char> E = S.img;
    std::vector<std::vector<float>> cand(M);
    for (int m = 0; m < M; ++m) {
        long ss = 0;
        for (int k = 0; k < K; ++k) { const int v = (int)(hsh((unsigned)m, (unsigned)k, seed * 8u + 1u) % 17u) - 8; hv[(size_t)m * K + k] = v; ss += (long)v * v; put_bf(S.img, oH0, (size_t)m * K + k, (float)v); put_bf(E, oH0, (size_t)m * K + k, (float)v);
            HOSTCHECK(std::labs(accr[(size_t)m * K + k]) <= 64, "producer sum"); put_bf(S.img, oHp, (size_t)m * K + k, (float)(v - accr[(size_t)m * K + k])); put_bf(E, oHp, (size_t)m * K + k, (float)v); }
        HOSTCHECK(ss < (1L << 24), "sum of squares");
        for (int j = 0; j < np; ++j) { long q = 0; for (int k = j * 16 * rIW; k < (j + 1) * 16 * rIW; ++k) q += (long)hv[(size_t)m * K + k] * hv[(size_t)m * K + k]; put_f32(E, oSsq, (size_t)m * np + j, (float)q); }
        const float t = (float)ss / (float)K + eps, c0 = (float)(1.0 / std::sqrt((double)t));
        cand[m] = {c0, nextafterf(c0, 0.f), nextafterf(c0, 2.f)};
    }
    GemmDP p0; memset(&p0, 0, sizeof p0);
    p0.W = S.dp<bf16_t>(oW); p0.M = M; p0.N = N; p0.K = K; p0.w_nt = 1; p0.f8_mfma = f8 == 2; p0.wscale = f8 ? S.dp<float>(oS) : nullptr; p0.pos = S.dp<int>(oPos);
    GemmDP pa = p0, pb = p0, pc = p0, pr; memset(&pr, 0, sizeof pr);
    pa.X = S.dp<bf16_t>(oXn); pa.outf = S.dp<float>(oA);
    pb.nh_in = S.dp<bf16_t>(oH0); pb.nw = S.dp<bf16_t>(oNw); pb.neps = eps; pb.outf = S.dp<float>(oB);
    pc.nh_in = S.dp<bf16_t>(oHp); pc.nw = S.dp<bf16_t>(oNw); pc.neps = eps; pc.ssq_in = S.dp<float>(oSsq); pc.ssq_np = np; pc.outf = S.dp<float>(oC);
    pr.W = S.dp<bf16_t>(oWr); pr.X = S.dp<bf16_t>(oXr); pr.M = M; pr.N = K; pr.K = 32; pr.w_nt = 1; pr.h = S.dp<bf16_t>(oHp); pr.ssq_out = S.dp<float>(oSsq); pr.ssq_ld = np;
    Norm2P nq; memset(&nq, 0, sizeof nq); nq.h_in = S.dp<bf16_t>(oH0); nq.xn = S.dp<bf16_t>(oXn); nq.w = S.dp<bf16_t>(oNw); nq.pos = S.dp<int>(oPos); nq.D = K; nq.eps = eps;
    DecGemmRoute ra, rb, rc, rr; std::string verdict = "OK";
    const int nku = K / (f8 ? 64 : 32); const int want3 = (M <= 16 && J == 1 && cfg % 10 == 1 && nku >= 8 && ((nku + 7) / 8) * (f8 ? 2 : 1) <= 16) ? 3 : 2;
    if (car_dec_gemm_route(&pa, EPI_LOGITS, cfg, 1, &ra) || ra.NORM != 0 || car_dec_gemm_route(&pc, EPI_LOGITS, cfg, 1, &rc) || rc.NORM != want3 || (do1 && (car_dec_gemm_route(&pb, EPI_LOGITS, cfg, 1, &rb) || rb.NORM != 1))
        || car_dec_gemm_route(&pr, EPI_RESID, rI >= 2 ? 211 : 111, 1, &rr) || rr.NORM != 0) verdict = "FAIL (route; not launched)";
    char head[200]; snprintf(head, sizeof head, "integer rows: rmsnorm2 + NORM 0 == NORM 1 == NORM %d | cfg %d LOGITS f8 %d M %d N %d K %d ssq_np %d%s", want3, cfg, f8, M, N, K, np, do1 ? "" : " (no NORM 1: M > 16, J > 1 or K > 2048)");
    if (verdict == "OK") {
        gemm_extents(S, pa, EPI_LOGITS, ra, 0, 0); gemm_extents(S, pc, EPI_LOGITS, rc, 0, 0); if (do1) gemm_extents(S, pb, EPI_LOGITS, rb, 0, 0); gemm_extents(S, pr, EPI_RESID, rr, 0, 0);
        S.extent("xn", oXn, (size_t)Mb * 16 * K * 2); S.extent("h rows", oH0, (size_t)M * K * 2);
    }
    if (verdict == "OK" && g_dev) {
        S.upload();
        car_launch_rmsnorm2(&nq, M, 0); ++g_launches;
        int lrc = launch(pa, EPI_LOGITS, cfg, 1); if (do1) lrc |= launch(pb, EPI_LOGITS, cfg, 1); lrc |= launch(pr, EPI_RESID, rI >= 2 ? 211 : 111, 1); lrc |= launch(pc, EPI_LOGITS, cfg, 1);
        std::vector<unsigned char> got; S.download(got);
        if (lrc) verdict = "FAIL (a launch was refused)";
        // (a) every row of xn against the candidate rstd values
        for (int m = 0; m < M && verdict == "OK"; ++m) {
            bool any = false;
            for (float rs : cand[m]) { bool all = true; for (int k = 0; k < K && all; ++k) { const bf16_t e = f2bf(rbf((float)hv[(size_t)m * K + k] * rs) * (float)nwv[k]); if (memcmp(&e, &got[oXn + xp_off(m, k, K) * 2], 2) != 0) all = false; } any |= all; }
            if (!any) verdict = "FAIL (rmsnorm2 row " + std::to_string(m) + " equals the row of none of the three candidate rstd values)";
        }
        // (b) the packed rows and the NORM 0 output are taken from the device; everything else has one possible value
        for (int m = 0; m < M; ++m) for (int k = 0; k < K; ++k) memcpy(&E[oXn + xp_off(m, k, K) * 2], &got[oXn + xp_off(m, k, K) * 2], 2);
        memcpy(&E[oA], &got[oA], (size_t)M * N * 4); memcpy(&E[oC], &got[oA], (size_t)M * N * 4); if (do1) memcpy(&E[oB], &got[oA], (size_t)M * N * 4);
        for (size_t i = 0; i < (size_t)M * N; ++i) { float f; memcpy(&f, &got[oA + i * 4], 4); if (!(std::fabs(f) < 1e30f)) verdict = "FAIL (NORM 0 output is not finite)"; }
        if (verdict == "OK") verdict = compare(got, E, S, nullptr, names);
    }
    printf("%-100s %-22s %s\n", head, "", g_dev ? verdict.c_str() : (verdict == "OK" ? "ok" : verdict.c_str())); fflush(stdout);
    if (verdict != "OK") ++g_fail;
}

// ---------------------------------------------------------------------------------------------------------------- one-hot attention: the reader side of the KV layouts
// q = 16 e_d and K_p[d] = 8 for ONE attended position p of each (sequence, head), K[d] <= 0 at every other attended one: the score of p exceeds every other by at
// least 128, every other probability underflows to exactly 0 in fp32, L = 1, and the output must be the bits of V_p.  Masked and never-written positions hold
// +-3.0e38 (e4m3 cache: +-448), not NaN, and must not reach the result.  The targets of the (sequence, head) items walk the first / last attended position, pos, and
// both sides of the 16- and 32-position block boundaries.
struct AC { int variant = 41, nsplit = 1, kv8 = 0, packed = 0, b = 1, pos = 40, maskkind = 0 /* 0 none, 1 left pad + jmin table, 2 holes + in-kernel scan, 3 holes + table */, persist = 0 /* 1: pgrid 3, 2: items + helpers */, pf = 0, rot = 0; };
static void run_attn(const AC& c) {
    const unsigned seed = (unsigned)++g_cases;
    const int T = 40, b = c.b, kvb = c.kv8 ? 1 : 2, Mb = (b + 15) / 16, items = b * HH;
    Sess S; std::vector<std::pair<size_t, const char*>> names;
    auto A = [&](const char* nm, size_t bytes) { const size_t o = S.alloc(bytes); names.push_back({o, nm}); return o; };
    const size_t oQ = A("q", (size_t)b * HH * 64 * 2), oKc = A("kc", (size_t)b * HH * SA * 64 * kvb), oVc = A("vc", (size_t)b * HH * SA * 64 * kvb), oPos = A("pos", 4), oM = A("mask", (size_t)b * T), oJ = A("jmin", (size_t)b * 4);
    const size_t oO = A("out", c.packed ? (size_t)Mb * 16 * DIM * 2 : (size_t)b * DIM * 2), oPart = A("part", (size_t)b * HH * 4 * 66 * 4), oPf = A("helper scratch", 32 * 1024);
    memset(&S.img[oPf], 0x5a, 32 * 1024); put_i32(S.img, oPos, 0, c.pos);
    HOSTCHECK(c.pos >= T && c.pos < SA && (c.nsplit == 1 || c.nsplit == 4), "attention case");
    std::vector<unsigned char> E;
    std::vector<std::pair<int, int>> tg(items);
    for (int i = 0; i < b; ++i) {
        std::vector<int> att;
        int jm = T;
        for (int j = 0; j < T; ++j) {
            bool v = true;
            if (c.maskkind == 1) v = j >= (i * 7 + 3) % T; else if (c.maskkind >= 2) v = (hsh((unsigned)i, (unsigned)j, seed) % 3u) != 0 || j == T - 1;
            S.img[oM + (size_t)i * T + j] = v ? 1 : 0; if (v && j < jm) jm = j; if (v) att.push_back(j);
        }
        put_i32(S.img, oJ, i, c.maskkind ? jm : 0);
        for (int j = T; j <= c.pos; ++j) att.push_back(j);
        std::vector<int> cd = {att.front(), att.back(), att[att.size() / 2], att.size() > 1 ? att[1] : att[0], att.size() > 1 ? att[att.size() - 2] : att[0]};
        for (int a : att) if ((a & 15) == 0 || (a & 15) == 15 || (a & 31) == 1 || (a & 31) == 17) cd.push_back(a);
        for (int h = 0; h < HH; ++h) {
            const int it = i * HH + h, pt = cd[(size_t)(it + c.rot) % cd.size()], dt = (int)(hsh((unsigned)it, 9u, seed) & 63u);
            tg[it] = {pt, dt};
            const size_t sb = ((size_t)i * HH + h) * SA * 64;
            for (int d = 0; d < 64; ++d) put_bf(S.img, oQ, (size_t)it * 64 + d, d == dt ? 16.f : 0.f);
            std::vector<char> isatt(SA, 0); for (int a : att) isatt[a] = 1;
            for (int pp = 0; pp < SA; ++pp) for (int d = 0; d < 64; ++d) {
                float kv, vv;
                if (isatt[pp]) { kv = d == dt ? (pp == pt ? 8.f : -(float)(hsh((unsigned)(it * SA + pp), 3u, seed) % 9u)) : (float)((int)(hsh((unsigned)(it * SA + pp), (unsigned)d, seed * 2u) % 17u) - 8); vv = (float)((int)(hsh((unsigned)(it * SA + pp), (unsigned)d, seed * 2u + 1u) % 33u) - 16); }
                else { const float big = c.kv8 ? 448.f : 3.0e38f; kv = ((pp + d) & 1) ? big : -big; vv = ((pp + d) & 1) ? -big : big; if (!c.kv8) { kv = rbf(kv); vv = rbf(vv); } }
                if (c.kv8) { S.img[oKc + sb + k8_off(pp, d)] = e4m3_encode(kv); S.img[oVc + sb + v8_off(pp, d)] = e4m3_encode(vv); HOSTCHECK(e4m3_round(kv) == kv && e4m3_round(vv) == vv, "e4m3 cache value"); }
                else { put_bf(S.img, oKc, sb + k_off(pp, d), kv); put_bf(S.img, oVc, sb + v_off(pp, d), vv); }
            }
        }
    }
    E = S.img;
    for (int it = 0; it < items; ++it) for (int d = 0; d < 64; ++d) {
        const int i = it / HH, h = it % HH, k = h * 64 + d;
        const float vv = (float)((int)(hsh((unsigned)(it * SA + tg[it].first), (unsigned)d, seed * 2u + 1u) % 33u) - 16);
        put_bf(E, oO, c.packed ? xp_off(i, k, DIM) : (size_t)i * DIM + k, vv);
    }
    Attn2P a; memset(&a, 0, sizeof a);
    a.q = S.dp<bf16_t>(oQ); a.kc = S.dp<bf16_t>(oKc); a.vc = S.dp<bf16_t>(oVc); a.pos = S.dp<int>(oPos); a.mask = c.maskkind ? S.dp<unsigned char>(oM) : nullptr; a.jmin = (c.maskkind == 1 || c.maskkind == 3) ? S.dp<int>(oJ) : nullptr;
    a.out = S.dp<bf16_t>(oO); a.part = S.dp<float>(oPart); a.H = HH; a.SA = SA; a.T = T; a.dim = DIM; a.nsplit = c.nsplit; a.out_packed = c.packed; a.kv8 = c.kv8;
    if (c.persist) { a.n_seq = b; a.pgrid = c.persist == 1 ? 3 : items + c.pf; }
    if (c.pf) { a.pf_p0 = S.dp<char>(oPf); a.pf_b0 = 32 * 1024; a.pf_wgs = c.pf; HOSTCHECK(c.pf % 8 == 0, "helpers"); }
    // extents: whole 32-position blocks up to the one that holds pos, the mask row, q, out, the partials
    S.extent("kc", oKc, ((size_t)(b * HH - 1) * SA * 64 + (size_t)((c.pos >> 5) + 1) * 32 * 64) * kvb); S.extent("vc", oVc, ((size_t)(b * HH - 1) * SA * 64 + (size_t)((c.pos >> 5) + 1) * 32 * 64) * kvb);
    S.extent("q", oQ, (size_t)b * HH * 64 * 2); S.extent("mask", oM, (size_t)b * T); S.extent("jmin", oJ, (size_t)b * 4); S.extent("part", oPart, (size_t)b * HH * c.nsplit * 66 * 4);
    S.extent("out", oO, c.packed ? (xp_off(b - 1, DIM - 1, DIM) + 1) * 2 : (size_t)b * DIM * 2);
    char head[220]; snprintf(head, sizeof head, "one-hot attention | variant %d nsplit %d %s %s b %d pos %d mask %s%s%s", c.variant, c.nsplit, c.kv8 ? "kv8" : "bf16", c.packed ? "packed" : "rows", b, c.pos,
        c.maskkind == 0 ? "none" : c.maskkind == 1 ? "left pad, table" : c.maskkind == 2 ? "holes, in-kernel scan" : "holes, table", c.persist == 1 ? ", persistent grid 3" : c.persist == 2 ? ", persistent grid + helpers" : "", (c.pf && !c.persist) ? ", helpers" : "");
    if (!g_dev) { printf("%-100s %-22s ok\n", head, ""); return; }
    S.upload();
    car_launch_dec_attn2_var(&a, b, c.variant, 0, 0); ++g_launches;
    std::vector<unsigned char> got; S.download(got);
    memcpy(&E[oPart], &got[oPart], (size_t)b * HH * c.nsplit * 66 * 4);          // the split partials are scratch: only their extent is checked (the guard behind them)
    std::string verdict = compare(got, E, S, nullptr, names);
    printf("%-100s %-22s %s\n", head, "", verdict.c_str()); fflush(stdout);
    if (verdict != "OK") ++g_fail;
}

// ---------------------------------------------------------------------------------------------------------------- host-only checks
static void selftest_host() {
    // e4m3 encoder against all 256 codes, the named ties and the clamp
    { int bad = 0; for (int cde = 0; cde < 256; ++cde) { if ((cde & 0x7f) == 0x7f) continue; if (e4m3_encode(e4m3_decode((unsigned char)cde)) != cde) ++bad; }
      if (e4m3_round(17.f) != 16.f || e4m3_round(19.f) != 20.f || e4m3_round(500.f) != 448.f || e4m3_round(-1e9f) != -448.f || e4m3_encode(448.f) != 0x7e || e4m3_encode(-0.f) != 0x80) ++bad;
      printf("selftest: e4m3 encoder over the 254 number codes, ties 17 -> 16 and 19 -> 20, clamp 500 -> 448: %s\n", bad ? "FAIL" : "ok"); if (bad) ++g_fail; }
    // layout formulas against the lane maps of the attention's edge trim, and as bijections of a stream
    { int bad = 0;
      for (int p = 0; p < 64; ++p) for (int d = 0; d < 64; ++d) {
          const size_t ko = k_off(p, d) - (size_t)(p >> 5) * 2048, vo = v_off(p, d) - (size_t)(p >> 5) * 2048;       // inside the 32-position block: four 1 KiB loads each
          const int ki = (int)(ko / 512), kl = (int)(ko % 512) / 8, vl = (int)(vo % 512) / 8;
          if (!attn2_edge_k_lane(ki, kl, p & 31, p & 31) || (d >> 5) != (ki & 1)) ++bad;
          if (!attn2_edge_v_lane(vl, p & 31, p & 31) || (int)(vo / 512) != (d >> 4)) ++bad;
          for (int o = 0; o < 32; ++o) { if (attn2_edge_k_lane(ki, kl, o, o) != (o == (p & 31))) ++bad; const int g = vl >> 4; const bool in = (o >= 4 * g && o < 4 * g + 4) || (o >= 16 + 4 * g && o < 20 + 4 * g); if (attn2_edge_v_lane(vl, o, o) != in) ++bad; }
      }
      std::vector<int> seen(4 * SA * 64, 0);
      for (int p = 0; p < SA; ++p) for (int d = 0; d < 64; ++d) { ++seen[k_off(p, d)]; ++seen[SA * 64 + v_off(p, d)]; ++seen[2 * SA * 64 + k8_off(p, d)]; ++seen[3 * SA * 64 + v8_off(p, d)]; }
      for (int v : seen) if (v != 1) ++bad;
      printf("selftest: K / V / K8 / V8 layout formulas: bijections of a stream, lanes agree with attn2_edge_k_lane / attn2_edge_v_lane: %s\n", bad ? "FAIL" : "ok"); if (bad) ++g_fail; }
    // sign rows: rnd(2^a * rstd) = 1 for every candidate rstd within 2 ulp of the correctly rounded one, eps = 1e-5 and 0
    { int bad = 0;
      for (int a = 0; a < 4; ++a) for (float eps : {1e-5f, 0.f}) {
          const float mean = ldexpf(1.f, 2 * a) + eps; float cnd = (float)(1.0 / std::sqrt((double)mean));
          float lo = cnd, hi = cnd; for (int i = 0; i < 2; ++i) { lo = nextafterf(lo, 0.f); hi = nextafterf(hi, 2.f); }
          for (float rr = lo; rr <= hi; rr = nextafterf(rr, 2.f)) if (rbf(ldexpf(1.f, a) * rr) != 1.f) ++bad;
      }
      printf("selftest: sign rows: rnd(v * rstd) = +-1 for every rstd within 2 ulp of 1/sqrt(4^a + eps), a = 0..3, eps = 1e-5 and 0: %s\n", bad ? "FAIL" : "ok"); if (bad) ++g_fail; }
    // car_pick_gemm_cfg followed by the route function over the engine's linears
    { int bad = 0, n = 0;
      const int Ms[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 32, 48, 49, 64, 96, 128, 192, 256, 384, 768};
      const int dims[5] = {768, 1024, 1280, 1536, 2048}, hid[5] = {2048, 2816, 3584, 4096, 5632};
      for (int M : Ms) for (int di = 0; di < 5; ++di) for (int lin = 0; lin < 5; ++lin) for (int form = 0; form < 4; ++form) for (int f8 = 0; f8 < 3; ++f8) {
          const int d = dims[di], N = lin == 0 ? 3 * d : lin == 1 ? d : lin == 2 ? 2 * hid[di] : lin == 3 ? d : 16384, K = lin == 3 ? hid[di] : d;
          const int epi = lin == 0 ? EPI_QKV : (lin == 1 || lin == 3) ? EPI_RESID : lin == 2 ? EPI_SWIGLU : EPI_LOGITS;
          if (form && epi == EPI_RESID) continue;                    // a residual linear never follows a norm
          if (form == 3 && (M > 16 || K > 2048)) continue;           // the fused prologue norm: one m-block chains
          GemmDP p; memset(&p, 0, sizeof p); p.M = M; p.N = N; p.K = K; p.W = (const bf16_t*)16; p.X = (const bf16_t*)16; if (f8) { p.wscale = (const float*)16; p.f8_mfma = f8 == 2; }
          if (form) { p.nw = (const bf16_t*)16; p.nh_in = (const bf16_t*)16; }
          if (form == 1) { p.ssq_in = (const float*)16; p.ssq_np = d / 32; }
          if (form == 2) { p.ssq_in = (const float*)16; p.ssq_np = d / 16; }
          const int cfg = car_pick_gemm_cfg(M, N, K, epi);
          DecGemmRoute r; ++n;
          if (car_dec_gemm_route(&p, epi, cfg, 1, &r)) { if (bad < 5) printf("  refused: M %d N %d K %d epi %d cfg %d form %d f8 %d\n", M, N, K, epi, cfg, form, f8); ++bad; continue; }
          if (form == 3 ? r.NORM != 1 : form ? (r.NORM != 2 && r.NORM != 3) : r.NORM != 0) ++bad;
          if (r.F8 != f8 || r.I * 100 + r.J * 10 + (r.WAVES == 8) != (cfg == 112 ? 110 : cfg) || (cfg == 112 && r.WAVES != 16)) ++bad;
      }
      printf("selftest: car_pick_gemm_cfg -> car_dec_gemm_route over %d (M, linear, norm form, weight format) combinations of the engine: %s\n", n, bad ? "FAIL" : "none refused, routes as picked  ok"); if (bad) ++g_fail; }
}

static int deep_k(int I, int J, int WAVES, int f8) {      // every wave's slice exceeds 2 x DEPTH stages (DEPTH: the kernel's own formula)
    const int XPU = f8 ? 2 : 1, q = 28 / (I + J * XPU), DEPTH = WAVES == 16 ? 8 : (q < 2 ? 2 : (q > 6 ? 6 : q));
    return (2 * DEPTH + 1) * WAVES * 32 * XPU;
}

int main(int argc, char** argv) {
    const std::string md = argc > 1 ? argv[1] : "quick";
    if (md != "quick" && md != "selftest") { printf("usage: decode_check [quick | selftest]\n"); return 2; }
    g_dev = md == "quick";
    const auto t0 = std::chrono::steady_clock::now();
    if (g_dev) CK(hipMalloc(&g_arena, ARENA));
    selftest_host();
    static const int Ms[7] = {1, 2, 5, 16, 17, 50, 70}, Ps[7] = {0, 15, 16, 31, 32, 33, SA - 1};
    int mi = 0, pi = 0, kvi = 0;
    std::vector<int> cfgs; for (int I : {1, 2, 4}) for (int J : {1, 2, 4}) for (int w : {0, 1}) cfgs.push_back(I * 100 + J * 10 + w); cfgs.push_back(112);
    GC c;
    // ================================================================= routing: every tile shape x every epilogue x F8 0 / 1 / 2 (K = 352 / 704: an uneven split)
    for (int cfg : cfgs) for (int f8 = 0; f8 < 3; ++f8) {
        const int I = cfg / 100, J = (cfg / 10) % 10, WAVES = cfg == 112 ? 16 : (cfg % 10 ? 8 : 4), Ku = f8 ? 704 : 352;
        // K: fewer k-units than waves; uneven; deep (refill more than once).  N: main grid a multiple of 8 (XCD remap on) / 3 row tiles (off)
        c = GC(); c.name = "K < waves"; c.cfg = cfg; c.f8 = f8; c.M = Ms[mi++ % 7]; c.N = 16 * I * 8; c.K = f8 ? 64 : 32; run_gemm(c);
        c = GC(); c.name = "K uneven, ragged m-tile"; c.cfg = cfg; c.f8 = f8; c.M = J > 1 ? 70 : Ms[mi++ % 7]; c.N = 16 * I * 3; c.K = Ku; c.w_nt = 0; run_gemm(c);
        c = GC(); c.name = "K deep"; c.cfg = cfg; c.f8 = f8; c.M = Ms[mi++ % 7]; c.N = 16 * I * ((mi & 1) ? 8 : 3); c.K = deep_k(I, J, WAVES, f8); run_gemm(c);
        c = GC(); c.name = "logits, helpers"; c.cfg = cfg; c.f8 = f8; c.M = Ms[mi++ % 7]; c.N = 16 * I * 8; c.K = Ku; c.pf = 8; run_gemm(c);
        for (int s = 0; s < 2; ++s) { c = GC(); c.name = "resid"; c.cfg = cfg; c.f8 = f8; c.epi = EPI_RESID; c.ssq = s; c.M = s ? (mi & 1 ? 5 : 16) : Ms[mi % 7]; if (s && (mi % 3) == 0) c.M = Ms[4 + mi % 3]; ++mi; c.N = 32 * I * (s ? 3 : 4); c.K = Ku; c.w_nt = s ? 1 : 3; run_gemm(c); }
        if (I >= 2) { c = GC(); c.name = "swiglu"; c.cfg = cfg; c.f8 = f8; c.epi = EPI_SWIGLU; c.M = Ms[mi++ % 7]; c.N = (mi & 1) ? 256 : 192; c.K = Ku; run_gemm(c); }
        c = GC(); c.name = "qkv"; c.cfg = cfg; c.f8 = f8; c.epi = EPI_QKV; c.M = Ms[mi++ % 7]; c.N = 384; c.K = Ku; c.pos = Ps[pi++ % 7]; c.kv8 = kvi++ & 1; run_gemm(c);
    }
    // ================================================================= RESID + ssq at M > 16 on every I, helpers next to a residual / QKV epilogue
    for (int cfg : {110, 111, 112, 121, 141, 211, 221, 240, 411, 420, 441}) { c = GC(); c.name = "resid M > 16"; c.cfg = cfg; c.epi = EPI_RESID; c.ssq = true; c.M = cfg % 2 ? 50 : 17; c.N = 32 * (cfg / 100) * 4; c.K = 352; run_gemm(c); }
    c = GC(); c.name = "resid, helpers"; c.cfg = 112; c.epi = EPI_RESID; c.ssq = true; c.M = 2; c.N = 128; c.K = 352; c.pf = 16; run_gemm(c);
    c = GC(); c.name = "qkv, helpers"; c.cfg = 211; c.epi = EPI_QKV; c.M = 5; c.N = 384; c.K = 352; c.pos = 33; c.pf = 8; run_gemm(c);
    // ================================================================= SwiGLU: sums far beyond 8 bits (the pre-gate rounding matters)
    for (int cfg : {211, 240, 441}) for (int f8 = 0; f8 < 3; ++f8) { c = GC(); c.name = "swiglu dense"; c.cfg = cfg; c.f8 = f8; c.epi = EPI_SWIGLU; c.dense = true; c.M = cfg == 211 ? 16 : 70; c.N = 256; c.K = 256; run_gemm(c); }
    // ================================================================= QKV: every position x bf16 / e4m3 rows x prologue (M <= 16) / late read (M = 17, 50)
    for (int pos : Ps) for (int kv8 = 0; kv8 < 2; ++kv8) for (int M : {5, 17, 50}) {
        static const int tc[6] = {211, 111, 120, 241, 411, 110};
        c = GC(); c.name = "qkv positions"; c.cfg = tc[(pi++) % 6]; c.f8 = (pi / 6) % 3; c.epi = EPI_QKV; c.M = M; c.N = 384; c.K = c.f8 ? 128 : 64; c.pos = pos; c.kv8 = kv8; run_gemm(c);
    }
    c = GC(); c.name = "qkv, q in the bf16 subnormal range"; c.cfg = 211; c.f8 = 1; c.epi = EPI_QKV; c.M = 16; c.N = 384; c.K = 128; c.pos = 33; c.tiny = true; run_gemm(c);
    // ================================================================= norm forms on sign rows
    static const int epis[3] = {EPI_LOGITS, EPI_SWIGLU, EPI_QKV};
    int ei = 0, fi = 0, gi = 0;
    auto norm_case = [&](const char* nm, int cfg, int norm, int M, int K, int staged_ok) {
        GC n; n.name = nm; n.cfg = cfg; n.norm = norm; n.src = 1; n.M = M; n.K = K; n.staged_ok = staged_ok;
        n.epi = epis[ei++ % 3]; if (n.epi == EPI_SWIGLU && cfg < 200) n.epi = epis[ei++ % 3]; if (n.epi == EPI_SWIGLU && cfg < 200) n.epi = EPI_LOGITS;
        n.f8 = (fi++ / 3) % 3; n.N = n.epi == EPI_QKV ? 384 : n.epi == EPI_SWIGLU ? 128 : 16 * (cfg / 100) * 3; if (n.epi == EPI_SWIGLU && n.N % (16 * (cfg / 100))) n.N = 256;
        n.pos = Ps[pi++ % 7]; n.kv8 = kvi++ & 1; n.eps = (gi & 4) ? 0.f : 1e-5f;
        if (norm <= 1) { n.gather = gi & 1; n.add = (gi >> 1) & 1; n.poslast = (gi >> 3) & 1; n.nhout = (gi % 3) != 0; if (n.pos < NTOK) n.pos += 16; }
        n.rI = (hsh((unsigned)gi, 7u, 1u) & 1u) ? 1 : 2; ++gi;      // (hashed: not in step with the D cycles of the callers, so that D = 768 / 1280 meet both partial widths: ssq_np 24, 40, 80)
        return n;
    };
    // rmsnorm2_kernel -> packed xn -> NORM 0 (the three NQ instantiations, ragged last workgroup)
    for (int D : {256, 768, 1280, 2048, 4096}) for (int rows : {1, 4, 5, 37}) { static const int tc[5] = {111, 211, 120, 241, 410}; run_gemm(norm_case("rmsnorm2 -> xn -> NORM 0", tc[gi % 5], 0, rows, D, 1)); }
    // NORM 1: the six tiles, M > WAVES takes the second-row path
    for (int cfg : {110, 111, 210, 211, 410, 411}) for (int M : {1, 5, 8, 9, 16}) { static const int Ds[4] = {256, 768, 1280, 2048}; run_gemm(norm_case("NORM 1 (prologue norm)", cfg, 1, M, Ds[gi % 4], 1)); }
    // NORM 2: every tile (8-wave one-m-block tiles at M <= 16 only with staged_ok = 0), J = 4 at M = 50 (cfg 141 / 241: the normx_j4 route)
    for (int cfg : cfgs) { if (cfg == 112) continue; for (int rep = 0; rep < 3; ++rep) {
        static const int Ds[3] = {256, 768, 1280};
        const int J = (cfg / 10) % 10; int M = Ms[mi++ % 7]; if (J == 4 && rep == 0) M = 50;
        const bool one = M <= 16 && J == 1 && cfg % 10 == 1;
        GC n = norm_case("NORM 2 (on the fly)", cfg, 2, M, Ds[(gi + rep) % 3], one ? 0 : 1); if (n.f8 != rep) { n.f8 = rep; } run_gemm(n);
    } }
    // NORM 3: I x M x K (K = 256: nku = 8 is the minimum; with e4m3 weights nku = 4 and the launcher must fall back to NORM 2)
    for (int cfg : {111, 211, 411}) for (int M : {1, 2, 5, 16}) for (int K : {256, 768, 1280}) {
        GC n = norm_case("NORM 3 (staged)", cfg, 3, M, K, 1); if (n.f8 && K == 256) { n.norm = 2; n.name = "NORM 3 ineligible (nku 4) -> NORM 2"; } run_gemm(n);
    }
    // ================================================================= the prefill writer, and a decode-time row behind it
    for (int Tn : {1, 33, 40}) for (int t0s : {0, 7, 32}) for (int kv8 = 0; kv8 < 2; ++kv8) run_prefill(Tn, t0s, kv8);
    // ================================================================= general integer rows: rmsnorm2 against the rstd candidates, the fused forms against rmsnorm2 + NORM 0
    { int gi2 = 0;
      for (int D : {256, 768, 1280, 2048, 4096}) for (int rows : {1, 4, 5, 37}) { static const int tc[6] = {111, 211, 411, 110, 221, 141}; run_general(rows > 16 ? tc[3 + gi2 % 3] : tc[gi2 % 3], gi2 % 3, rows, D, ((gi2 & 1) && D < 4096) ? 1 : 2); ++gi2; }      // (D = 4096 with one-row-block partials: ssq_np 256 > 128)
      for (int cfg : {111, 211, 411, 410, 210}) for (int M : {2, 9, 16}) { run_general(cfg, gi2 % 3, M, (gi2 & 1) ? 768 : 1280, (gi2 % 3) ? 2 : 1); ++gi2; } }
    // ================================================================= one-hot attention
    { static const int Bs[3] = {1, 8, 17}, Pp[7] = {40, 47, 48, 63, 64, 65, SA - 1}; int ai = 0;
      for (int kv8 = 0; kv8 < 2; ++kv8) for (int variant : {20, 21, 40, 41, 80, 81, 160, 161}) for (int nsplit : {1, 4}) {
          AC a; a.variant = variant; a.nsplit = nsplit; a.kv8 = kv8; a.b = Bs[ai % 3]; a.packed = (ai >> 1) & 1; a.pos = Pp[ai % 7]; a.maskkind = ai % 4; a.rot = ai; run_attn(a); ++ai;
      }
      for (int kv8 = 0; kv8 < 2; ++kv8) for (int pf : {0, 8}) for (int bb : {8, 17, 1}) for (int mk : {0, 1, 3}) {
          if (pf && bb != 8) continue;
          AC a; a.variant = 162; a.kv8 = kv8; a.b = bb; a.pf = pf; a.maskkind = mk; a.packed = ai & 1; a.pos = Pp[ai % 7]; a.rot = ai; run_attn(a); ++ai;
      }
      for (int kv8 = 0; kv8 < 2; ++kv8) for (int variant : {40, 161}) for (int persist : {1, 2}) for (int bb : {8, 17}) {
          AC a; a.variant = variant; a.kv8 = kv8; a.b = bb; a.persist = persist; a.pf = persist == 2 ? 8 : 0; a.maskkind = 1 + ai % 3; a.packed = ai & 1; a.pos = Pp[ai % 7]; a.rot = ai; run_attn(a); ++ai;
      }
      for (int rot = 0; rot < 12; ++rot) { AC a; a.variant = rot & 1 ? 162 : 41; a.kv8 = (rot >> 1) & 1; a.b = 1; a.pos = Pp[rot % 7]; a.maskkind = rot % 4 == 2 && (rot & 1) ? 3 : rot % 4; a.rot = 100 + rot; run_attn(a); } }
    // ================================================================= refusals: non-zero, nothing launched, nothing written
    run_refusal("EPI_SWIGLU with I = 1", EPI_SWIGLU, 111, 5, 128, 64, 0, 0, 0);
    run_refusal("N % (16 I)", EPI_LOGITS, 211, 5, 48, 64, 0, 0, 0);
    run_refusal("N % (16 I), I = 4", EPI_LOGITS, 411, 5, 96, 64, 0, 0, 0);
    run_refusal("K % 32", EPI_LOGITS, 111, 5, 64, 48, 0, 0, 0);
    run_refusal("wscale with K % 64", EPI_LOGITS, 111, 5, 64, 96, 1, 0, 0);
    run_refusal("wscale (W8A8) with K % 64", EPI_LOGITS, 211, 5, 64, 96, 2, 0, 0);
    run_refusal("ssq_in with ssq_np 0", EPI_LOGITS, 211, 5, 64, 256, 0, 2, 0);
    run_refusal("ssq_in with ssq_np 6", EPI_LOGITS, 211, 5, 64, 256, 0, 2, 6);
    run_refusal("ssq_in with ssq_np 132", EPI_LOGITS, 211, 5, 64, 256, 0, 2, 132);
    run_refusal("ssq_in with EPI_RESID", EPI_RESID, 211, 5, 64, 256, 0, 2, 8);
    run_refusal("ssq_in with cfg 112", EPI_LOGITS, 112, 5, 64, 256, 0, 2, 8);
    run_refusal("fused norm with M 17", EPI_LOGITS, 211, 17, 64, 256, 0, 1, 0);
    run_refusal("fused norm with J 2", EPI_LOGITS, 221, 5, 64, 256, 0, 1, 0);
    run_refusal("fused norm with K 2080", EPI_LOGITS, 211, 5, 64, 2080, 0, 1, 0);
    run_refusal("fused norm with EPI_RESID", EPI_RESID, 211, 5, 64, 256, 0, 1, 0);
    run_refusal("fused norm with cfg 112", EPI_LOGITS, 112, 5, 64, 256, 0, 1, 0);
    for (int cfg : {0, 11, 310, 113, 150, 511, 999}) { char nm[48]; snprintf(nm, sizeof nm, "unknown cfg %d", cfg); run_refusal(nm, EPI_LOGITS, cfg, 5, 960, 64, 0, 0, 0); }

    printf("e4m3 content of the cases: KV rows %d ties / %d beyond 448, W8A8 activations %d ties / %d beyond 448\n", kv8_ties, kv8_clamps, x8_ties, x8_clamps);
    if (!kv8_ties || !kv8_clamps || !x8_ties || !x8_clamps) { printf("PRECONDITION FAIL (harness): the cases hold no e4m3 tie or no value beyond 448\n"); ++g_fail; }
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%d cases, %d launches (%s), wall %.1f s\n", g_cases, g_launches, md.c_str(), wall);
    if (g_fail) { printf("%d check(s) FAILED\n", g_fail); return 1; }
    printf(g_dev ? "all checks passed\n" : "selftest passed\n");
    return 0;
}
