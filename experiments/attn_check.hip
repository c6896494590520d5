// experiments/attn_check.hip — the batched attention path behind attn_run (controlar_amd/csrc/engine_attn.hip) against EXACT and fp64 references:
// flash64_kernel<QT, MODE> (attn.hip) in the bf16 mode, transpose_pad_kernel -> car_launch_gemm -> softmax_wave / softmax_reg / softmax / t5_softmax kernel ->
// car_launch_gemm in the exact mode and, with CAR_NO_FLASH=1, in the bf16 mode.  The harness includes the product sources and drives attn_run ITSELF on a
// default-constructed car_ctx (mode, esz, ws[4..6] sized by attn_bytes and pointing into the case's arena); only the Tq != Tk cases and the refusals call
// car_launch_flash64 directly, and the row-softmax section calls car_launch_softmax / car_launch_softmax_at (and, as comparators, the kernels).
// Built with -DCAR_DEV_KNOBS: CAR_NO_FLASH is read once per process (use_flash), so the unfused bf16 form is a second invocation with CAR_NO_FLASH=1, which
// runs the bf16 unfused cases only.
//
// FRAMING.  Every case lives in one arena poisoned with 0xff bytes (NaNs): inputs, mask, bias, out plus two rows behind it, the three scratch planes, 1 KiB
// guards around each.  After the run every byte outside {out[nb][T][D], S, P, V^T} must be unchanged (memcmp); V^T must hold the bits of V with zero pad columns,
// every P pad column must be zero; the case runs twice from the same image and both post-images must be equal ("BITS DIFFER").  Both layouts: separate planes
// (ld = D) and the packed wqkv rows (ld = 3D).  H = 2, nb = 3, T in {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 120, 128, 129, 192, 193, 197, 257}: the 16-query
// tile, the 32-key block, the 64 QT workgroup, the QT switch (192 | 193), one / two / three workgroups along x at QT = 2 (T <= 128 | 129.. | 257), the causal
// trim (last >> 5) + 1 on a block edge.  Masks per batch row (so the mask's batch stride matters), rotating with T: left padding, right padding, holes, a fully
// masked row (causal: only the diagonal attends; T5: the documented uniform distribution over all Tk keys).
//
// 1. EXACT, no tolerance.
//   uniform   Q = 0: every allowed score is 0 (T5 with a bias of 0 / -128: exp(-128 - 0) is exactly 0 in fp32, so the bias acts as a second mask that differs per
//             head and query), every probability exactly 1, l = the count of attended keys.  V holds integers in +-[1, 4]: the accumulators are exact integers.
//             Fused: the 64 values of a (batch, head, query) must be rnd(sum * inv) for ONE of three inv: the correctly rounded 1 / count and its two neighbours (as
//             decode_check treats rsqrtf).  Unfused bf16: the P row must be rnd(inv) on exactly the attended keys and 0 elsewhere, for one of the three; P v products
//             (8 x 4 bits) and their sums (< 2^20 units) are exact in fp32 in any order, so out = rnd(rnd(inv) * sum).  fp32: the P row is pinned the same way (bits of
//             inv), but inv * v carries 24 bits and the GEMM's sum is not exact: out is held to the fp32 bound of section 2 (one key more or less moves it by >= 1e-3).
//   one-hot   K_j = 8 e_{j % 17} + 8 e_{17 + j / 17} + j e_63, Q_i = 2^16 (e_{w % 17} + e_{17 + w / 17}) + 1024 e_63 (dimensions rotated by 5 per head), scale 1/8:
//             the winner w(b, h, i) leads every allowed key by >= 2^15 and ANY two allowed keys differ by >= 128 after scaling.  So at every block of the online
//             softmax exactly one probability is 1 and the others are exactly 0, no matter which block the winner sits in: out must be the bits of V_w.  Winners at
//             0, 15, 16, 31, 32, 33, T - 1 (where allowed; else the diagonal / first allowed key), chosen per (b, h, i).  V rows that never win and masked rows hold
//             +-3e38.  (With tied losers, as a bias of 0 / -128 alone gives, a block in front of the winner would sum several 3e38 to inf and inf * alpha(0) = NaN: a
//             property of online softmax at the edge of the format, not a fault.  So the T5 one-hot kind whose winner is set by Q K^T (no e_63 term: T5 rounds its
//             scores to bf16) under a hashed 0 / -128 bias gives allowed non-winners +-2^100 and only masked rows +-3e38.  The kind whose winner is set by the bias
//             ALONE, Q = 0, uses the ladder bias[h][i][j] = -128 ((j - w0(h, i)) mod Tk), exact in bf16: the first allowed key at or after w0 wins in every batch
//             row — the bias has no batch axis, the masks do — all keys are >= 128 apart again, and the losers hold +-3e38.)
//   softmax   softmax_reg_kernel at col0 = 0 == softmax_kernel (launched directly) bit for bit, dense scores, plain and causal, fp32 and bf16 stores; window
//             invariance of softmax_wave_kernel and softmax_reg_kernel: a row over the full prefix with the first c columns masked == the row on the window
//             starting at c (col0 = c), c in {5, 16, 48}, on the surviving columns.  (c = 5 is added for a window that is no multiple of the 16-lane groups.  For the WAVE kernel the
//             property holds by more than the lane rule: wave_sum's xor butterfly 32, 16, .., 1 is invariant under ANY cyclic rotation of the 64 lanes, and the
//             masked prefix puts exact zeros into the lanes that wrap, so a kernel that took the lane relative to the window would give the same bits — that
//             mutant is equivalent, experiments/README.md.  The register kernel's block_sum adds its four waves in sequence and is not invariant: there the
//             absolute position is what the equality rests on.)
//   refusals  every condition of car_launch_flash64 violated alone returns -1 and writes nothing; attn_run passes the refusal on with `out` untouched.
// 2. DENSE against an fp64 softmax, bound DERIVED (not measured), checked on every (batch, head, query, d).  Q, K hashed integers in [-3, 3]: every score is an
//   exact integer times the scale in fp32 (checked per element), so T5's rnd(rnd(x) + bias) is replayed without a tie flipping.  V, bias random bf16.
//   With o* = sum p_j v_j, A = sum p_j |v_j|, u = 2^-24, ub = 2^-8 (unit roundoffs of fp32 and bf16: half the spacing of 24 and 8 significant bits), X = the largest max - min of the allowed scores of a row, n = Tk,
//   nblk = ceil(Tk / 32):   |o - o*| <= c1 A + c2 |o*| + c3.
//   fused (attn.hip's rounding points): p^_j = bf16(e^(s_j - base_k)) prod alpha_k'.  e^ = v_exp_f32(x log2e): one rounding of the product and the constant's
//     error on an argument <= X log2e, one ulp of the instruction: relative ee = (1 + X) 2^-23.  alpha has the same error plus one multiply, there are < nblk of
//     them; the MFMA adds n products (exact in fp32) with at most one ulp per add.  etaN = ub + nblk ee + (nblk + n) 2u.  l is summed from UNROUNDED e^: 7 adds in
//     the lane, 2 shuffles, one multiply and add per later block: etaL = nblk ee + (n + 10 + 2 nblk) u.  inv: one ulp (2u); acc * inv: u; one bf16 rounding of the
//     result.  c1 = 1.01 etaN (1 + ub), c2 = ub + 1.01 (etaL + 3u)(1 + ub), c3 = 1e-35 (flushed subnormals).  1.01 covers the second-order terms (eta <= 3e-3).
//   unfused bf16 (ops.hip, t5.hip, gemm.hip): e^ = expf (1 ulp), sum of n positive terms in any order (n u), inv one ulp, one multiply, P rounded AFTER
//     normalisation (ub): etaP = ub + (n + 7) u; the GEMM adds n products in fp32 (2u each); out rounded once.  c1 = 1.01 (1 + ub)(ub + (3n + 7) u), c2 = ub.
//   exact mode: the same without the two bf16 roundings: c1 = 1.01 (3n + 7) u, c2 = 0 — fp32 level.  (T5: the exact mode's scores are fl(x + bias), rnd being the
//     identity there, so its fp64 reference is taken over THOSE scores.)
//   The worst error / bound is printed per case.  `selftest` replays the fused kernel's arithmetic on the host (32-key blocks, running maximum, fp32 expf, bf16
//   probabilities, fp32 accumulators) on every dense case and requires it inside the fused bound: the bound is a property of the algorithm.
//
//   quick      all checks, no timing; prints "all checks passed"   (with CAR_NO_FLASH=1: the bf16 unfused cases only)
//   selftest   host only, no HIP call: every case's data, every precondition, the host emulation, the launcher's refusals
//   time       the old timing cases of flash64_kernel (ViT 1025, prefill 120, T5 120)
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -DCAR_DEV_KNOBS -I controlar_amd/csrc experiments/attn_check.hip -o experiments/attn_check && experiments/attn_check quick && CAR_NO_FLASH=1 experiments/attn_check quick
#ifndef CAR_DEV_KNOBS
#error "attn_check needs -DCAR_DEV_KNOBS: without it CAR_NO_FLASH selects nothing and the second invocation would run the fused kernel again"
#endif
#include "../controlar_amd/csrc/gemm.hip"
#include "../controlar_amd/csrc/gemm_split.hip"
#include "../controlar_amd/csrc/ops.hip"
#include "../controlar_amd/csrc/t5.hip"
#include "../controlar_amd/csrc/attn.hip"
#include "../controlar_amd/csrc/engine_attn.hip"

#include <chrono>
#include <cstdarg>

extern "C" { int g_car_knob_hits = 0; }        // the development build's counter lives in engine.hip, which is not part of this program
unsigned long long g_alloc_gen = 0;            // DevBuf's generation counter, likewise

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)

static int g_fail = 0, g_cases = 0;
static bool g_host_only = false;
static unsigned hsh(unsigned a, unsigned b, unsigned seed) {
    unsigned x = a * 2654435761u + b * 0x85ebca6bu + seed * 0x9e3779b9u; x ^= x >> 15; x *= 2246822519u; x ^= x >> 13; x *= 3266489917u; x ^= x >> 16; return x;
}
static unsigned hsh4(unsigned a, unsigned b, unsigned c, unsigned d, unsigned seed) { return hsh(hsh(a, b, seed), hsh(c, d, seed + 77u), seed + 5u); }
static float rbf(float v) { return bf2f(f2bf(v)); }
static float unit(unsigned h) { return (float)(h & 0xFFFFFF) / 8388608.0f - 1.0f; }      // [-1, 1)
static void fail(const std::string& name, const char* fmt, ...) {
    char b[512]; va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof(b), fmt, ap); va_end(ap);
    printf("  FAIL %s: %s\n", name.c_str(), b); g_fail++;
}

// ---------------------------------------------------------------------------------------------------------------- arena
static const size_t GUARDB = 1024;
struct Arena {
    std::vector<unsigned char> pre, post, post2;
    std::vector<std::pair<size_t, size_t>> wr;        // what the operation may write, in increasing order
    size_t top = 0;
    size_t take(size_t bytes, bool writable = false) {
        top = (top + 255) / 256 * 256 + GUARDB; const size_t o = top; top += bytes;
        if (writable && bytes) wr.push_back({o, bytes});
        return o;
    }
    void finish() { top = (top + 255) / 256 * 256 + GUARDB; pre.assign(top, 0xFF); }
    void put(size_t off, size_t i, int esz, float v) { if (esz == 2) { const bf16_t b = f2bf(v); memcpy(&pre[off + i * 2], &b, 2); } else memcpy(&pre[off + i * 4], &v, 4); }
    // bytes outside the writable ranges that differ between pre and a post-image
    size_t stray(const std::vector<unsigned char>& po) const {
        size_t at = 0, bad = 0;
        auto span = [&](size_t a, size_t b) { if (b > a && memcmp(&pre[a], &po[a], b - a)) for (size_t i = a; i < b; ++i) bad += pre[i] != po[i]; };
        for (auto& r : wr) { span(at, r.first); at = r.first + r.second; }
        span(at, top);
        return bad;
    }
};
static unsigned char* g_dev = nullptr; static size_t g_devcap = 0;
static unsigned char* dev_for(const Arena& a) {
    if (a.top > g_devcap) { if (g_dev) CK(hipFree(g_dev)); g_devcap = a.top + (a.top >> 2); CK(hipMalloc(&g_dev, g_devcap)); }
    return g_dev;
}
// upload the image, run, wait, download — twice; false when a HIP error came back
template <typename F> static bool run_twice(Arena& a, const std::string& name, F&& go) {
    unsigned char* d = dev_for(a);
    for (int r = 0; r < 2; ++r) {
        CK(hipMemcpy(d, a.pre.data(), a.top, hipMemcpyHostToDevice));
        go(d);
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) { printf("  FAIL %s: HIP error %s\n", name.c_str(), hipGetErrorString(e)); g_fail++; exit(2); }
        std::vector<unsigned char>& po = r ? a.post2 : a.post; po.resize(a.top);
        CK(hipMemcpy(po.data(), d, a.top, hipMemcpyDeviceToHost));
    }
    if (memcmp(a.post.data(), a.post2.data(), a.top)) { printf("  BITS DIFFER %s: two runs of the same case\n", name.c_str()); g_fail++; return false; }
    const size_t bad = a.stray(a.post);
    if (bad) { fail(name, "%zu bytes written outside the output and the scratch planes", bad); return false; }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- case data (host, shared by layouts and forms)
enum { CHK_UNI = 0, CHK_UNIB = 1, CHK_HOT = 2, CHK_HOTB = 3, CHK_DENSE = 4 };
static const char* chk_name[] = {"uniform", "uniform+bias", "one-hot", "one-hot-by-bias", "dense"};
static const char* kind_name[] = {"none", "causal", "t5"};
enum { F_FUSED = 0, F_UNF16 = 1, F_UNF32 = 2 };
static const char* form_name[] = {"bf16 fused", "bf16 unfused", "fp32 unfused"};
static const int NB = 3, NH = 2, DH = 64, DM = NH * DH;

struct Data {
    int kind = 0, chk = 0, Tq = 0, Tk = 0; float scale = 0.125f; std::string name;
    std::vector<float> Q, K, V, bias;                 // [NB][T][DM] (values exact in bf16), bias [NH][Tq][Tk]
    std::vector<unsigned char> mask, none;            // [NB][Tk]; none[b]: T5 and every key masked
    std::vector<unsigned char> att;                   // uniform / one-hot: [NB][NH][Tq][Tk] attended flags
    std::vector<int> cnt, win;                        // [NB][NH][Tq]
    std::vector<int> sum;                             // uniform: [NB][NH][Tq][64]
    std::vector<double> o, A;                         // fp64 reference and sum p |v|, [NB][Tq][DM] (uniform and dense)
    std::vector<double> o32, A32;                     // dense T5: the same for the exact mode, whose scores are x + bias without the two bf16 roundings
    std::vector<float> xs;                            // dense: the replayed fp32 score of every (b, h, i, j), -inf where not allowed
    double X = 0; bool pre_ok = true;
    size_t row(int b, int h, int i) const { return ((size_t)b * NH + h) * Tq + i; }
    bool allowed(int b, int i, int j) const {
        if (kind == 0) return true;
        const unsigned char* mk = &mask[(size_t)b * Tk];
        if (kind == 1) return j <= i && (mk[j] || j == i);
        return none[b] || mk[j];
    }
};

static void gen_masks(Data& d, int variant, bool nofull, unsigned seed) {
    static const int table[3][3] = {{0, 2, 3}, {1, 3, 2}, {2, 0, 1}};      // 0 left padding, 1 right padding, 2 holes, 3 fully masked
    const int T = d.Tk;
    d.mask.assign((size_t)NB * T, 0); d.none.assign(NB, 0);
    for (int b = 0; b < NB; ++b) {
        int pat = table[variant % 3][b]; if (pat == 3 && nofull) pat = 1;
        unsigned char* mk = &d.mask[(size_t)b * T];
        const int r = (int)(hsh((unsigned)b, (unsigned)T, seed) % (unsigned)T);
        if (pat == 0) { const int npad = T == 1 ? 0 : 1 + r % (T - 1); for (int j = 0; j < T; ++j) mk[j] = j >= npad; }
        else if (pat == 1) { for (int j = 0; j < T; ++j) mk[j] = j <= r; }
        else if (pat == 2) { for (int j = 0; j < T; ++j) mk[j] = hsh((unsigned)b, (unsigned)j, seed + 1u) % 10u < 7u; mk[r] = 1; }
        if (d.kind == 2) { int any = 0; for (int j = 0; j < T; ++j) any |= mk[j]; d.none[b] = !any; }
    }
}

static void build(Data& d, int kind, int chk, int Tq, int Tk, int variant) {
    d.kind = kind; d.chk = chk; d.Tq = Tq; d.Tk = Tk; d.scale = kind == 2 ? 1.0f : 0.125f;
    const unsigned seed = 1000u * (unsigned)chk + 100u * (unsigned)kind + (unsigned)Tq;
    char nm[96]; snprintf(nm, sizeof(nm), "%-15s %-6s T %3d%s", chk_name[chk], kind_name[kind], Tq, Tq != Tk ? " x 70" : ""); d.name = nm;
    const bool hot = chk == CHK_HOT || chk == CHK_HOTB, uni = chk == CHK_UNI || chk == CHK_UNIB;
    if (kind) gen_masks(d, variant, kind == 2 && hot, seed);
    d.Q.assign((size_t)NB * Tq * DM, 0.f); d.K.assign((size_t)NB * Tk * DM, 0.f); d.V.assign((size_t)NB * Tk * DM, 0.f);
    if (kind == 2) d.bias.assign((size_t)NH * Tq * Tk, 0.f);
    const size_t nrow = (size_t)NB * NH * Tq;
    auto rot = [](int dim, int h) { return (dim + 5 * h) % DH; };
    // ---- K (every kind of check reads it; the hashed integers are the dense operand and a finite filler elsewhere)
    for (int b = 0; b < NB; ++b) for (int j = 0; j < Tk; ++j) for (int h = 0; h < NH; ++h) {
        float* k = &d.K[((size_t)b * Tk + j) * DM + h * DH];
        if (chk == CHK_HOT) { k[rot(j % 17, h)] = 8.f; k[rot(17 + j / 17, h)] = 8.f; k[rot(63, h)] = (float)j; }
        else for (int e = 0; e < DH; ++e) k[e] = (float)((int)(hsh4(b, j, h, e, seed + 2u) % 7u) - 3);
    }
    if (uni || hot) {
        d.att.assign(nrow * Tk, 0); d.cnt.assign(nrow, 0); d.win.assign(nrow, -1);
        if (chk == CHK_UNIB) for (size_t i = 0; i < d.bias.size(); ++i) d.bias[i] = (hsh((unsigned)i, 3u, seed + 3u) & 1u) ? -128.f : 0.f;
    }
    if (uni) {
        d.sum.assign(nrow * DH, 0); d.o.assign((size_t)NB * Tq * DM, 0); d.A.assign(d.o.size(), 0);
        for (size_t i = 0; i < d.V.size(); ++i) { const unsigned h = hsh((unsigned)i, 5u, seed + 4u); d.V[i] = (float)((1 + (int)(h % 4u)) * ((h & 0x100u) ? -1 : 1)); }
        for (int b = 0; b < NB; ++b) for (int h = 0; h < NH; ++h) for (int i = 0; i < Tq; ++i) {
            const size_t r = d.row(b, h, i);
            float mx = -INFINITY;
            auto sc = [&](int j) { return (kind == 2 && !d.none[b]) ? d.bias[((size_t)h * Tq + i) * Tk + j] : 0.f; };
            for (int j = 0; j < Tk; ++j) if (d.allowed(b, i, j)) mx = fmaxf(mx, sc(j));
            int n = 0; long sabs[DH] = {0};
            for (int j = 0; j < Tk; ++j) if (d.allowed(b, i, j) && sc(j) == mx) {
                d.att[r * Tk + j] = 1; ++n;
                for (int e = 0; e < DH; ++e) { const int v = (int)d.V[((size_t)b * Tk + j) * DM + h * DH + e]; d.sum[r * DH + e] += v; sabs[e] += v < 0 ? -v : v; }
            }
            d.cnt[r] = n; if (n < 1) d.pre_ok = false;
            for (int e = 0; e < DH; ++e) { const size_t oi = ((size_t)b * Tq + i) * DM + h * DH + e; d.o[oi] = (double)d.sum[r * DH + e] / n; d.A[oi] = (double)sabs[e] / n; }
        }
    } else if (hot) {
        std::vector<unsigned char> wins((size_t)NB * NH * Tk, 0);
        const int cand[7] = {0, 15, 16, 31, 32, 33, Tk - 1};
        for (int b = 0; b < NB; ++b) for (int h = 0; h < NH; ++h) for (int i = 0; i < Tq; ++i) {
            const size_t r = d.row(b, h, i);
            const unsigned hh = hsh4(chk == CHK_HOTB ? 0 : b, h, i, 0, seed + 6u);
            int w = -1;
            if (chk == CHK_HOTB) {      // the bias has no batch axis: a ladder -128 ((j - w0) mod Tk) makes the first allowed key at or after w0(h, i) win in every batch row
                const int w0 = std::min(cand[hh % 7u], Tk - 1);
                for (int t = 0; t < Tk && w < 0; ++t) if (d.allowed(b, i, (w0 + t) % Tk)) w = (w0 + t) % Tk;
                for (int j = 0; j < Tk; ++j) d.bias[((size_t)h * Tq + i) * Tk + j] = -128.f * (float)((j - w0 + Tk) % Tk);
            } else {
                for (int t = 0; t < 7 && w < 0; ++t) { const int c = cand[(hh + t) % 7u]; if (c >= 0 && c < Tk && d.allowed(b, i, c)) w = c; }
                if (w < 0) for (int j = Tk - 1; j >= 0 && w < 0; --j) if (d.allowed(b, i, j)) w = j;       // causal: the diagonal
            }
            if (w < 0) { d.pre_ok = false; w = 0; }
            d.win[r] = w; d.cnt[r] = 1; d.att[r * Tk + w] = 1; wins[((size_t)b * NH + h) * Tk + w] = 1;
            float* q = &d.Q[((size_t)b * Tq + i) * DM + h * DH];
            if (chk == CHK_HOT) { q[rot(w % 17, h)] = 65536.f; q[rot(17 + w / 17, h)] = 65536.f; if (kind != 2) q[rot(63, h)] = 1024.f; }
            if (kind == 2 && chk == CHK_HOT) for (int j = 0; j < Tk; ++j) d.bias[((size_t)h * Tq + i) * Tk + j] = (hsh4(h, i, j, 1, seed + 7u) & 1u) ? -128.f : 0.f;
        }
        for (int b = 0; b < NB; ++b) for (int j = 0; j < Tk; ++j) for (int h = 0; h < NH; ++h) {
            float* v = &d.V[((size_t)b * Tk + j) * DM + h * DH];
            const bool key_ok = kind == 0 || d.mask[(size_t)b * Tk + j];
            for (int e = 0; e < DH; ++e) {
                const unsigned x = hsh4(b, j, h, e, seed + 8u);
                if (wins[((size_t)b * NH + h) * Tk + j]) v[e] = rbf(unit(x) * 4.f);
                else v[e] = ((x & 1u) ? -1.f : 1.f) * ((chk == CHK_HOT && kind == 2 && key_ok) ? 1.2676506e30f /* 2^100 */ : rbf(3e38f));
            }
        }
        // precondition: the winner leads every other allowed key by >= 128 after scaling, and (no bias) any two allowed keys are >= 128 apart
        for (int b = 0; b < NB && d.pre_ok; ++b) for (int h = 0; h < NH; ++h) for (int i = 0; i < Tq; ++i) {
            const int w = d.win[d.row(b, h, i)];
            const float* q = &d.Q[((size_t)b * Tq + i) * DM + h * DH];
            auto score = [&](int j) {
                double s = 0; const float* k = &d.K[((size_t)b * Tk + j) * DM + h * DH];
                for (int e = 0; e < DH; ++e) s += (double)q[e] * k[e];
                float x = (float)s * d.scale; if ((double)x != s * d.scale) d.pre_ok = false;
                if (kind == 2) x = rbf(rbf(x) + d.bias[((size_t)h * Tq + i) * Tk + j]);
                return x;
            };
            if (!d.allowed(b, i, w)) d.pre_ok = false;
            const float sw = score(w); std::vector<float> all;
            for (int j = 0; j < Tk; ++j) if (j != w && d.allowed(b, i, j)) {
                const float s = score(j); all.push_back(s);
                if (!(sw - s >= 128.f)) d.pre_ok = false;
            }
            if (kind != 2 || chk == CHK_HOTB) { std::sort(all.begin(), all.end()); for (size_t t = 1; t < all.size(); ++t) if (!(all[t] - all[t - 1] >= 128.f)) d.pre_ok = false; }
        }
    } else {      // dense
        for (size_t i = 0; i < d.Q.size(); ++i) d.Q[i] = (float)((int)(hsh((unsigned)i, 9u, seed + 9u) % 7u) - 3);
        for (size_t i = 0; i < d.V.size(); ++i) d.V[i] = rbf(unit(hsh((unsigned)i, 10u, seed + 10u)));
        for (size_t i = 0; i < d.bias.size(); ++i) d.bias[i] = rbf(2.f * unit(hsh((unsigned)i, 11u, seed + 11u)));
        d.o.assign((size_t)NB * Tq * DM, 0); d.A.assign(d.o.size(), 0); d.xs.assign(nrow * Tk, -INFINITY);
        std::vector<double> p(Tk); std::vector<float> xrow(Tk);
        if (kind == 2) { d.o32.assign(d.o.size(), 0); d.A32.assign(d.o.size(), 0); }
        for (int pass = 0; pass < (kind == 2 ? 2 : 1); ++pass)
        for (int b = 0; b < NB; ++b) for (int h = 0; h < NH; ++h) for (int i = 0; i < Tq; ++i) {
            std::vector<double>& O = pass ? d.o32 : d.o; std::vector<double>& AA = pass ? d.A32 : d.A;
            const float* q = &d.Q[((size_t)b * Tq + i) * DM + h * DH];
            float* xs = pass ? xrow.data() : &d.xs[d.row(b, h, i) * Tk];
            float mx = -INFINITY, mn = INFINITY;
            for (int j = 0; j < Tk; ++j) xs[j] = -INFINITY;
            for (int j = 0; j < Tk; ++j) if (d.allowed(b, i, j)) {
                const float* k = &d.K[((size_t)b * Tk + j) * DM + h * DH];
                int s = 0; for (int e = 0; e < DH; ++e) s += (int)q[e] * (int)k[e];
                float x = (float)s * d.scale;
                if ((double)x != (double)s * (double)d.scale) d.pre_ok = false;                 // exact in fp32 and fp64 alike
                if (kind == 2) { const float bz = d.bias[((size_t)h * Tq + i) * Tk + j]; x = d.none[b] ? 0.f : pass ? x + bz : rbf(rbf(x) + bz); }
                xs[j] = x; mx = fmaxf(mx, x); mn = fminf(mn, x);
            }
            if (!(mx > -INFINITY)) { d.pre_ok = false; continue; }
            if (!pass && mx - mn > d.X) d.X = mx - mn;
            double L = 0; for (int j = 0; j < Tk; ++j) { p[j] = xs[j] == -INFINITY ? 0.0 : std::exp((double)xs[j] - (double)mx); L += p[j]; }
            for (int e = 0; e < DH; ++e) {
                double a = 0, aa = 0;
                for (int j = 0; j < Tk; ++j) { const double v = d.V[((size_t)b * Tk + j) * DM + h * DH + e]; a += p[j] * v; aa += p[j] * std::fabs(v); }
                const size_t oi = ((size_t)b * Tq + i) * DM + h * DH + e; O[oi] = a / L; AA[oi] = aa / L;
            }
        }
    }
    if (!d.pre_ok) { printf("  FAIL PRECONDITION %s\n", d.name.c_str()); g_fail++; }
}

// ---------------------------------------------------------------------------------------------------------------- the derived bound (header, section 2)
struct Bound { double c1, c2, c3; };
static Bound bound_for(int form, int Tk, double X) {
    const double u = std::ldexp(1.0, -24), ub = std::ldexp(1.0, -8), n = Tk, nblk = (Tk + 31) / 32;
    Bound B; B.c3 = 1e-35;
    if (form == F_FUSED) {
        const double ee = (1.0 + X) * 2 * u, etaN = ub + nblk * ee + (nblk + n) * 2 * u, etaL = nblk * ee + (n + 10 + 2 * nblk) * u;
        B.c1 = 1.01 * etaN * (1 + ub); B.c2 = ub + 1.01 * (etaL + 3 * u) * (1 + ub);
    } else if (form == F_UNF16) { B.c1 = 1.01 * (1 + ub) * (ub + (3 * n + 7) * u); B.c2 = ub; }
    else { B.c1 = 1.01 * (3 * n + 7) * u; B.c2 = 0; }
    return B;
}
// worst error / bound over every element; `get(oi)` returns the value under test
template <typename G> static double worst_ratio(const Data& d, const Bound& B, G&& get, long* nbad, bool exact_mode = false) {
    double worst = 0; *nbad = 0;
    const std::vector<double>& O = exact_mode && !d.o32.empty() ? d.o32 : d.o; const std::vector<double>& AA = exact_mode && !d.o32.empty() ? d.A32 : d.A;
    for (size_t oi = 0; oi < O.size(); ++oi) {
        const double got = get(oi), bnd = B.c1 * AA[oi] + B.c2 * std::fabs(O[oi]) + B.c3, e = std::fabs(got - O[oi]);
        if (!(e <= bnd)) { ++*nbad; worst = INFINITY; } else if (e / bnd > worst) worst = e / bnd;
    }
    return worst;
}
// the fused kernel's arithmetic on the host: 32-key blocks, running maximum, fp32 expf, bf16 probabilities, fp32 accumulators
static void emulate_fused(const Data& d, std::vector<float>& out) {
    out.assign(d.o.size(), 0.f);
    for (int b = 0; b < NB; ++b) for (int h = 0; h < NH; ++h) for (int i = 0; i < d.Tq; ++i) {
        const float* xs = &d.xs[d.row(b, h, i) * d.Tk];
        float m = -INFINITY, l = 0.f, acc[DH] = {0.f};
        for (int j0 = 0; j0 < d.Tk; j0 += 32) {
            const int j1 = std::min(j0 + 32, d.Tk);
            float mx = -INFINITY; for (int j = j0; j < j1; ++j) mx = fmaxf(mx, xs[j]);
            const float mn = fmaxf(m, mx), base = mn == -INFINITY ? 0.f : mn, alpha = expf(m - base);
            float ps = 0.f; for (int e = 0; e < DH; ++e) acc[e] *= alpha;
            for (int j = j0; j < j1; ++j) {
                const float p = expf(xs[j] - base); ps += p; const float pb = rbf(p);
                const float* v = &d.V[((size_t)b * d.Tk + j) * DM + h * DH];
                for (int e = 0; e < DH; ++e) acc[e] += pb * v[e];
            }
            l = l * alpha + ps; m = mn;
        }
        const float inv = l > 0.f ? 1.0f / l : 0.f;
        for (int e = 0; e < DH; ++e) out[((size_t)b * d.Tq + i) * DM + h * DH + e] = rbf(acc[e] * inv);
    }
}

// ---------------------------------------------------------------------------------------------------------------- one case on the GPU
static float ld_elem(const std::vector<unsigned char>& buf, size_t off, size_t i, int esz) {
    if (esz == 2) { bf16_t b; memcpy(&b, &buf[off + i * 2], 2); return bf2f(b); } float f; memcpy(&f, &buf[off + i * 4], 4); return f;
}
static bool same_bits(const std::vector<unsigned char>& buf, size_t off, size_t i, int esz, float v) {
    if (esz == 2) { const bf16_t b = f2bf(v); return !memcmp(&buf[off + i * 2], &b, 2); } return !memcmp(&buf[off + i * 4], &v, 4);
}
static void inv_candidates(int n, float c[3]) { c[1] = 1.0f / (float)n; c[0] = nextafterf(c[1], 0.f); c[2] = nextafterf(c[1], 2.f); }

// direct: car_launch_flash64 on a V^T built by car_launch_transpose_pad (the Tq != Tk cases); otherwise attn_run
static void run_case(const Data& d, int form, bool packed, bool direct) {
    static car_ctx ctx;
    const int esz = form == F_UNF32 ? 4 : 2, Tq = d.Tq, Tk = d.Tk, Tpad = (Tk + 31) / 32 * 32;
    const std::string name = d.name + "  " + form_name[form] + (direct ? "  direct" : packed ? "  ld 3D" : "  ld D ");
    ++g_cases;
    ctx.mode = form == F_UNF32 ? CAR_F32 : CAR_BF16; ctx.esz = (size_t)esz;
    AttnBytes ab = attn_bytes(&ctx, NB, Tk, NH, DH);
    if (direct) { ab.S = ab.P = 0; }
    if ((form == F_FUSED) != (ab.S == 0)) { fail(name, "CAR_NO_FLASH and the form disagree (attn_bytes.S = %zu)", ab.S); return; }
    Arena a;
    const long ld = packed ? 3 * DM : DM;
    size_t oq, ok_, ov;
    if (packed) { oq = a.take((size_t)NB * Tq * ld * esz); ok_ = oq + (size_t)DM * esz; ov = oq + (size_t)2 * DM * esz; }
    else { oq = a.take((size_t)NB * Tq * DM * esz); ok_ = a.take((size_t)NB * Tk * DM * esz); ov = a.take((size_t)NB * Tk * DM * esz); }
    const size_t om = d.kind ? a.take((size_t)NB * Tk) : 0, obz = d.kind == 2 ? a.take((size_t)NH * Tq * Tk * 4) : 0;
    const size_t oo = a.take((size_t)NB * Tq * DM * esz, true);
    a.top += (size_t)2 * DM * esz;                                                        // two rows behind out: not writable
    const size_t oS = a.take(ab.S, true), oP = a.take(ab.P, true), oVt = a.take(ab.Vt, true);
    a.finish();
    for (int b = 0; b < NB; ++b) {
        for (int t = 0; t < Tq; ++t) for (int c = 0; c < DM; ++c) a.put(oq, ((size_t)b * Tq + t) * ld + c, esz, d.Q[((size_t)b * Tq + t) * DM + c]);
        for (int t = 0; t < Tk; ++t) for (int c = 0; c < DM; ++c) {
            a.put(ok_, ((size_t)b * Tk + t) * ld + c, esz, d.K[((size_t)b * Tk + t) * DM + c]);
            a.put(ov, ((size_t)b * Tk + t) * ld + c, esz, d.V[((size_t)b * Tk + t) * DM + c]);
        }
    }
    if (d.kind) memcpy(&a.pre[om], d.mask.data(), d.mask.size());
    if (d.kind == 2) memcpy(&a.pre[obz], d.bias.data(), d.bias.size() * 4);
    int rc = 0;
    const bool ran = run_twice(a, name, [&](unsigned char* dv) {
        const unsigned char* mk = d.kind ? dv + om : nullptr; const float* bz = d.kind == 2 ? (const float*)(dv + obz) : nullptr;
        if (direct) {
            car_launch_transpose_pad(CAR_BF16, dv + ov, ld, (long)Tk * ld, dv + oVt, NB, Tk, Tpad, DM, 0);
            FlashP f; memset(&f, 0, sizeof(f));
            f.q = (const bf16_t*)(dv + oq); f.k = (const bf16_t*)(dv + ok_); f.vt = (const bf16_t*)(dv + oVt); f.o = (bf16_t*)(dv + oo);
            f.q_sb = (long)Tq * ld; f.k_sb = (long)Tk * ld; f.q_st = f.k_st = ld; f.vt_sb = (long)DM * Tpad; f.vt_ld = Tpad; f.o_sb = (long)Tq * DM; f.o_st = DM;
            f.Tq = Tq; f.Tk = Tk; f.H = NH; f.scale = d.scale; f.mode = d.kind; f.mask = mk; f.bias = bz;
            rc |= car_launch_flash64(&f, NB, 0);
        } else {
            ctx.ws[4].p = dv + oS; ctx.ws[4].cap = ab.S; ctx.ws[5].p = dv + oP; ctx.ws[5].cap = ab.P; ctx.ws[6].p = dv + oVt; ctx.ws[6].cap = ab.Vt;
            AttnCall c; memset(&c, 0, sizeof(c));
            c.q = dv + oq; c.k = dv + ok_; c.v = dv + ov; c.ld = ld; c.out = dv + oo; c.nb = NB; c.T = Tq; c.H = NH; c.hd = DH; c.scale = d.scale;
            c.kind = d.kind; c.mask = mk; c.bias = bz; c.col0 = 0;
            rc |= attn_run(&ctx, c, 0);
        }
    });
    ctx.ws[4] = DevBuf(); ctx.ws[5] = DevBuf(); ctx.ws[6] = DevBuf();
    if (rc) { fail(name, "the launcher refused (%d)", rc); return; }
    if (!ran) return;
    const std::vector<unsigned char>& po = a.post;
    // ---- V^T: the bits of V, zero pad columns
    long bad = 0;
    for (int b = 0; b < NB; ++b) for (int c = 0; c < DM; ++c) for (int t = 0; t < Tpad; ++t)
        bad += !same_bits(po, oVt, ((size_t)b * DM + c) * Tpad + t, esz, t < Tk ? d.V[((size_t)b * Tk + t) * DM + c] : 0.f);
    if (bad) { fail(name, "%ld elements of V^T differ from V / its zero padding", bad); return; }
    const bool unf = form != F_FUSED, uni = d.chk == CHK_UNI || d.chk == CHK_UNIB, hot = d.chk == CHK_HOT || d.chk == CHK_HOTB;
    if (unf) {
        for (size_t r = 0; r < (size_t)NB * NH * Tq; ++r) for (int j = Tk; j < Tpad; ++j) bad += !same_bits(po, oP, r * Tpad + j, esz, 0.f);
        if (bad) { fail(name, "%ld pad columns of P are not zero", bad); return; }
    }
    double worst = -1; long nbad = 0;
    if (uni) {
        for (int b = 0; b < NB; ++b) for (int h = 0; h < NH; ++h) for (int i = 0; i < Tq; ++i) {
            const size_t r = d.row(b, h, i), o0 = ((size_t)b * Tq + i) * DM + h * DH;
            float cand[3]; inv_candidates(d.cnt[r], cand);
            bool rowok = false;
            for (int c = 0; c < 3 && !rowok; ++c) {
                bool okc = true;
                if (unf) for (int j = 0; j < Tk && okc; ++j) okc = same_bits(po, oP, r * Tpad + j, esz, d.att[r * Tk + j] ? cand[c] : 0.f);
                const float pinv = form == F_UNF16 ? rbf(cand[c]) : cand[c];
                if (form != F_UNF32) for (int e = 0; e < DH && okc; ++e) okc = same_bits(po, oo, o0 + e, 2, (float)d.sum[r * DH + e] * pinv);
                rowok = okc;
            }
            nbad += !rowok;
        }
        if (nbad) { fail(name, "%ld rows match none of the three candidate 1 / count (attended set or sum wrong)", nbad); return; }
    }
    if (hot) {
        for (int b = 0; b < NB; ++b) for (int h = 0; h < NH; ++h) for (int i = 0; i < Tq; ++i) {
            const size_t r = d.row(b, h, i), o0 = ((size_t)b * Tq + i) * DM + h * DH; const int w = d.win[r];
            bool okr = true;
            for (int e = 0; e < DH && okr; ++e) okr = same_bits(po, oo, o0 + e, esz, d.V[((size_t)b * Tk + w) * DM + h * DH + e]);
            if (unf) for (int j = 0; j < Tk && okr; ++j) okr = same_bits(po, oP, r * Tpad + j, esz, j == w ? 1.f : 0.f);
            nbad += !okr;
        }
        if (nbad) { fail(name, "%ld rows are not the bits of the winner's V row", nbad); return; }
    }
    if (d.chk == CHK_DENSE || (uni && form == F_UNF32)) {
        const Bound B = bound_for(form, Tk, d.X);
        worst = worst_ratio(d, B, [&](size_t oi) { return (double)ld_elem(po, oo, oi, esz); }, &nbad, form == F_UNF32);
        if (nbad) { fail(name, "%ld elements beyond the derived bound %.3g A + %.3g |o| + %.0e", nbad, B.c1, B.c2, B.c3); return; }
    }
    if (worst >= 0) printf("  ok   %s   worst error / bound %.3f\n", name.c_str(), worst); else printf("  ok   %s   exact\n", name.c_str());
}

// ---------------------------------------------------------------------------------------------------------------- refusals of car_launch_flash64 / attn_run
static FlashP good_flash(unsigned char* base, int kind, int Tq, int Tk) {
    FlashP f; memset(&f, 0, sizeof(f));
    const int Tpad = (Tk + 31) / 32 * 32;
    f.q = (const bf16_t*)(base + 4096); f.k = (const bf16_t*)(base + 4096 + 65536); f.vt = (const bf16_t*)(base + 4096 + 2 * 65536); f.o = (bf16_t*)(base + 4096 + 3 * 65536);
    f.q_sb = (long)Tq * DM; f.k_sb = (long)Tk * DM; f.q_st = f.k_st = DM; f.vt_sb = (long)DM * Tpad; f.vt_ld = Tpad; f.o_sb = (long)Tq * DM; f.o_st = DM;
    f.Tq = Tq; f.Tk = Tk; f.H = NH; f.scale = 0.125f; f.mode = kind; f.mask = base + 4096 + 4 * 65536; f.bias = (const float*)(base + 4096 + 4 * 65536 + 4096);
    return f;
}
static void refusals(unsigned char* base) {
    struct V { const char* what; void (*edit)(FlashP&); };
    const V vs[] = {
        {"q_st % 8", [](FlashP& f) { f.q_st += 4; }}, {"k_st % 8", [](FlashP& f) { f.k_st += 4; }}, {"q_sb % 8", [](FlashP& f) { f.q_sb += 4; }},
        {"k_sb % 8", [](FlashP& f) { f.k_sb += 4; }}, {"vt_sb % 8", [](FlashP& f) { f.vt_sb += 4; }}, {"o_st % 4", [](FlashP& f) { f.o_st += 2; }},
        {"o_sb % 4", [](FlashP& f) { f.o_sb += 2; }}, {"vt_ld % 32", [](FlashP& f) { f.vt_ld += 16; }}, {"vt_ld < rup(Tk, 32)", [](FlashP& f) { f.vt_ld -= 32; }},
        {"q misaligned", [](FlashP& f) { f.q += 4; }}, {"k misaligned", [](FlashP& f) { f.k += 4; }}, {"vt misaligned", [](FlashP& f) { f.vt += 4; }},
        {"o misaligned", [](FlashP& f) { f.o += 2; }}, {"causal with Tq != Tk", [](FlashP& f) { f.mode = 1; }},
    };
    for (const V& v : vs) {
        FlashP f = good_flash(base, 0, 40, 70); v.edit(f); ++g_cases;
        const int rc = car_launch_flash64(&f, NB, 0);
        if (rc != -1) fail(std::string("refusal ") + v.what, "returned %d, not -1", rc); else printf("  ok   refusal: %s\n", v.what);
    }
}
static void refusals_gpu() {
    Arena a; const size_t o = a.take(8 * 65536); a.finish();
    run_twice(a, "refusals of car_launch_flash64", [&](unsigned char* dv) { refusals(dv + o); });
    if (a.post.size() && memcmp(a.post.data(), a.pre.data(), a.top)) fail("refusals of car_launch_flash64", "a refused call wrote");
    // attn_run: ld = D + 4 breaks q_st % 8; V^T is built first, then the refusal must come back and out stay untouched
    static car_ctx ctx; ctx.mode = CAR_BF16; ctx.esz = 2;
    const int T = 33, Tpad = 64; const long ld = DM + 4;
    Arena b; const size_t oq = b.take((size_t)NB * T * ld * 2), okk = b.take((size_t)NB * T * ld * 2), ov = b.take((size_t)NB * T * ld * 2);
    const size_t oo = b.take((size_t)NB * T * DM * 2), oVt = b.take((size_t)NB * DM * Tpad * 2, true);
    b.finish(); ++g_cases;
    for (size_t i = 0; i < (size_t)NB * T * ld; ++i) b.put(ov, i, 2, (float)((int)(i % 7) - 3));
    int rc = 0;
    const bool ran = run_twice(b, "attn_run refusal", [&](unsigned char* dv) {
        ctx.ws[6].p = dv + oVt; ctx.ws[6].cap = (size_t)NB * DM * Tpad * 2;
        AttnCall c; memset(&c, 0, sizeof(c));
        c.q = dv + oq; c.k = dv + okk; c.v = dv + ov; c.ld = ld; c.out = dv + oo; c.nb = NB; c.T = T; c.H = NH; c.hd = DH; c.scale = 0.125f; c.kind = ATTN_NONE;
        rc = attn_run(&ctx, c, 0);
    });
    ctx.ws[6] = DevBuf();
    if (ran && rc == 0) fail("attn_run refusal", "attn_run returned 0 for a token stride of D + 4");
    else if (ran) printf("  ok   attn_run passes the refusal on (%d), out untouched\n", rc);
}

// ---------------------------------------------------------------------------------------------------------------- the row-softmax launchers
struct SmCase { int mode, rows, ncols, mm, Tq, col0; long lds, ldp; };
static float sm_score(unsigned r, unsigned j, unsigned seed) { return 8.f * unit(hsh(r, j, seed)); }
static std::vector<unsigned char> sm_mask(int T, int c, unsigned seed) {
    std::vector<unsigned char> m(T); for (int j = 0; j < T; ++j) m[j] = j >= c && hsh((unsigned)j, 13u, seed) % 8u != 0; return m;
}
// P of car_launch_softmax_at (kernel 0) or of one kernel launched directly (1: softmax_reg_kernel at col0, 2: softmax_kernel); S[r][j] = score(r + r0, j + c0)
static bool sm_run(const std::string& name, const SmCase& c, int which, const std::vector<unsigned char>& mask, int moff, int r0, int c0, unsigned seed,
                   std::vector<unsigned char>& P) {
    const int esz = c.mode == 1 ? 2 : 4;
    Arena a; const size_t oS = a.take((size_t)c.rows * c.lds * 4), om = a.take(mask.size() + 1), oP = a.take((size_t)c.rows * c.ldp * esz, true);
    a.finish(); ++g_cases;
    for (int r = 0; r < c.rows; ++r) for (int j = 0; j < c.ncols; ++j) a.put(oS, (size_t)r * c.lds + j, 4, sm_score((unsigned)(r + r0), (unsigned)(j + c0), seed));
    if (!mask.empty()) memcpy(&a.pre[om], mask.data(), mask.size());
    const bool ran = run_twice(a, name, [&](unsigned char* dv) {
        const float* S = (const float*)(dv + oS); void* Pd = dv + oP; const unsigned char* mk = c.mm ? dv + om + moff : nullptr;
        if (which == 0) car_launch_softmax_at(c.mode, S, c.lds, Pd, c.ldp, c.rows, c.ncols, c.mm, mk, c.Tq, 1, c.col0, 0);
        else if (which == 1) { LAUNCH_T(c.mode, softmax_reg_kernel, dim3(c.rows), dim3(256), 0, S, c.lds, Pd, c.ldp, c.ncols, c.mm, mk, c.Tq, 1, c.col0); }
        else { LAUNCH_T(c.mode, softmax_kernel, dim3(c.rows), dim3(256), 0, S, c.lds, Pd, c.ldp, c.ncols, c.mm, mk, c.Tq, 1); }
    });
    if (!ran) return false;
    P.assign(a.post.begin() + oP, a.post.begin() + oP + (size_t)c.rows * c.ldp * esz);
    return true;
}
// against the fp64 softmax: |p - p*| <= ((n + 7) u [+ ub]) 1.01 p* + 1e-37  (expf one ulp, n-term sum, inv one ulp, one multiply[, one bf16 rounding]); masked and pad columns exactly 0
static void sm_against_fp64(const std::string& name, const SmCase& c, const std::vector<unsigned char>& mask, unsigned seed, const std::vector<unsigned char>& P) {
    const int esz = c.mode == 1 ? 2 : 4; long nbad = 0; double worst = 0;
    const double eta = 1.01 * ((c.ncols + 7) * std::ldexp(1.0, -24) + (c.mode == 1 ? std::ldexp(1.0, -8) : 0.0));
    std::vector<double> p(c.ncols);
    for (int r = 0; r < c.rows; ++r) {
        const int i = c.mm ? r % c.Tq : 0; double mx = -INFINITY, L = 0;
        auto ok = [&](int j) { return !c.mm || (j <= i && (mask[j] || j == i)); };
        for (int j = 0; j < c.ncols; ++j) if (ok(j)) mx = std::max(mx, (double)sm_score((unsigned)r, (unsigned)j, seed));
        for (int j = 0; j < c.ncols; ++j) { p[j] = ok(j) ? std::exp((double)sm_score((unsigned)r, (unsigned)j, seed) - mx) : 0.0; L += p[j]; }
        for (int j = 0; j < c.ldp; ++j) {
            const double want = j < c.ncols ? p[j] / L : 0.0, got = ld_elem(P, 0, (size_t)r * c.ldp + j, esz), e = std::fabs(got - want), bnd = want == 0 ? 0 : eta * want + 1e-37;
            if (!(e <= bnd)) ++nbad; else if (bnd > 0 && e / bnd > worst) worst = e / bnd;
        }
    }
    if (nbad) fail(name, "%ld probabilities beyond the bound (or a masked / pad column not zero)", nbad); else printf("  ok   %s   worst error / bound %.3f\n", name.c_str(), worst);
}
static void softmax_section() {
    char nm[128];
    for (int mode = 1; mode >= 0; --mode) {
        const char* ms = mode ? "bf16" : "fp32";
        // A. the launcher's three routes on five rows against fp64; causal on the full square where it is small
        const int ncs[] = {1, 33, 64, 65, 127, 128, 129, 1025, 2016, 2050};
        for (int nc : ncs) {
            SmCase c{mode, 5, nc, 0, 0, nc <= 128 ? 0 : -1, nc + 3, (nc + 31) / 32 * 32};
            snprintf(nm, sizeof(nm), "softmax launcher   ncols %4d %s plain (%s)", nc, ms, nc <= 128 ? "wave" : nc <= 2048 ? "register" : "three-pass");
            std::vector<unsigned char> P, none;
            if (sm_run(nm, c, 0, none, 0, 0, 0, 77u + nc, P)) sm_against_fp64(nm, c, none, 77u + nc, P);
            if (nc > 129) continue;
            SmCase cc{mode, nc, nc, 1, nc, nc <= 128 ? 0 : -1, nc, (nc + 31) / 32 * 32};
            snprintf(nm, sizeof(nm), "softmax launcher   ncols %4d %s causal + holes", nc, ms);
            const std::vector<unsigned char> mk = sm_mask(nc, 0, 5u + nc);
            if (sm_run(nm, cc, 0, mk, 0, 0, 0, 78u + nc, P)) sm_against_fp64(nm, cc, mk, 78u + nc, P);
        }
        // B. softmax_reg_kernel at col0 = 0 == softmax_kernel, bit for bit
        for (int nc : {129, 1025, 2016}) for (int mm = 0; mm < 2; ++mm) {
            SmCase c{mode, mm ? nc : 5, nc, mm, nc, 0, nc, (nc + 31) / 32 * 32};
            snprintf(nm, sizeof(nm), "softmax_reg_kernel == softmax_kernel   ncols %4d %s %s", nc, ms, mm ? "causal + holes" : "plain");
            const std::vector<unsigned char> mk = mm ? sm_mask(nc, 0, 9u + nc) : std::vector<unsigned char>();
            std::vector<unsigned char> P1, P2;
            if (!sm_run(nm, c, 1, mk, 0, 0, 0, 90u + nc, P1) || !sm_run(nm, c, 2, mk, 0, 0, 0, 90u + nc, P2)) continue;
            if (P1 != P2) { printf("  BITS DIFFER %s\n", nm); g_fail++; } else printf("  ok   %s   equal bits\n", nm);
        }
        // C. window invariance: the full prefix with c masked columns in front == the window starting at c
        for (int Tf : {100, 128, 200, 2048}) for (int cw : {5, 16, 48}) {
            const int Tw = Tf - cw, esz = mode ? 2 : 4; const long ldpf = (Tf + 31) / 32 * 32;
            snprintf(nm, sizeof(nm), "softmax window invariance   prefix %4d window from %2d %s (%s)", Tf, cw, ms, Tf <= 128 ? "wave" : "register");
            const std::vector<unsigned char> mk = sm_mask(Tf, cw, 21u + Tf);
            SmCase full{mode, Tf, Tf, 1, Tf, 0, Tf, ldpf}, win{mode, Tw, Tw, 1, Tw, cw, Tw, Tw};
            std::vector<unsigned char> Pf, Pw;
            if (!sm_run(nm, full, 0, mk, 0, 0, 0, 300u + Tf, Pf) || !sm_run(nm, win, 0, mk, cw, cw, cw, 300u + Tf, Pw)) continue;
            long bad = 0;
            for (int r = 0; r < Tw; ++r) bad += memcmp(&Pw[(size_t)r * Tw * esz], &Pf[((size_t)(r + cw) * ldpf + cw) * esz], (size_t)Tw * esz) != 0;
            if (bad) { printf("  BITS DIFFER %s: %ld rows\n", nm, bad); g_fail++; } else printf("  ok   %s   equal bits\n", nm);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- timing (the old cases of this file)
static void time_case(const char* name, int B, int H, int T, int mode, float scale, bool packed3) {
    const int D = H * 64, Tpad = (T + 31) / 32 * 32; const long ld = packed3 ? 3 * D : D;
    std::vector<bf16_t> q((size_t)B * T * ld), vt((size_t)B * D * Tpad, 0);
    for (size_t i = 0; i < q.size(); ++i) q[i] = f2bf(1.5f * unit(hsh((unsigned)i, 1u, 1u)));
    for (size_t i = 0; i < vt.size(); ++i) vt[i] = (int)(i % Tpad) < T ? f2bf(unit(hsh((unsigned)i, 2u, 2u))) : 0;
    std::vector<unsigned char> mask((size_t)B * T, 1);
    if (mode) for (int b = 0; b < B; ++b) { const int nv = 1 + (b * 37 + 11) % T; for (int t = 0; t < T; ++t) mask[(size_t)b * T + t] = mode == 1 ? (t >= T - nv) : (t < nv); }
    std::vector<float> bias; if (mode == 2) { bias.resize((size_t)H * T * T); for (size_t i = 0; i < bias.size(); ++i) bias[i] = rbf(2.f * unit(hsh((unsigned)i, 3u, 3u))); }
    bf16_t *dq, *dk, *dvt, *dout; unsigned char* dmask; float* dbias = nullptr;
    CK(hipMalloc(&dq, q.size() * 2)); CK(hipMemcpy(dq, q.data(), q.size() * 2, hipMemcpyHostToDevice));
    dk = dq + D; if (!packed3) { CK(hipMalloc(&dk, q.size() * 2)); CK(hipMemcpy(dk, q.data(), q.size() * 2, hipMemcpyHostToDevice)); }
    CK(hipMalloc(&dvt, vt.size() * 2)); CK(hipMemcpy(dvt, vt.data(), vt.size() * 2, hipMemcpyHostToDevice));
    CK(hipMalloc(&dout, (size_t)B * T * D * 2)); CK(hipMalloc(&dmask, mask.size())); CK(hipMemcpy(dmask, mask.data(), mask.size(), hipMemcpyHostToDevice));
    if (mode == 2) { CK(hipMalloc(&dbias, bias.size() * 4)); CK(hipMemcpy(dbias, bias.data(), bias.size() * 4, hipMemcpyHostToDevice)); }
    FlashP p{}; p.q = dq; p.k = dk; p.vt = dvt; p.o = dout; p.q_sb = (long)T * ld; p.q_st = ld; p.k_sb = (long)T * ld; p.k_st = ld;
    p.vt_sb = (long)D * Tpad; p.vt_ld = Tpad; p.o_sb = (long)T * D; p.o_st = D; p.Tq = T; p.Tk = T; p.H = H; p.scale = scale; p.mode = mode; p.mask = dmask; p.bias = dbias;
    if (car_launch_flash64(&p, B, 0) != 0) { printf("%s: launcher refused\n", name); g_fail++; return; }
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) car_launch_flash64(&p, B, 0);
    CK(hipEventRecord(e0, 0));
    const int n = 20; for (int i = 0; i < n; ++i) car_launch_flash64(&p, B, 0);
    CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1)); ms /= n;
    printf("%-44s B %3d H %2d T %4d   %.3f ms  %.1f TFLOP/s\n", name, B, H, T, ms, 4.0 * B * H * (double)T * T * 64 * (mode == 1 ? 0.5 : 1.0) / ms / 1e9);
    CK(hipFree(dq)); if (!packed3) CK(hipFree(dk)); CK(hipFree(dvt)); CK(hipFree(dout)); CK(hipFree(dmask)); if (dbias) CK(hipFree(dbias));
}

// ---------------------------------------------------------------------------------------------------------------- main
int main(int argc, char** argv) {
    const std::string arg = argc > 1 ? argv[1] : "quick";
    if (arg == "time") {
        time_case("time: vit 1025 x 256 img x 6 heads", 256, 6, 1025, 0, 0.125f, false);
        time_case("time: vit-base 1025 x 64 img x 12 heads", 64, 12, 1025, 0, 0.125f, false);
        time_case("time: prefill 120 x 512 rows x 20 heads", 512, 20, 120, 1, 0.125f, true);
        time_case("time: t5 120 x 256 x 32 heads", 256, 32, 120, 2, 1.0f, false);
        return g_fail ? 1 : 0;
    }
    if (arg != "quick" && arg != "selftest") { printf("usage: attn_check [quick | selftest | time]\n"); return 2; }
    g_host_only = arg == "selftest";
    const bool noflash = getenv("CAR_NO_FLASH") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    printf("attn_check %s%s\n", arg.c_str(), noflash ? "  (CAR_NO_FLASH: the bf16 unfused cases only)" : "");
    const int Ts[] = {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 120, 128, 129, 192, 193, 197, 257};
    int ti = 0;
    for (int T : Ts) {
        for (int kind = 0; kind < 3; ++kind) for (int chk = 0; chk < 5; ++chk) {
            if ((chk == CHK_UNIB || chk == CHK_HOTB) && kind != 2) continue;
            Data d; build(d, kind, chk, T, T, ti + kind);
            if (!d.pre_ok) continue;
            if (g_host_only) {
                ++g_cases;
                if (chk != CHK_DENSE) { printf("  ok   %s   preconditions\n", d.name.c_str()); continue; }
                std::vector<float> emu; emulate_fused(d, emu); long nbad = 0;
                const Bound B = bound_for(F_FUSED, T, d.X);
                const double w = worst_ratio(d, B, [&](size_t oi) { return (double)emu[oi]; }, &nbad);
                if (nbad) fail(d.name, "host emulation of the fused kernel: %ld elements beyond the derived bound", nbad);
                else printf("  ok   %s   host emulation of the fused kernel: worst error / bound %.3f (score range %.1f)\n", d.name.c_str(), w, d.X);
                continue;
            }
            for (int packed = 0; packed < 2; ++packed) {
                if (noflash) run_case(d, F_UNF16, packed, false);
                else { run_case(d, F_FUSED, packed, false); run_case(d, F_UNF32, packed, false); }
            }
        }
        ++ti;
    }
    if (!noflash) {
        // Tq != Tk (40 x 70), straight through car_launch_flash64, the two non-causal modes
        for (int kind : {0, 2}) for (int chk : {CHK_UNI, CHK_UNIB, CHK_HOT, CHK_HOTB, CHK_DENSE}) {
            if ((chk == CHK_UNIB || chk == CHK_HOTB) && kind != 2) continue;
            Data d; build(d, kind, chk, 40, 70, kind);
            if (!d.pre_ok) continue;
            if (!g_host_only) { run_case(d, F_FUSED, false, true); continue; }
            ++g_cases;
            if (chk == CHK_DENSE) {
                std::vector<float> emu; emulate_fused(d, emu); long nbad = 0;
                const double w = worst_ratio(d, bound_for(F_FUSED, 70, d.X), [&](size_t oi) { return (double)emu[oi]; }, &nbad);
                if (nbad) fail(d.name, "host emulation of the fused kernel: %ld elements beyond the derived bound", nbad);
                else printf("  ok   %s   host emulation of the fused kernel: worst error / bound %.3f\n", d.name.c_str(), w);
            }
        }
        if (g_host_only) { static unsigned char fake[16]; refusals((unsigned char*)(((uintptr_t)fake + 255) & ~(uintptr_t)255)); }
        else { refusals_gpu(); softmax_section(); }
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%d cases, %.1f s\n", g_cases, secs);
    if (g_fail) { printf("%d checks FAILED\n", g_fail); return 1; }
    printf("all checks passed\n");
    return 0;
}
