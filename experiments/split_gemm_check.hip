// experiments/split_gemm_check.hip — standalone check of gemm_f32s_kernel (controlar_amd/csrc/gemm_split.hip), launched through car_launch_gemm with
// GemmP::split3, on integer-valued operands whose split products and sums are exact in fp32: the expected output has NO tolerance (==).
//   data set a   A has at most 8 significant bits (its lo is zero), W has 9-16: the result needs the A-hi · W-lo cross term
//   data set b   the mirror image: needs A-lo · W-hi
//   data set c   both have 9 or more bits: the result is the three-term sum  hi·hi + hi·lo + lo·hi  — and differs from the exact product by the lo·lo left out
// The host checks for every output element that the absolute values of all its terms sum to less than 2^23, which makes every partial sum of every
// summation order, the epilogue's alpha / bias / residual included, exact in fp32; the widths of the operands are chosen per shape to stay below it.
// Shapes: the smallest that reach every edge of the 128 x 128 x 32 tile (plain with bias, residual and alpha; batched; three convolutions, one with the
// folded x2 upsample), and an ineligible call (Cin = 16) whose output must be bit-equal with and without the flag.  Test infrastructure.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I controlar_amd/csrc experiments/split_gemm_check.hip -o experiments/split_gemm_check && experiments/split_gemm_check
#include "../controlar_amd/csrc/gemm.hip"
#include "../controlar_amd/csrc/gemm_split.hip"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)

static int g_fail = 0;
static unsigned hsh(unsigned i, unsigned seed) { unsigned x = i * 2654435761u + seed * 0x9e3779b9u; x ^= x >> 15; x *= 2246822519u; x ^= x >> 13; x *= 3266489917u; x ^= x >> 16; return x; }
// an integer with exactly `bits` significant bits (top bit and lowest bit set), random sign
static float with_bits(int bits, unsigned h) { const int mag = (1 << (bits - 1)) | (int)((h >> 8) & ((1u << (bits - 1)) - 1u)) | 1; return (h & 1u) ? (float)-mag : (float)mag; }

struct Case {
    const char* name; int amode, nb, M, N, K;       // plain: nb batches of [M, K] x [N, K];  conv: nb images, M = nb * Ho * Wo
    int Ho, Wo, Cin, ups; bool bias, resid; float alpha;
};

// element (row, col) of an operand of data set `ds`: `small` = the at-most-8-bit side of a / b (1 entry in 16, |v| in {1, 2}); c: one entry per 32 on the A side
static float gen(char ds, bool is_a, int row, int col, int bmax, unsigned seed) {
    const unsigned h = hsh((unsigned)row * 8191u + (unsigned)col, seed);
    if (ds == 'c') {
        if (is_a && (col & 31) != ((7 * row) & 31)) return 0.f;
        return with_bits(9 + (int)((h >> 3) % (unsigned)(bmax - 8)), h);
    }
    const bool small = (ds == 'a') == is_a;
    if (!small) return with_bits(9 + (int)((h >> 3) & 7u), h);
    if (((col + 3 * row) & 15) != 0) return 0.f;
    const float v = (float)(1 + (int)((h >> 1) & 1u));
    return (h & 1u) ? -v : v;
}

static void run(const Case& cs, char ds) {
    const bool conv = cs.amode == AMODE_CONV3;
    const int Hin = conv ? cs.Ho >> cs.ups : 0, Win = conv ? cs.Wo >> cs.ups : 0;
    const size_t arows = conv ? (size_t)cs.nb * Hin * Win : (size_t)cs.nb * cs.M, acols = conv ? cs.Cin : cs.K;
    const int zb = conv ? 1 : cs.nb;                                  // GEMM batches
    const size_t nA = arows * acols, nW = (size_t)zb * cs.N * cs.K, nC = (size_t)zb * cs.M * cs.N, guard = 4096;
    // widest operands of data set c that keep K / 32 three-term products below 2^23
    int bmax = 9; while (bmax < 16 && (double)(cs.K / 32) * std::pow(2.0, 2 * (bmax + 1)) * 1.02 < 8388608.0) ++bmax;
    std::vector<float> hA(nA), hW(nW), hb(cs.N), hR(nC), hC(nC + guard);
    for (size_t r = 0; r < arows; ++r) for (size_t c = 0; c < acols; ++c) hA[r * acols + c] = gen(ds, true, (int)r, (int)c, bmax, 11u);
    for (size_t r = 0; r < (size_t)zb * cs.N; ++r) for (int k = 0; k < cs.K; ++k) hW[r * cs.K + k] = gen(ds, false, (int)r, k, bmax, 23u);
    for (int n = 0; n < cs.N; ++n) hb[n] = (float)((int)(hsh(n, 5u) % 129u) - 64);
    for (size_t i = 0; i < nC; ++i) hR[i] = (float)((int)(hsh((unsigned)i, 7u) % 129u) - 64);
    // host reference: the three-term integer sum of the split operands, and the exact product next to it
    std::vector<unsigned short> ahi(nA), alo(nA), whi(nW), wlo(nW);
    car_debug_split_bf16(hA.data(), (int64_t)nA, ahi.data(), alo.data());
    car_debug_split_bf16(hW.data(), (int64_t)nW, whi.data(), wlo.data());
    std::vector<double> ref(nC);
    double worst = 0; size_t lolo = 0; bool sides_ok = true;
    for (int z = 0; z < zb; ++z)
        for (int m = 0; m < cs.M; ++m) {
            std::vector<long> arow_of(cs.K / (int)acols, -1);         // for each tap (conv) or the single row (plain): the A row it reads, -1 = zero padding
            if (!conv) arow_of[0] = (long)z * cs.M + m;
            else {
                const int hw = cs.Ho * cs.Wo, b = m / hw, y = (m % hw) / cs.Wo, x = m % cs.Wo;
                for (int tap = 0; tap < 9; ++tap) {
                    const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
                    if (yy >= 0 && yy < cs.Ho && xx >= 0 && xx < cs.Wo) arow_of[tap] = ((long)b * Hin + (yy >> cs.ups)) * Win + (xx >> cs.ups);
                }
            }
            for (int n = 0; n < cs.N; ++n) {
                double s3 = 0, sx = 0, sabs = 0;
                for (int k = 0; k < cs.K; ++k) {
                    const long ar = arow_of[k / (int)acols];
                    if (ar < 0) continue;
                    const size_t ia = (size_t)ar * acols + k % (int)acols, iw = ((size_t)z * cs.N + n) * cs.K + k;
                    const double ah = bf2f(ahi[ia]), al = bf2f(alo[ia]), wh = bf2f(whi[iw]), wl = bf2f(wlo[iw]);
                    if (ah + al != (double)hA[ia] || wh + wl != (double)hW[iw]) sides_ok = false;       // at most 16 significant bits: hi + lo is the value
                    s3 += ah * wh + ah * wl + al * wh; sx += (double)hA[ia] * hW[iw];
                    sabs += std::fabs(ah * wh) + std::fabs(ah * wl) + std::fabs(al * wh);
                }
                if (sabs > worst) worst = sabs;
                if (s3 != sx) ++lolo;
                double v = s3 * cs.alpha;
                if (cs.bias) v += hb[n];
                const size_t ic = ((size_t)z * cs.M + m) * cs.N + n;
                if (cs.resid) v += hR[ic];
                ref[ic] = v;
            }
        }
    if (!sides_ok || worst >= 8388608.0 - 256.0) { printf("%-28s set %c: PRECONDITION FAIL (sum of |terms| %.0f, split exact %d)\n", cs.name, ds, worst, (int)sides_ok); ++g_fail; return; }
    if ((ds == 'c') != (lolo > 0)) { printf("%-28s set %c: PRECONDITION FAIL (%zu outputs where the three-term sum differs from the exact product)\n", cs.name, ds, lolo); ++g_fail; return; }
    float *dA, *dW, *db, *dR, *dC;
    CK(hipMalloc(&dA, nA * 4)); CK(hipMalloc(&dW, nW * 4)); CK(hipMalloc(&db, cs.N * 4)); CK(hipMalloc(&dR, nC * 4)); CK(hipMalloc(&dC, (nC + guard) * 4));
    CK(hipMemcpy(dA, hA.data(), nA * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dW, hW.data(), nW * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(db, hb.data(), cs.N * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dR, hR.data(), nC * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dC, 0xff, (nC + guard) * 4));
    GemmP p; memset(&p, 0, sizeof(p));
    p.A = dA; p.W = dW; p.C = dC; p.lda = conv ? 0 : cs.K; p.ldw = cs.K; p.ldc = cs.N; p.M = cs.M; p.N = cs.N; p.K = cs.K; p.alpha = cs.alpha; p.nb0 = zb; p.nb1 = 1;
    p.sA0 = (long)cs.M * cs.K; p.sW0 = (long)cs.N * cs.K; p.sC0 = (long)cs.M * cs.N; p.sR0 = p.sC0;
    if (cs.bias) { p.bias = db; p.bias_mode = BIAS_N; }
    if (cs.resid) { p.R = dR; p.ldr = cs.N; }
    if (conv) { p.Ho = cs.Ho; p.Wo = cs.Wo; p.Cin = cs.Cin; p.ups = cs.ups; }
    p.split3 = 1;
    if (!car_gemm_split_ok(cs.amode, &p)) { printf("%-28s set %c: FAIL (the predicate refuses an eligible call)\n", cs.name, ds); ++g_fail; return; }
    const int rc = car_launch_gemm(0, cs.amode, &p, 0);
    CK(hipDeviceSynchronize()); CK(hipGetLastError());
    CK(hipMemcpy(hC.data(), dC, (nC + guard) * 4, hipMemcpyDeviceToHost));
    size_t bad = 0, first = (size_t)-1, gbad = 0;
    for (size_t i = 0; i < nC; ++i) if (!((double)hC[i] == ref[i])) { if (!bad) first = i; ++bad; }
    for (size_t i = nC; i < nC + guard; ++i) { unsigned u; memcpy(&u, &hC[i], 4); if (u != 0xffffffffu) ++gbad; }
    const bool ok = rc == 0 && bad == 0 && gbad == 0;
    printf("%-28s set %c: M %d N %d K %d  sum|terms| <= %.0f  lo·lo matters on %zu outputs  mismatches %zu  written past the end %zu  %s\n", cs.name, ds, cs.M, cs.N, cs.K, worst, lolo, bad, gbad, ok ? "OK" : "FAIL");
    if (bad) printf("    first mismatch at element %zu: got %.1f expected %.1f\n", first, (double)hC[first], ref[first]);
    if (!ok) ++g_fail;
    CK(hipFree(dA)); CK(hipFree(dW)); CK(hipFree(db)); CK(hipFree(dR)); CK(hipFree(dC));
}

// Cin = 16: a chunk of 32 would straddle two taps, so the predicate must refuse and the flag must change nothing
static void run_ineligible() {
    const int B = 1, Ho = 6, Wo = 5, Cin = 16, Cout = 40, M = B * Ho * Wo, K = 9 * Cin;
    const size_t nA = (size_t)M * Cin, nW = (size_t)Cout * K, nC = (size_t)M * Cout;
    std::vector<float> hA(nA), hW(nW), h0(nC), h1(nC);
    for (size_t i = 0; i < nA; ++i) hA[i] = (float)((int)(hsh((unsigned)i, 31u) % 20001u) - 10000) / 8192.0f;
    for (size_t i = 0; i < nW; ++i) hW[i] = (float)((int)(hsh((unsigned)i, 37u) % 20001u) - 10000) / 65536.0f;
    float *dA, *dW, *dC;
    CK(hipMalloc(&dA, nA * 4)); CK(hipMalloc(&dW, nW * 4)); CK(hipMalloc(&dC, nC * 4));
    CK(hipMemcpy(dA, hA.data(), nA * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dW, hW.data(), nW * 4, hipMemcpyHostToDevice));
    GemmP p; memset(&p, 0, sizeof(p));
    p.A = dA; p.W = dW; p.C = dC; p.ldw = K; p.ldc = Cout; p.M = M; p.N = Cout; p.K = K; p.alpha = 1.f; p.nb0 = p.nb1 = 1; p.Ho = Ho; p.Wo = Wo; p.Cin = Cin;
    int rc = 0;
    for (int f = 0; f < 2; ++f) {
        p.split3 = f;
        CK(hipMemset(dC, 0xff, nC * 4));
        rc |= car_launch_gemm(0, AMODE_CONV3, &p, 0);
        CK(hipDeviceSynchronize()); CK(hipGetLastError());
        CK(hipMemcpy((f ? h1 : h0).data(), dC, nC * 4, hipMemcpyDeviceToHost));
    }
    p.split3 = 1;
    const bool refused = !car_gemm_split_ok(AMODE_CONV3, &p), same = memcmp(h0.data(), h1.data(), nC * 4) == 0;
    bool finite = true; for (size_t i = 0; i < nC; ++i) if (!(std::fabs(h0[i]) < 1e30f)) finite = false;
    const bool ok = rc == 0 && refused && same && finite;
    printf("%-28s Cin %d: predicate refuses %d  bits equal with and without the flag %d  %s\n", "ineligible conv", Cin, (int)refused, (int)same, ok ? "OK" : "FAIL");
    if (!ok) ++g_fail;
    CK(hipFree(dA)); CK(hipFree(dW)); CK(hipFree(dC));
}

int main() {
    const Case cases[] = {
        { "plain bias+resid+alpha",  AMODE_PLAIN, 1, 130, 136,  96,  0,  0,  0, 0, true,  true,  0.5f },
        { "plain batched nb0=2",     AMODE_PLAIN, 2,  48,  48,  64,  0,  0,  0, 0, false, false, 1.0f },
        { "conv 2x5x7 32->96 resid", AMODE_CONV3, 2,  70,  96, 288,  5,  7, 32, 0, true,  true,  1.0f },
        { "conv 12x11 64->160",      AMODE_CONV3, 1, 132, 160, 576, 12, 11, 64, 0, true,  false, 1.0f },
        { "conv ups 4x6->8x12 32->128", AMODE_CONV3, 1, 96, 128, 288,  8, 12, 32, 1, true,  false, 1.0f },
    };
    for (const Case& cs : cases)
        for (char ds : { 'a', 'b', 'c' }) run(cs, ds);
    run_ineligible();
    if (g_fail) { printf("%d check(s) FAILED\n", g_fail); return 1; }
    printf("all checks passed\n");
    return 0;
}
