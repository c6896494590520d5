// engine_fid.hip — the statistics half of evaluations/c2i/evaluator.py as chains of fid.hip launches: car_fid_accumulate / car_fid_finalize
// (compute_statistics, :186-189), car_manifold_radii / car_manifold_pr (ManifoldEstimator.manifold_radii, :260-293, and evaluate_pr, :337-371, over
// DistanceBlock, :374-442), car_inception_score (:191-204 with the softmax of _create_softmax_graph, :615-626) and car_debug_pairwise_distances.
// No weights, any context of either mode.  (one of the translation units behind include/controlar_hip.h; shared declarations: engine_internal.h)
#include "engine_internal.h"
#include "fid_params.h"

extern "C" {
int car_launch_fid_prep(const float* x, long N, int D, int Kp, void* h16, void* nu16, float* nu32, hipStream_t st);
int car_launch_fid_tile(int arith, int epi, const FidTileP* p, hipStream_t st);
int car_launch_fid_radii_fold(const float* lists, long N, int ncb, int k, float* radii, hipStream_t st);
int car_launch_fid_pr_fold(const unsigned char* s1part, long N1, long parts1, const unsigned char* s2part, long N2, long parts2, unsigned char* status1,
                           unsigned char* status2, double* pr, hipStream_t st);
int car_launch_fid_accumulate(const float* x, long n, int D, double* state, hipStream_t st);
int car_launch_fid_finalize(const double* state, int D, double* mu, double* sigma, hipStream_t st);
int car_launch_is_transpose(const float* w, int D, int C, float* wt, hipStream_t st);
int car_launch_is_score(float* z, long N, int C, long split, int splits, int chunks, double* logm, double* part, double* out, hipStream_t st);
}

#define FDCHK(ctx, x) do { const int _e = (x); if (_e != 0) FAIL(ctx, "%s: %s failed: %s (%s:%d)", kWho, #x, hipGetErrorString((hipError_t)_e), __FILE__, __LINE__); } while (0)

static const int kMaxD = 16384;                        // a moment state of D = 16384 is 2 GiB
static const size_t kMaxPart = (size_t)4 << 30;        // bytes the per-batch lists / status parts of one call may take

// a bump allocator over the context's workspace: sizes first (p == nullptr), then pointers
struct FidCarve {
    char* p; size_t off = 0;
    explicit FidCarve(void* base) : p((char*)base) {}
    template <typename T> T* take(size_t n) { T* r = p ? (T*)(p + off) : nullptr; off += rup(n * sizeof(T), 256); return r; }
};

// one feature set in the workspace: the fp16 copy and both norm vectors
struct FidSet { void* h16; void* nu16; float* nu32; };
static FidSet carve_set(FidCarve& cv, long N, int Kp) {
    FidSet s;
    s.h16 = cv.take<uint16_t>((size_t)N * Kp); s.nu16 = cv.take<uint16_t>((size_t)N); s.nu32 = cv.take<float>((size_t)N);
    return s;
}

struct FidGrid { long rbz, cbz; int nrb, ncb, rt_per_rb; double wgs; };
static FidGrid fid_grid(long N1, long N2, long row_batch, long col_batch) {
    FidGrid g;
    g.rbz = std::min<long>(row_batch, N1); g.cbz = std::min<long>(col_batch, N2);       // a batch larger than the set is the whole set
    g.nrb = (int)std::min<long>((N1 + g.rbz - 1) / g.rbz, 1L << 30); g.ncb = (int)std::min<long>((N2 + g.cbz - 1) / g.cbz, 1L << 30);
    g.rt_per_rb = (int)((g.rbz + FID_TM - 1) / FID_TM);
    g.wgs = (double)g.rt_per_rb * g.nrb * g.ncb;
    return g;
}
static void fill_tile(FidTileP& p, int arith, const float* U, const FidSet& su, long N1, const float* V, const FidSet& sv, long N2, int D, int Kp, const FidGrid& g) {
    p.N1 = N1; p.N2 = N2; p.D = D; p.Kp = Kp; p.row_batch = g.rbz; p.col_batch = g.cbz; p.rt_per_rb = g.rt_per_rb; p.nrb = g.nrb; p.ncb = g.ncb;
    if (arith == FID_F16) { p.U = su.h16; p.V = sv.h16; p.ldu = p.ldv = Kp; p.nu = su.nu16; p.nv = sv.nu16; }
    else { p.U = U; p.V = V; p.ldu = p.ldv = D; p.nu = su.nu32; p.nv = sv.nu32; }
}

static int fid_common_checks(car_ctx* c, const char* kWho, int64_t N1, int64_t N2, int32_t D, int64_t row_batch, int64_t col_batch) {
    if (N1 < 1 || N2 < 1 || N1 > 2147483647L || N2 > 2147483647L) FAIL(c, "%s: a set holds 1 .. 2^31 - 1 rows (got %lld and %lld)", kWho, (long long)N1, (long long)N2);
    if (D < 1 || D > (1 << 20)) FAIL(c, "%s: D must be in 1 .. 2^20 (got %d)", kWho, D);
    if (row_batch < 1 || col_batch < 1) FAIL(c, "%s: row_batch and col_batch must be positive (got %lld and %lld)", kWho, (long long)row_batch, (long long)col_batch);
    return 0;
}

extern "C" int64_t car_fid_state_bytes(int32_t D) { return D < 1 || D > kMaxD ? 0 : (int64_t)sizeof(double) * (1 + 2 * (int64_t)D + (int64_t)D * D); }

extern "C" int car_fid_accumulate(car_ctx* c, const float* acts, int64_t n, int32_t D, void* state, void* stream_) {
    static const char* kWho = "car_fid_accumulate";
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!acts || !state) FAIL(c, "%s: acts and state must not be NULL", kWho);
    if (D < 1 || D > kMaxD) FAIL(c, "%s: D must be in 1 .. %d (got %d)", kWho, kMaxD, D);
    if (n < 1 || n > 2147483647L) FAIL(c, "%s: a batch holds 1 .. 2^31 - 1 rows (got %lld)", kWho, (long long)n);
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    FDCHK(c, car_launch_fid_accumulate(acts, (long)n, D, (double*)state, st));
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// Returns to the host whether the state can be finalised, so it waits for the stream: once per evaluation.
extern "C" int car_fid_finalize(car_ctx* c, const void* state, int32_t D, double* mu, double* sigma, void* stream_) {
    static const char* kWho = "car_fid_finalize";
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!state || !mu || !sigma) FAIL(c, "%s: state, mu and sigma must not be NULL", kWho);
    if (D < 1 || D > kMaxD) FAIL(c, "%s: D must be in 1 .. %d (got %d)", kWho, kMaxD, D);
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    double n = 0.0;
    HIPCHK(c, hipMemcpyAsync(&n, state, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (!(n >= 2.0)) { fence_out(c, caller); FAIL(c, "%s: the state holds %.0f rows; the covariance (ddof = 1) needs at least 2", kWho, n); }
    FDCHK(c, car_launch_fid_finalize((const double*)state, D, mu, sigma, st));
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int car_manifold_radii(car_ctx* c, const float* feats, int64_t N, int32_t D, int32_t k, int64_t row_batch, int64_t col_batch, float* radii, void* stream_) {
    static const char* kWho = "car_manifold_radii";
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!feats || !radii) FAIL(c, "%s: feats and radii must not be NULL", kWho);
    if (fid_common_checks(c, kWho, N, N, D, row_batch, col_batch)) return -1;
    if (k < 0 || k + 1 > FID_KMAX) FAIL(c, "%s: k must be in 0 .. %d (got %d)", kWho, FID_KMAX - 1, k);
    if ((int64_t)k + 1 > N) FAIL(c, "%s: the (k+1)-th smallest of N distances needs k + 1 <= N (got k %d, N %lld)", kWho, k, (long long)N);
    const int Kp = (int)rup((size_t)D, FID_KC);
    const FidGrid g = fid_grid(N, N, row_batch, col_batch);
    const size_t list_bytes = (size_t)g.ncb * (size_t)N * FID_KMAX * sizeof(float);
    if (g.wgs > 2147483647.0 || (double)g.ncb * (double)N * FID_KMAX * sizeof(float) > (double)kMaxPart)
        FAIL(c, "%s: %d x %d blocks of (%lld, %lld) are too many for N %lld: raise row_batch / col_batch", kWho, g.nrb, g.ncb, (long long)row_batch, (long long)col_batch, (long long)N);
    FidCarve sz(nullptr);
    carve_set(sz, N, Kp); sz.take<int>((size_t)g.nrb * g.ncb); sz.take<char>(list_bytes);
    NEED(c, c->fid_ws, sz.off);
    FidCarve cv(c->fid_ws.p);
    const FidSet s = carve_set(cv, N, Kp);
    int* flags = cv.take<int>((size_t)g.nrb * g.ncb);
    float* lists = (float*)cv.take<char>(list_bytes);
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    FDCHK(c, car_launch_fid_prep(feats, (long)N, D, Kp, s.h16, s.nu16, s.nu32, st));
    HIPCHK(c, hipMemsetAsync(flags, 0, (size_t)g.nrb * g.ncb * sizeof(int), st));
    // the fp16 pass raises the flag of every block with a distance that is not finite; the fp32 pass redoes exactly those blocks, without the host
    for (int arith : {FID_F16, FID_F32}) {
        FidTileP p; memset(&p, 0, sizeof(p));
        fill_tile(p, arith, feats, s, N, feats, s, N, D, Kp, g);
        p.flags = flags; p.lists = lists;
        FDCHK(c, car_launch_fid_tile(arith, FID_EPI_KSMALL, &p, st));
    }
    FDCHK(c, car_launch_fid_radii_fold(lists, (long)N, g.ncb, k, radii, st));
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int car_manifold_pr(car_ctx* c, const float* f1, const float* r1, int64_t N1, const float* f2, const float* r2, int64_t N2, int32_t D,
                               int64_t row_batch, int64_t col_batch, uint8_t* status1, uint8_t* status2, double* pr, void* stream_) {
    static const char* kWho = "car_manifold_pr";
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!f1 || !r1 || !f2 || !r2 || !status1 || !status2 || !pr) FAIL(c, "%s: no pointer may be NULL", kWho);
    if (fid_common_checks(c, kWho, N1, N2, D, row_batch, col_batch)) return -1;
    const int Kp = (int)rup((size_t)D, FID_KC);
    const FidGrid g = fid_grid(N1, N2, row_batch, col_batch);
    const double b1 = (double)g.ncb * (double)N1, b2 = (double)g.nrb * g.rt_per_rb * (double)N2;
    if (g.wgs > 2147483647.0 || b1 + b2 > (double)kMaxPart)
        FAIL(c, "%s: %d x %d blocks of (%lld, %lld) are too many for N %lld, %lld: raise row_batch / col_batch", kWho, g.nrb, g.ncb, (long long)row_batch, (long long)col_batch,
             (long long)N1, (long long)N2);
    const size_t n1 = (size_t)b1, n2 = (size_t)b2;
    FidCarve sz(nullptr);
    carve_set(sz, N1, Kp); carve_set(sz, N2, Kp); sz.take<int>((size_t)g.nrb * g.ncb); sz.take<uint8_t>(n1); sz.take<uint8_t>(n2);
    NEED(c, c->fid_ws, sz.off);
    FidCarve cv(c->fid_ws.p);
    const FidSet s1 = carve_set(cv, N1, Kp), s2 = carve_set(cv, N2, Kp);
    int* flags = cv.take<int>((size_t)g.nrb * g.ncb);
    uint8_t* s1part = cv.take<uint8_t>(n1);
    uint8_t* s2part = cv.take<uint8_t>(n2);
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    FDCHK(c, car_launch_fid_prep(f1, (long)N1, D, Kp, s1.h16, s1.nu16, s1.nu32, st));
    FDCHK(c, car_launch_fid_prep(f2, (long)N2, D, Kp, s2.h16, s2.nu16, s2.nu32, st));
    // flags, s1part and s2part are adjacent: row tiles behind the end of a short last row batch write no status part
    HIPCHK(c, hipMemsetAsync(flags, 0, (size_t)((char*)s2part - (char*)flags) + n2, st));
    for (int arith : {FID_F16, FID_F32}) {
        FidTileP p; memset(&p, 0, sizeof(p));
        fill_tile(p, arith, f1, s1, N1, f2, s2, N2, D, Kp, g);
        p.flags = flags; p.r1 = r1; p.r2 = r2; p.s1part = s1part; p.s2part = s2part;
        FDCHK(c, car_launch_fid_tile(arith, FID_EPI_THRESH, &p, st));
    }
    FDCHK(c, car_launch_fid_pr_fold(s1part, (long)N1, g.ncb, s2part, (long)N2, (long)g.nrb * g.rt_per_rb, status1, status2, pr, st));
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int car_debug_pairwise_distances(car_ctx* c, const float* U, int64_t n, const float* V, int64_t m, int32_t D, float* out, int32_t* used_fp32, void* stream_) {
    static const char* kWho = "car_debug_pairwise_distances";
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!U || !V || !out || !used_fp32) FAIL(c, "%s: no pointer may be NULL", kWho);
    if (fid_common_checks(c, kWho, n, m, D, n > 0 ? n : 1, m > 0 ? m : 1)) return -1;
    const int Kp = (int)rup((size_t)D, FID_KC);
    const FidGrid g = fid_grid(n, m, n, m);                 // one block
    FidCarve sz(nullptr);
    carve_set(sz, n, Kp); carve_set(sz, m, Kp);
    NEED(c, c->fid_ws, sz.off);
    FidCarve cv(c->fid_ws.p);
    const FidSet su = carve_set(cv, n, Kp), sv = carve_set(cv, m, Kp);
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    FDCHK(c, car_launch_fid_prep(U, (long)n, D, Kp, su.h16, su.nu16, su.nu32, st));
    FDCHK(c, car_launch_fid_prep(V, (long)m, D, Kp, sv.h16, sv.nu16, sv.nu32, st));
    HIPCHK(c, hipMemsetAsync(used_fp32, 0, sizeof(int32_t), st));
    for (int arith : {FID_F16, FID_F32}) {
        FidTileP p; memset(&p, 0, sizeof(p));
        fill_tile(p, arith, U, su, n, V, sv, m, D, Kp, g);
        p.flags = used_fp32; p.out = out; p.ldo = m;
        FDCHK(c, car_launch_fid_tile(arith, FID_EPI_STORE, &p, st));
    }
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int car_inception_score(car_ctx* c, const float* acts, int64_t N, int32_t D, const float* w, int32_t C, int64_t split_size, double* out, void* stream_) {
    static const char* kWho = "car_inception_score";
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!acts || !w || !out) FAIL(c, "%s: acts, w and out must not be NULL", kWho);
    if (N < 1 || N > 2147483647L) FAIL(c, "%s: N must be in 1 .. 2^31 - 1 (got %lld)", kWho, (long long)N);
    if (D < 1 || D > (1 << 20) || C < 1 || C > (1 << 20)) FAIL(c, "%s: D and C must be in 1 .. 2^20 (got %d and %d)", kWho, D, C);
    if (split_size < 1) FAIL(c, "%s: split_size must be positive (got %lld)", kWho, (long long)split_size);
    const long split = std::min<long>(split_size, N);
    const long splits = (N + split - 1) / split;
    if (splits > 65535) FAIL(c, "%s: at most 65535 splits (N %lld, split_size %lld)", kWho, (long long)N, (long long)split_size);
    const int chunks = (int)((split + 63) / 64), Kp = (int)rup((size_t)D, FID_KC);
    FidCarve sz(nullptr);
    sz.take<float>((size_t)C * D); sz.take<float>((size_t)N * C); sz.take<double>((size_t)splits * C); sz.take<double>((size_t)splits * chunks);
    NEED(c, c->fid_ws, sz.off);
    FidCarve cv(c->fid_ws.p);
    float* wt = cv.take<float>((size_t)C * D);
    float* z = cv.take<float>((size_t)N * C);
    double* logm = cv.take<double>((size_t)splits * C);
    double* part = cv.take<double>((size_t)splits * chunks);
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    FDCHK(c, car_launch_is_transpose(w, D, C, wt, st));
    // the logits acts . w on the distance tile loop in its fp32 arithmetic: rows of acts against rows of w^T
    const FidGrid g = fid_grid(N, C, N, C);
    FidTileP p; memset(&p, 0, sizeof(p));
    const FidSet none = {nullptr, nullptr, nullptr};
    fill_tile(p, FID_F32, acts, none, N, wt, none, C, D, Kp, g);
    p.out = z; p.ldo = C;
    FDCHK(c, car_launch_fid_tile(FID_F32, FID_EPI_PRODUCT, &p, st));
    FDCHK(c, car_launch_is_score(z, (long)N, C, split, (int)splits, chunks, logm, part, out, st));
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    return 0;
}
