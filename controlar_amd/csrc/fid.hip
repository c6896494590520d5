// fid.hip — the statistics half of evaluations/c2i/evaluator.py on the GPU (everything from compute_statistics down; the Inception tower is not here).
//   fid_prep            fp32 features -> their fp16 copy (round to nearest even, K padded with zeros) and both squared norms of every row.
//   fid_tile            ONE tile loop for every N x N x D product of the script: 128 rows x 64 columns per step on v_mfma_f32_16x16x32_f16 (FID_F16) or
//                       v_mfma_f32_16x16x4_f32 (FID_F32), two LDS stages.  The arithmetic decides how a product becomes a squared distance
//                       (_batch_pairwise_distances, evaluator.py:426-442); the epilogue what happens to the tile: the k+1 smallest values of every row
//                       (ManifoldEstimator.manifold_radii), the two threshold tests of DistanceBlock.less_thans, a plain store (car_debug_pairwise_distances),
//                       or the raw product (the logits of the Inception Score).  Nothing of size N x N is written.
//   fid_radii_fold / fid_status_fold / fid_pr_count     the per-column-batch lists and per-tile status bytes, merged in index order.
//   fid_shift / fid_sum / fid_cov / fid_finalize        np.mean and np.cov(rowvar=False) as a running fp64 state on v_mfma_f64_16x16x4_f64.
//   is_*                softmax(acts . w) in fp32, then compute_inception_score (evaluator.py:191-204) in fp64.
// No floating-point atomics and a fixed summation order everywhere: the same calls give the same bits.
#include "car_common.h"
#include "fid_params.h"

// Every product, sum and difference written with an operator below is rounded on its own: the distance is max((nu - 2 mm) + nv, 0) with one rounding
// per operation, and a contracted multiply-add would skip one.
#pragma clang fp contract(off)

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float fid_r16(float x) { return (float)(_Float16)x; }      // one fp16 rounding (an fp32 result rounded again: innocuous, 24 >= 2 * 11 + 2)

// ------------------------------------------------------------------------------------- features -> fp16 copy and norms
// one wave per row.  nu16 = fl16(sum in fp32 of fl16(h * h)), h the fp16 feature; nu32 = sum in fp32 of fl32(x * x); both sums lane-strided, then a butterfly.
__global__ __launch_bounds__(256) void fid_prep_kernel(const float* __restrict__ x, long N, int D, int Kp, _Float16* __restrict__ h16, _Float16* __restrict__ nu16,
                                                       float* __restrict__ nu32) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= N) return;
    const float* src = x + row * D;
    float s16 = 0.f, s32 = 0.f;
    for (int k = lane; k < Kp; k += 64) {
        const float v = k < D ? src[k] : 0.f;
        const float h = fid_r16(v);
        h16[row * Kp + k] = (_Float16)h;
        s16 = s16 + fid_r16(h * h);
        s32 = s32 + v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s16 = s16 + __shfl_xor(s16, o, 64); s32 = s32 + __shfl_xor(s32, o, 64); }
    if (lane == 0) { nu16[row] = (_Float16)s16; nu32[row] = s32; }
}

// ------------------------------------------------------------------------------------- the tile loop
template <int ARITH> struct FidArith;
template <> struct FidArith<FID_F16> {
    typedef _Float16 T;
    static constexpr int LD = 40, VE = 8;      // LDS row stride in elements (80 B), elements per 16 B
    // 16 bytes at element k of a row of the padded fp16 copy
    static __device__ __forceinline__ uint4 ldvec(const T* row, int k, int) { return *(const uint4*)(row + k); }
    static __device__ __forceinline__ float norm(const void* n, long i) { return (float)((const _Float16*)n)[i]; }
    // d = fl16(fl16(nu - fl16(2 fl16(acc))) + nv); *bad: d is not finite
    static __device__ __forceinline__ float dist(float acc, float nu, float nv, bool* bad) {
        const float mm = fid_r16(acc);
        const float t2 = fid_r16(2.0f * mm);
        const float t = fid_r16(nu - t2);
        const float d = fid_r16(t + nv);
        *bad = !(fabsf(d) <= 65504.0f);
        return fmaxf(d, 0.0f);
    }
};
template <> struct FidArith<FID_F32> {
    typedef float T;
    static constexpr int LD = 36, VE = 4;
    // the fp32 originals have an arbitrary row stride: element by element, zero behind D
    static __device__ __forceinline__ uint4 ldvec(const T* row, int k, int D) {
        uint4 v;
        v.x = k < D ? __float_as_uint(row[k]) : 0u; v.y = k + 1 < D ? __float_as_uint(row[k + 1]) : 0u;
        v.z = k + 2 < D ? __float_as_uint(row[k + 2]) : 0u; v.w = k + 3 < D ? __float_as_uint(row[k + 3]) : 0u;
        return v;
    }
    static __device__ __forceinline__ float norm(const void* n, long i) { return ((const float*)n)[i]; }
    static __device__ __forceinline__ float dist(float acc, float nu, float nv, bool* bad) {
        const float t2 = 2.0f * acc;
        const float t = nu - t2;
        const float d = t + nv;
        *bad = false;
        return fmaxf(d, 0.0f);
    }
};

// one staged k chunk: A points at row (lane & 15) of the wave's 32 rows, B at row (lane & 15) of the 64 columns
template <int ARITH>
__device__ __forceinline__ void fid_mfma_step(const typename FidArith<ARITH>::T* A, const typename FidArith<ARITH>::T* B, int lane, f32x4 (&acc)[2][4]) {
    constexpr int LD = FidArith<ARITH>::LD;
    if constexpr (ARITH == FID_F16) {
        f16x8 a[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = *(const f16x8*)&A[16 * i * LD + 8 * (lane >> 4)];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f16x8 b = *(const f16x8*)&B[16 * j * LD + 8 * (lane >> 4)];
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b, acc[i][j], 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            float a[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = A[16 * i * LD + 4 * ks + (lane >> 4)];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float b = B[16 * j * LD + 4 * ks + (lane >> 4)];
#pragma unroll
                for (int i = 0; i < 2; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b, acc[i][j], 0, 0, 0);
            }
        }
    }
}

// keeps the FID_KMAX smallest values seen, ascending, duplicates included
__device__ __forceinline__ void fid_insert(float (&L)[FID_KMAX], float d) {
    if (d < L[FID_KMAX - 1]) {
        L[FID_KMAX - 1] = d;
#pragma unroll
        for (int e = FID_KMAX - 1; e > 0; --e) {
            const float lo = fminf(L[e - 1], L[e]), hi = fmaxf(L[e - 1], L[e]);
            L[e - 1] = lo; L[e] = hi;
        }
    }
}

template <int ARITH, int EPI>
__global__ __launch_bounds__(256) void fid_tile_kernel(const FidTileP p) {
    using AR = FidArith<ARITH>;
    using T = typename AR::T;
    constexpr int LD = AR::LD, VE = AR::VE, VPR = FID_KC / VE, NA = FID_TM * VPR / 256, NB = FID_TN * VPR / 256, ABUF = FID_TM * LD, BBUF = FID_TN * LD;
    constexpr int STAGE_BYTES = 2 * (ABUF + BBUF) * (int)sizeof(T), CS_BYTES = FID_TM * FID_CLD * 4;
    constexpr int SMEM_BYTES = STAGE_BYTES > CS_BYTES ? STAGE_BYTES : CS_BYTES;             // As [2][128][LD] | Bs [2][64][LD], overlaid by Cs [128][FID_CLD]
    __shared__ __attribute__((aligned(16))) char smem[SMEM_BYTES];
    __shared__ float r1s[FID_TM], r2s[FID_TN];

    long wg = blockIdx.x;
    const int rt = (int)(wg % p.rt_per_rb); wg /= p.rt_per_rb;
    const int rb = (int)(wg % p.nrb), cb = (int)(wg / p.nrb);
    const int blk = cb * p.nrb + rb;
    if (ARITH == FID_F32 && p.flags && p.flags[blk] == 0) return;       // this block's fp16 distances were all finite
    const long r0 = (long)rb * p.row_batch + (long)rt * FID_TM;
    const long rend = ((long)rb + 1) * p.row_batch < p.N1 ? ((long)rb + 1) * p.row_batch : p.N1;
    if (r0 >= rend) return;                                             // the last row batch may be shorter
    const long cbeg = (long)cb * p.col_batch, cend = cbeg + p.col_batch < p.N2 ? cbeg + p.col_batch : p.N2;
    const int nr = rend - r0 < FID_TM ? (int)(rend - r0) : FID_TM;

    T* const As = (T*)smem;
    T* const Bs = As + 2 * ABUF;
    float* const Cs = (float*)smem;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // vector v of this thread is k slice rko[v] of tile row rrow[v]; rows behind the batch's end repeat its last row and are masked in the epilogue
    int rrow[NA], rko[NA];
    const T* arow[NA];
#pragma unroll
    for (int v = 0; v < NA; ++v) {
        const int vi = tid + v * 256;
        rrow[v] = vi / VPR; rko[v] = (vi % VPR) * VE;
        const long r = r0 + rrow[v] < rend ? r0 + rrow[v] : rend - 1;
        arow[v] = (const T*)p.U + r * p.ldu;
    }
    float nu[2][4];
    if constexpr (EPI != FID_EPI_PRODUCT) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = r0 + 32 * wv + 16 * i + 4 * (lane >> 4) + r;
                nu[i][r] = AR::norm(p.nu, row < rend ? row : rend - 1);
            }
    }
    if constexpr (EPI == FID_EPI_THRESH) { if (tid < FID_TM) r1s[tid] = p.r1[r0 + tid < rend ? r0 + tid : rend - 1]; }
    float L[FID_KMAX];
#pragma unroll
    for (int e = 0; e < FID_KMAX; ++e) L[e] = INFINITY;
    bool any1 = false, anybad = false;

    for (long c0 = cbeg; c0 < cend; c0 += FID_TN) {
        const int nc = cend - c0 < FID_TN ? (int)(cend - c0) : FID_TN;
        const T* brow[NB];
#pragma unroll
        for (int v = 0; v < NB; ++v) {
            const long c = c0 + rrow[v] < cend ? c0 + rrow[v] : cend - 1;
            brow[v] = (const T*)p.V + c * p.ldv;
        }
        if constexpr (EPI == FID_EPI_THRESH) { if (tid >= 128 && tid < 128 + FID_TN) r2s[tid - 128] = p.r2[c0 + tid - 128 < cend ? c0 + tid - 128 : cend - 1]; }
        f32x4 acc[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        uint4 ra[NA], rbv[NB];
        auto load = [&](int k0) {
#pragma unroll
            for (int v = 0; v < NA; ++v) ra[v] = AR::ldvec(arow[v], k0 + rko[v], p.D);
#pragma unroll
            for (int v = 0; v < NB; ++v) rbv[v] = AR::ldvec(brow[v], k0 + rko[v], p.D);
        };
        auto stage = [&](int buf) {
            T* A = As + buf * ABUF; T* B = Bs + buf * BBUF;
#pragma unroll
            for (int v = 0; v < NA; ++v) *(uint4*)&A[rrow[v] * LD + rko[v]] = ra[v];
#pragma unroll
            for (int v = 0; v < NB; ++v) *(uint4*)&B[rrow[v] * LD + rko[v]] = rbv[v];
        };
        load(0);
        stage(0);
        __syncthreads();
        int cur = 0;
        for (int k0 = 0; k0 < p.Kp; k0 += FID_KC) {
            const bool more = k0 + FID_KC < p.Kp;
            if (more) load(k0 + FID_KC);
            fid_mfma_step<ARITH>(As + cur * ABUF + (32 * wv + (lane & 15)) * LD, Bs + cur * BBUF + (lane & 15) * LD, lane, acc);
            if (more) stage(cur ^ 1);             // the other stage: its last readers passed the barrier that ended the previous chunk
            __syncthreads();
            cur ^= 1;
        }
        // accumulators (col = lane & 15, row = 4 * (lane >> 4) + r) -> distances -> Cs, which overlays the stages: every wave is past the loop's last barrier
        float nv[4];
        if constexpr (EPI != FID_EPI_PRODUCT) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const long c = c0 + 16 * j + (lane & 15); nv[j] = AR::norm(p.nv, c < cend ? c : cend - 1); }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 32 * wv + 16 * i + 4 * (lane >> 4) + r, col = 16 * j + (lane & 15);
                    float d = acc[i][j][r];
                    if constexpr (EPI != FID_EPI_PRODUCT) {
                        bool bad;
                        d = AR::dist(d, nu[i][r], nv[j], &bad);
                        anybad |= bad && row < nr && col < nc;
                    }
                    Cs[row * FID_CLD + col] = d;
                }
        __syncthreads();
        if constexpr (EPI == FID_EPI_KSMALL) {
            if (tid < nr) for (int c = 0; c < nc; ++c) fid_insert(L, Cs[tid * FID_CLD + c]);
        } else if constexpr (EPI == FID_EPI_THRESH) {
            if (tid < nr) {
                for (int c = 0; c < nc; ++c) any1 |= Cs[tid * FID_CLD + c] <= r2s[c];
            } else if (tid >= 128 && tid - 128 < nc) {
                bool any2 = false;
                for (int r = 0; r < nr; ++r) any2 |= Cs[r * FID_CLD + tid - 128] <= r1s[r];
                p.s2part[((long)rb * p.rt_per_rb + rt) * p.N2 + c0 + tid - 128] = any2 ? 1 : 0;
            }
        } else {
            for (int e = tid; e < FID_TM * FID_TN; e += 256) {
                const int row = e / FID_TN, col = e % FID_TN;
                if (row < nr && col < nc) p.out[(r0 + row) * p.ldo + c0 + col] = Cs[row * FID_CLD + col];
            }
        }
        __syncthreads();                          // the next column tile stages over Cs
    }
    if (ARITH == FID_F16 && p.flags && anybad) p.flags[blk] = 1;        // every writer stores the same value
    if constexpr (EPI == FID_EPI_KSMALL) {
        if (tid < nr) {
            float* o = p.lists + ((long)cb * p.N1 + r0 + tid) * FID_KMAX;
#pragma unroll
            for (int e = 0; e < FID_KMAX; ++e) o[e] = L[e];
        }
    } else if constexpr (EPI == FID_EPI_THRESH) {
        if (tid < nr) p.s1part[(long)cb * p.N1 + r0 + tid] = any1 ? 1 : 0;
    }
}

// the lists of the column batches in index order -> the (k+1)-th smallest of the whole row
__global__ __launch_bounds__(256) void fid_radii_fold_kernel(const float* __restrict__ lists, long N, int ncb, int k, float* __restrict__ radii) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    float L[FID_KMAX];
#pragma unroll
    for (int e = 0; e < FID_KMAX; ++e) L[e] = INFINITY;
    for (int cb = 0; cb < ncb; ++cb) {
        const float* q = lists + ((long)cb * N + i) * FID_KMAX;
#pragma unroll
        for (int e = 0; e < FID_KMAX; ++e) fid_insert(L, q[e]);
    }
    float r = L[0];
#pragma unroll
    for (int e = 1; e < FID_KMAX; ++e) if (e == k) r = L[e];
    radii[i] = r;
}

// out[i] = OR over parts of part[q][i]
__global__ __launch_bounds__(256) void fid_status_fold_kernel(const unsigned char* __restrict__ part, long N, long parts, unsigned char* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    unsigned char v = 0;
    for (long q = 0; q < parts; ++q) v |= part[q * N + i];
    out[i] = v;
}
// one workgroup: pr = (mean status2, mean status1); integer counts, so no order matters
__global__ __launch_bounds__(1024) void fid_pr_count_kernel(const unsigned char* __restrict__ s1, long N1, const unsigned char* __restrict__ s2, long N2, double* __restrict__ pr) {
    __shared__ unsigned long long sm[2][16];
    unsigned long long c1 = 0, c2 = 0;
    for (long i = threadIdx.x; i < N1; i += 1024) c1 += s1[i];
    for (long i = threadIdx.x; i < N2; i += 1024) c2 += s2[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { c1 += __shfl_xor(c1, o, 64); c2 += __shfl_xor(c2, o, 64); }
    if ((threadIdx.x & 63) == 0) { sm[0][threadIdx.x >> 6] = c1; sm[1][threadIdx.x >> 6] = c2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        c1 = c2 = 0;
        for (int i = 0; i < 16; ++i) { c1 += sm[0][i]; c2 += sm[1][i]; }
        pr[0] = (double)c2 / (double)N2; pr[1] = (double)c1 / (double)N1;
    }
}

// ------------------------------------------------------------------------------------- moments (state: n | c [D] | s [D] | S [D][D], all fp64)
// fp64 sum of one column of v(row) over the batch: row group g = threadIdx.x >> 6 takes rows g, g + 4, ... in order, the four groups are added in order
template <typename F>
__device__ __forceinline__ double fid_colsum(long n, bool ok, double (*sm)[64], F v) {
    const int g = threadIdx.x >> 6, cl = threadIdx.x & 63;
    double a = 0.0;
    if (ok) for (long r = g; r < n; r += 4) a = a + v(r);
    sm[g][cl] = a;
    __syncthreads();
    return ((sm[0][cl] + sm[1][cl]) + sm[2][cl]) + sm[3][cl];
}
// an empty state takes its shift from this batch: the column mean rounded to fp32.  grid ceil(D / 64)
__global__ __launch_bounds__(256) void fid_shift_kernel(const float* __restrict__ x, long n, int D, double* __restrict__ st) {
    __shared__ double sm[4][64];
    if (st[0] != 0.0) return;
    const int col = blockIdx.x * 64 + (threadIdx.x & 63);
    const bool ok = col < D;
    const double s = fid_colsum(n, ok, sm, [&](long r) { return (double)x[r * D + col]; });
    if (ok && threadIdx.x < 64) st[1 + col] = (double)(float)(s / (double)n);
}
// s += sum of (x - c); the last thing the block of column 0 does is n += the batch (fid_shift of this call has read n, nothing later in it does)
__global__ __launch_bounds__(256) void fid_sum_kernel(const float* __restrict__ x, long n, int D, double* __restrict__ st) {
    __shared__ double sm[4][64];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63);
    const bool ok = col < D;
    const double c = ok ? st[1 + col] : 0.0;
    const double s = fid_colsum(n, ok, sm, [&](long r) { return (double)x[r * D + col] - c; });
    if (ok && threadIdx.x < 64) st[1 + D + col] = st[1 + D + col] + s;
    if (blockIdx.x == 0 && threadIdx.x == 0) st[0] = st[0] + (double)n;
}
// S += y^T y, y = x - c: workgroup (ti <= tj) owns the 64 x 64 tile (ti, tj) and its mirror image; wave w the rows 16 w .. of it.  The accumulators start from
// the state, so the sum over all updates is one k-ordered fma chain.  f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg.
__global__ __launch_bounds__(256) void fid_cov_kernel(const float* __restrict__ x, long n, int D, double* __restrict__ st) {
    __shared__ double Ya[FID_COV_K][FID_COV_LD], Yb[FID_COV_K][FID_COV_LD];
    // blockIdx.x enumerates the pairs ti <= tj row by row
    const int T = (D + FID_COV_T - 1) / FID_COV_T;
    int ti = 0, rem = blockIdx.x;
    while (rem >= T - ti) { rem -= T - ti; ++ti; }
    const int tj = ti + rem;
    const bool diag = ti == tj;
    const int i0 = ti * FID_COV_T, j0 = tj * FID_COV_T;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double* c = st + 1;
    double* S = st + 1 + 2 * (long)D;
    f64x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = i0 + 16 * wv + (lane >> 4) + 4 * r, col = j0 + 16 * j + (lane & 15);
            acc[j][r] = row < D && col < D ? S[(long)row * D + col] : 0.0;
        }
    const int scol = tid & 63, srow = tid >> 6;
    const bool oka = i0 + scol < D, okb = j0 + scol < D;
    const double ca = oka ? c[i0 + scol] : 0.0, cbv = okb ? c[j0 + scol] : 0.0;
    const double (*B)[FID_COV_LD] = diag ? Ya : Yb;
    for (long k0 = 0; k0 < n; k0 += FID_COV_K) {
#pragma unroll
        for (int e = 0; e < FID_COV_K / 4; ++e) {
            const long r = k0 + srow + 4 * e;
            Ya[srow + 4 * e][scol] = oka && r < n ? (double)x[r * D + i0 + scol] - ca : 0.0;
            if (!diag) Yb[srow + 4 * e][scol] = okb && r < n ? (double)x[r * D + j0 + scol] - cbv : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < FID_COV_K / 4; ++ks) {
            const double a = Ya[4 * ks + (lane >> 4)][16 * wv + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, B[4 * ks + (lane >> 4)][16 * j + (lane & 15)], acc[j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = i0 + 16 * wv + (lane >> 4) + 4 * r, col = j0 + 16 * j + (lane & 15);
            if (row < D && col < D) {
                S[(long)row * D + col] = acc[j][r];
                if (!diag) S[(long)col * D + row] = acc[j][r];
            }
        }
}
// mu = c + s / n; sigma = (S - s s^T / n) / (n - 1), written in full
__global__ __launch_bounds__(256) void fid_finalize_kernel(const double* __restrict__ st, int D, double* __restrict__ mu, double* __restrict__ sigma) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)D * D) return;
    const int i = (int)(e / D), j = (int)(e % D);
    const double n = st[0];
    const double* s = st + 1 + D;
    const double* S = st + 1 + 2 * (long)D;
    const double m = s[i] * s[j] / n;
    sigma[e] = (S[e] - m) / (n - 1.0);
    if (e < D) mu[e] = st[1 + e] + s[e] / n;
}

// ------------------------------------------------------------------------------------- Inception Score
__global__ __launch_bounds__(256) void is_transpose_kernel(const float* __restrict__ w, int D, int C, float* __restrict__ wt) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)D * C) return;
    const int c = (int)(e / D), d = (int)(e % D);
    wt[e] = w[(long)d * C + c];
}
// one wave per row, in place: exp(x - max) / sum, fp32
__global__ __launch_bounds__(256) void is_softmax_kernel(float* __restrict__ z, long N, int C) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= N) return;
    float* q = z + row * C;
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, q[c]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) { const float e = expf(q[c] - m); q[c] = e; s = s + e; }
    s = wave_sum(s);
    for (int c = lane; c < C; c += 64) q[c] = __fdiv_rn(q[c], s);
}
// grid (ceil(C / 64), splits): logm[split][c] = log(mean over the split's rows of p[., c]), fp64
__global__ __launch_bounds__(256) void is_colmean_kernel(const float* __restrict__ p, long N, int C, long split, double* __restrict__ logm) {
    __shared__ double sm[4][64];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63);
    const bool ok = col < C;
    const long r0 = (long)blockIdx.y * split, n = N - r0 < split ? N - r0 : split;
    const double s = fid_colsum(n, ok, sm, [&](long r) { return (double)p[(r0 + r) * C + col]; });
    if (ok && threadIdx.x < 64) logm[(long)blockIdx.y * C + col] = log(s / (double)n);
}
// grid (chunks, splits): part[split][chunk] = sum over 64 rows of sum_c p (log p - logm); a wave takes 16 rows one after the other
__global__ __launch_bounds__(256) void is_kl_kernel(const float* __restrict__ p, long N, int C, long split, int chunks, const double* __restrict__ logm, double* __restrict__ part) {
    __shared__ double sm[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long r0 = (long)blockIdx.y * split, n = N - r0 < split ? N - r0 : split;
    const double* lm = logm + (long)blockIdx.y * C;
    double acc = 0.0;
    for (int e = 0; e < 16; ++e) {
        const long r = (long)blockIdx.x * 64 + 16 * wv + e;
        if (r >= n) break;
        const float* q = p + (r0 + r) * C;
        double v = 0.0;
        for (int c = lane; c < C; c += 64) { const double pc = (double)q[c]; v = v + pc * (log(pc) - lm[c]); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
        acc = acc + v;
    }
    if (lane == 0) sm[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(long)blockIdx.y * chunks + blockIdx.x] = ((sm[0] + sm[1]) + sm[2]) + sm[3];
}
// one thread: out[1 + s] = exp(mean over the split's rows), out[0] = the mean of those
__global__ void is_final_kernel(const double* __restrict__ part, long N, long split, int splits, int chunks, double* __restrict__ out) {
    double tot = 0.0;
    for (int s = 0; s < splits; ++s) {
        const long r0 = (long)s * split, n = N - r0 < split ? N - r0 : split;
        double a = 0.0;
        for (int q = 0; q < chunks; ++q) a = a + part[(long)s * chunks + q];
        const double v = exp(a / (double)n);
        out[1 + s] = v;
        tot = tot + v;
    }
    out[0] = tot / (double)splits;
}

// ------------------------------------------------------------------------------------- launchers: every one returns the launch status
extern "C" int car_launch_fid_prep(const float* x, long N, int D, int Kp, void* h16, void* nu16, float* nu32, hipStream_t st) {
    if (N <= 0 || D <= 0 || Kp < D || Kp % FID_KC) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fid_prep_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, x, N, D, Kp, (_Float16*)h16, (_Float16*)nu16, nu32);
    return (int)hipGetLastError();
}
template <int ARITH> static void fid_tile_launch(int epi, const FidTileP* p, unsigned grid, hipStream_t st) {
    switch (epi) {
        case FID_EPI_KSMALL: hipLaunchKernelGGL((fid_tile_kernel<ARITH, FID_EPI_KSMALL>), dim3(grid), dim3(256), 0, st, *p); break;
        case FID_EPI_THRESH: hipLaunchKernelGGL((fid_tile_kernel<ARITH, FID_EPI_THRESH>), dim3(grid), dim3(256), 0, st, *p); break;
        case FID_EPI_STORE: hipLaunchKernelGGL((fid_tile_kernel<ARITH, FID_EPI_STORE>), dim3(grid), dim3(256), 0, st, *p); break;
        default: hipLaunchKernelGGL((fid_tile_kernel<ARITH, FID_EPI_PRODUCT>), dim3(grid), dim3(256), 0, st, *p); break;
    }
}
extern "C" int car_launch_fid_tile(int arith, int epi, const FidTileP* p, hipStream_t st) {
    const double wgs = (double)p->rt_per_rb * p->nrb * p->ncb;
    if (p->N1 <= 0 || p->N2 <= 0 || p->D <= 0 || p->Kp < p->D || p->Kp % FID_KC || p->row_batch <= 0 || p->col_batch <= 0 || p->rt_per_rb <= 0 || p->nrb <= 0 ||
        p->ncb <= 0 || wgs > 2147483647.0 || (long)p->nrb * p->row_batch < p->N1 || (long)p->ncb * p->col_batch < p->N2 ||
        (long)p->rt_per_rb * FID_TM < p->row_batch || !p->U || !p->V || epi < FID_EPI_KSMALL || epi > FID_EPI_PRODUCT || (arith != FID_F16 && arith != FID_F32) ||
        (arith == FID_F16 && (epi == FID_EPI_PRODUCT || p->ldu != p->Kp || p->ldv != p->Kp)) || (arith == FID_F32 && (p->ldu < p->D || p->ldv < p->D)) ||
        (epi != FID_EPI_PRODUCT && (!p->nu || !p->nv)) || (epi == FID_EPI_KSMALL && !p->lists) ||
        (epi == FID_EPI_THRESH && (!p->r1 || !p->r2 || !p->s1part || !p->s2part)) || (epi >= FID_EPI_STORE && (!p->out || p->ldo < p->N2)))
        return (int)hipErrorInvalidValue;
    if (arith == FID_F16) fid_tile_launch<FID_F16>(epi, p, (unsigned)wgs, st); else fid_tile_launch<FID_F32>(epi, p, (unsigned)wgs, st);
    return (int)hipGetLastError();
}
extern "C" int car_launch_fid_radii_fold(const float* lists, long N, int ncb, int k, float* radii, hipStream_t st) {
    if (N <= 0 || ncb <= 0 || k < 0 || k >= FID_KMAX) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fid_radii_fold_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, lists, N, ncb, k, radii);
    return (int)hipGetLastError();
}
extern "C" int car_launch_fid_pr_fold(const unsigned char* s1part, long N1, long parts1, const unsigned char* s2part, long N2, long parts2,
                                      unsigned char* status1, unsigned char* status2, double* pr, hipStream_t st) {
    if (N1 <= 0 || N2 <= 0 || parts1 <= 0 || parts2 <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fid_status_fold_kernel, dim3((unsigned)((N1 + 255) / 256)), dim3(256), 0, st, s1part, N1, parts1, status1);
    hipLaunchKernelGGL(fid_status_fold_kernel, dim3((unsigned)((N2 + 255) / 256)), dim3(256), 0, st, s2part, N2, parts2, status2);
    hipLaunchKernelGGL(fid_pr_count_kernel, dim3(1), dim3(1024), 0, st, (const unsigned char*)status1, N1, (const unsigned char*)status2, N2, pr);
    return (int)hipGetLastError();
}
extern "C" int car_launch_fid_accumulate(const float* x, long n, int D, double* state, hipStream_t st) {
    if (n <= 0 || D <= 0) return (int)hipErrorInvalidValue;
    const int cb = (D + 63) / 64, T = (D + FID_COV_T - 1) / FID_COV_T;
    hipLaunchKernelGGL(fid_shift_kernel, dim3(cb), dim3(256), 0, st, x, n, D, state);
    hipLaunchKernelGGL(fid_sum_kernel, dim3(cb), dim3(256), 0, st, x, n, D, state);
    hipLaunchKernelGGL(fid_cov_kernel, dim3((unsigned)((long)T * (T + 1) / 2)), dim3(256), 0, st, x, n, D, state);
    return (int)hipGetLastError();
}
extern "C" int car_launch_fid_finalize(const double* state, int D, double* mu, double* sigma, hipStream_t st) {
    if (D <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fid_finalize_kernel, dim3((unsigned)(((long)D * D + 255) / 256)), dim3(256), 0, st, state, D, mu, sigma);
    return (int)hipGetLastError();
}
extern "C" int car_launch_is_transpose(const float* w, int D, int C, float* wt, hipStream_t st) {
    hipLaunchKernelGGL(is_transpose_kernel, dim3((unsigned)(((long)D * C + 255) / 256)), dim3(256), 0, st, w, D, C, wt);
    return (int)hipGetLastError();
}
extern "C" int car_launch_is_score(float* z, long N, int C, long split, int splits, int chunks, double* logm, double* part, double* out, hipStream_t st) {
    if (N <= 0 || C <= 0 || split <= 0 || splits <= 0 || splits > 65535 || chunks <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(is_softmax_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, z, N, C);
    hipLaunchKernelGGL(is_colmean_kernel, dim3((C + 63) / 64, splits), dim3(256), 0, st, (const float*)z, N, C, split, logm);
    hipLaunchKernelGGL(is_kl_kernel, dim3(chunks, splits), dim3(256), 0, st, (const float*)z, N, C, split, chunks, (const double*)logm, part);
    hipLaunchKernelGGL(is_final_kernel, dim3(1), dim3(1), 0, st, (const double*)part, N, split, splits, chunks, out);
    return (int)hipGetLastError();
}
