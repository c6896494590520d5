// score.hip — car_score's own kernels: the fused vocabulary projection + cross-entropy, and the three small kernels that lay one teacher-forced pass out
// (token-embedding rows, RoPE in place without a KV cache, the causal mask extended over the image rows).
//
// score_kernel: logits = xn · output.weight^T reduced to (max, sum of exp, target logit) per row WITHOUT writing the [rows, V] tensor (XL, 1024 tokens:
// 67 MB per sequence).  Workgroup = 4 waves = a tile of 128 X rows x 128 vocabulary columns per step, wave (wm, wn) owns 64 x 64 of it as 4 x 4 accumulator
// fragments; K runs through a double-buffered LDS stage, the loader and fragment reads of gemm.hip's tiles (bf16: v_mfma_f32_16x16x32_bf16, 32 k per stage,
// row stride 40; fp32: the exact v_mfma_f32_16x16x4_f32, 16 k per stage, row stride 20, the same fixed k permutation inside a 16-block).  The weight fragment
// is the A operand and the X fragment the B operand: D[n = (lane >> 4) * 4 + r][m = lane & 15], so a lane holds 16 logits of ONE row per fragment column and
// the row statistics need two xor-shuffles (16, 32) per tile, as in attn.hip.  The workgroup walks the vocabulary tiles of its grid.y slice with a running
// maximum and a rescaled running sum per row (online log-sum-exp, fp32, expf / logf), and picks the target's logit out of the tile that holds it.
// CFG: the 16-row fragments of a tile alternate [cond | uncond] of the same 16 (image, position) pairs, so both accumulators of a pair sit in the same lane
// and register slot; the mix u + (c - u) * s runs on the accumulators with a PER-ROW scale (cfg_interval: s = 1 takes the conditional row as it is, what
// sample_greedy_kernel does).  With `logits` set the mixed accumulators are also stored: nll and logits of one call describe the same numbers.
// Order: per row and part the tiles are folded in ascending order and every sum has a fixed association; the parts ([grid.y][wn]) are folded in index order
// by score_fold_kernel.  No atomics.  The split depends on V alone, never on the number of rows: a row's nll does not depend on its batch.
#include "car_common.h"
#include "kernel_params.h"

typedef __attribute__((ext_vector_type(4))) float sc_f4;

// the X row of slot `s` (0..127) of row tile `t`, or -1 past the last output row
template <int PAIRED>
__device__ __forceinline__ long score_xrow(const ScoreP& p, int t, int s) {
    int orow, u = 0;
    if (PAIRED) { const int f = s >> 4; orow = t * 64 + (f >> 1) * 16 + (s & 15); u = f & 1; }
    else orow = t * 128 + s;
    if (orow >= p.R) return -1;
    const int q = orow / p.rows_per_seq, i = orow - q * p.rows_per_seq;
    return (long)q * p.seq_stride + p.row_off + i + (u ? p.unc_off : 0);
}

template <typename T, int PAIRED>
__global__ __launch_bounds__(256) void score_kernel(ScoreP p) {
    constexpr bool BF = ET<T>::mode == 1;
    constexpr int LD = BF ? 40 : 20;                   // LDS row stride in elements (80 bytes)
    constexpr int KS = BF ? 32 : 16;                   // k per stage: 64 bytes of every row
    constexpr int EPC = 16 / (int)sizeof(T);           // elements per 16-byte chunk
    constexpr int NO = PAIRED ? 2 : 4;                 // output-row fragments per wave
    __shared__ __attribute__((aligned(16))) T sX[2][128 * LD];
    __shared__ __attribute__((aligned(16))) T sW[2][128 * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    const int t = blockIdx.x, split = blockIdx.y;
    const T* X = (const T*)p.x; const T* W = (const T*)p.w;
    // loader: two 16-byte chunks of X and of W per thread and stage (rows tid >> 2 and + 64, chunk tid & 3)
    const int lrow0 = tid >> 2, lrow1 = lrow0 + 64, lkc = (tid & 3) * EPC;
    const long xr0 = score_xrow<PAIRED>(p, t, lrow0), xr1 = score_xrow<PAIRED>(p, t, lrow1);
    const T* x0p = xr0 >= 0 ? X + xr0 * p.ldx + lkc : nullptr;
    const T* x1p = xr1 >= 0 ? X + xr1 * p.ldx + lkc : nullptr;

    int orow[NO], tgt[NO]; float sc[NO], m[NO], l[NO], tg[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        orow[o] = PAIRED ? t * 64 + (wm * 2 + o) * 16 + fr : t * 128 + (wm * 4 + o) * 16 + fr;
        const bool valid = orow[o] < p.R;
        tgt[o] = valid ? p.targets[orow[o]] : -1;
        sc[o] = 1.f;
        if (PAIRED && valid) sc[o] = p.scale ? p.scale[orow[o]] : ((p.cfg_interval > -1 && (orow[o] % p.rows_per_seq) - 1 > p.cfg_interval) ? 1.f : p.cfg_scale);
        m[o] = -INFINITY; l[o] = 0.f; tg[o] = 0.f;
    }
    const int ntiles = (p.V + 127) >> 7;
    const int nt0 = split * p.tiles_per_split, nt1 = min(nt0 + p.tiles_per_split, ntiles);
    const int nk = p.D / KS;
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    for (int nt = nt0; nt < nt1; ++nt) {
        const int n0 = nt * 128;
        const T* w0p = (n0 + lrow0) < p.V ? W + (long)(n0 + lrow0) * p.D + lkc : nullptr;
        const T* w1p = (n0 + lrow1) < p.V ? W + (long)(n0 + lrow1) * p.D + lkc : nullptr;
        uint4 ra0, ra1, rb0, rb1;
        auto gload = [&](int kt) {
            const long k = (long)kt * KS;
            ra0 = x0p ? *(const uint4*)(x0p + k) : zero4; ra1 = x1p ? *(const uint4*)(x1p + k) : zero4;
            rb0 = w0p ? *(const uint4*)(w0p + k) : zero4; rb1 = w1p ? *(const uint4*)(w1p + k) : zero4;
        };
        auto sstore = [&](int buf) {
            *(uint4*)&sX[buf][lrow0 * LD + lkc] = ra0; *(uint4*)&sX[buf][lrow1 * LD + lkc] = ra1;
            *(uint4*)&sW[buf][lrow0 * LD + lkc] = rb0; *(uint4*)&sW[buf][lrow1 * LD + lkc] = rb1;
        };
        f32x4 acc[4][4];      // [i: 16 vocabulary columns][j: 16 X rows]
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        gload(0); sstore(0);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < nk) gload(kt + 1);
            if constexpr (BF) {
                bf16x8 a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = *(const bf16x8*)&sW[buf][(wn * 64 + i * 16 + fr) * LD + fq * 8];
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = *(const bf16x8*)&sX[buf][(wm * 64 + j * 16 + fr) * LD + fq * 8];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
            } else {
                sc_f4 wa[4], xa[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) wa[i] = *(const sc_f4*)&sW[buf][(wn * 64 + i * 16 + fr) * LD + fq * 4];
#pragma unroll
                for (int j = 0; j < 4; ++j) xa[j] = *(const sc_f4*)&sX[buf][(wm * 64 + j * 16 + fr) * LD + fq * 4];
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[i][s], xa[j][s], acc[i][j], 0, 0, 0);
            }
            if (kt + 1 < nk) sstore(buf ^ 1);
            __syncthreads();
        }
        // ---- the tile's 64 columns of this wave: (rounding,) CFG mix, optional store, target pick, online log-sum-exp per row = per lane column
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            float v[4][4];
            float mx = -INFINITY;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int nb = n0 + wn * 64 + i * 16 + fq * 4;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float c = PAIRED ? acc[i][2 * o][r] : acc[i][o][r];
                    if (p.round_bf16) c = bf2f(f2bf(c));
                    if (PAIRED) {
                        float u = acc[i][2 * o + 1][r];
                        if (p.round_bf16) u = bf2f(f2bf(u));
                        c = sc[o] == 1.f ? c : u + (c - u) * sc[o];
                    }
                    if (nb + r >= p.V) c = -INFINITY;
                    if (nb + r == tgt[o]) tg[o] = c;
                    v[i][r] = c; mx = fmaxf(mx, c);
                }
                if (p.logits && orow[o] < p.R && nb < p.V)      // V % 4 == 0: the four columns are in range together
                    *(float4*)(p.logits + (long)orow[o] * p.V + nb) = make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64)); mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mn = fmaxf(m[o], mx);
            const float base = mn == -INFINITY ? 0.f : mn;      // no column of this wave in range yet: every term is 0
            float ps = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) ps += expf(v[i][r] - base);
            ps += __shfl_xor(ps, 16, 64); ps += __shfl_xor(ps, 32, 64);
            l[o] = l[o] * expf(m[o] - base) + ps; m[o] = mn;
        }
    }
    // ---- one (max, sum, target logit) per row and part; the lane group that held the target's column has it, the others add exact zeros
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        float tv = tg[o];
        tv += __shfl_xor(tv, 16, 64); tv += __shfl_xor(tv, 32, 64);
        if (fq == 0 && orow[o] < p.R)
            *(float4*)(p.part + ((long)(split * 2 + wn) * p.R + orow[o]) * 4) = make_float4(m[o], l[o], tv, 0.f);
    }
}

// nll[r] = (max - target logit) + log(sum), the parts folded in index order.  A target outside [0, V) took no logit: the sticky flag marks the call invalid.
__global__ __launch_bounds__(256) void score_fold_kernel(const float* part, int nparts, int R, const int* targets, int V, float* nll, int* err_flag) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    float M = -INFINITY;
    for (int k = 0; k < nparts; ++k) M = fmaxf(M, part[((long)k * R + r) * 4]);
    float S = 0.f, tv = 0.f;
    for (int k = 0; k < nparts; ++k) {
        const float4 q = *(const float4*)(part + ((long)k * R + r) * 4);
        if (q.x > -INFINITY) S += q.y * expf(q.x - M);
        tv += q.z;
    }
    nll[r] = (M - tv) + logf(S);
    const int t = targets[r];
    if ((t < 0 || t >= V) && err_flag) __hip_atomic_store(err_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// vocabulary parts per row: 2 (the wave columns of a tile) x the grid.y slices; a function of V alone
static int score_nsplit(int V) { const int ntiles = (V + 127) / 128; int ns = ntiles / 16; if (ns < 1) ns = 1; if (ns > 8) ns = 8; return ns; }
extern "C" int car_score_nparts(int V) { return 2 * score_nsplit(V); }

// 0, or -1 when the shape breaks the loader's rules (nothing launched).  p->part holds car_score_nparts(V) * R * 4 floats.
extern "C" int car_launch_score(int mode, const ScoreP* pp, float* nll, int* err_flag, hipStream_t st) {
    ScoreP p = *pp;
    const size_t es = mode == 1 ? 2 : 4;
    if (p.R <= 0 || p.V <= 0 || (p.V & 3) || p.D <= 0 || p.D % (mode == 1 ? 32 : 16) || p.rows_per_seq <= 0 || ((p.ldx * es) & 15) ||
        ((uintptr_t)p.x & 15) || ((uintptr_t)p.w & 15) || ((uintptr_t)p.part & 15) || ((uintptr_t)p.logits & 15)) return -1;
    p.nsplit = score_nsplit(p.V);
    const int ntiles = (p.V + 127) / 128;
    p.tiles_per_split = (ntiles + p.nsplit - 1) / p.nsplit;
    const dim3 g((unsigned)((p.R + (p.paired ? 63 : 127)) / (p.paired ? 64 : 128)), (unsigned)p.nsplit);
    if (mode == 1) { if (p.paired) hipLaunchKernelGGL((score_kernel<bf16_t, 1>), g, dim3(256), 0, st, p); else hipLaunchKernelGGL((score_kernel<bf16_t, 0>), g, dim3(256), 0, st, p); }
    else { if (p.paired) hipLaunchKernelGGL((score_kernel<float, 1>), g, dim3(256), 0, st, p); else hipLaunchKernelGGL((score_kernel<float, 0>), g, dim3(256), 0, st, p); }
    hipLaunchKernelGGL(score_fold_kernel, dim3((unsigned)((p.R + 255) / 256)), dim3(256), 0, st, p.part, 2 * p.nsplit, p.R, p.targets, p.V, nll, err_flag);
    return 0;
}

// ------------------------------------------------------------------ the pass's input rows
// h[(s * Ts + Tv + j), :] = tok_embeddings[tokens[s % ng][j]] for j < n_new - 1: the rows behind the prefix window of sequence s (the chunk's sequences are
// [cond 0..ng) | uncond 0..ng), both halves feed the same tokens back, generate.py:88-92).  An id outside [0, V) reads row 0 and raises the sticky flag.
template <typename T>
__global__ void score_embed_kernel(const void* emb, const int* tokens, void* h, int nseq, int ng, int n_new, int Ts, int Tv, int D, int V, int* err_flag) {
    const long total = (long)nseq * (n_new - 1) * D;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        const int d = (int)(i % D); const long rr = i / D; const int j = (int)(rr % (n_new - 1)); const int s = (int)(rr / (n_new - 1));
        int tok = tokens[(long)(s % ng) * n_new + j];
        if (tok < 0 || tok >= V) { if (d == 0 && err_flag) __hip_atomic_store(err_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); tok = 0; }
        ((T*)h)[((long)s * Ts + Tv + j) * D + d] = ((const T*)emb)[(long)tok * D + d];
    }
}
extern "C" void car_launch_score_embed(int mode, const void* emb, const int* tokens, void* h, int nseq, int ng, int n_new, int Ts, int Tv, int D, int V, int* err_flag, hipStream_t st) {
    const long total = (long)nseq * (n_new - 1) * D; if (total <= 0) return;
    int g = (int)((total + 255) / 256); if (g > 4096) g = 4096;
    if (mode == 1) hipLaunchKernelGGL(score_embed_kernel<bf16_t>, dim3(g), dim3(256), 0, st, emb, tokens, h, nseq, ng, n_new, Ts, Tv, D, V, err_flag);
    else hipLaunchKernelGGL(score_embed_kernel<float>, dim3(g), dim3(256), 0, st, emb, tokens, h, nseq, ng, n_new, Ts, Tv, D, V, err_flag);
}

// RoPE on q, k of qkv [b * Tn, 3 * dim] in place; row t of a sequence is position t0 + t.  The arithmetic of prefill_rope_kv_kernel (decode.hip) without its
// cache writes: car_score keeps no KV cache.
template <typename T>
__global__ void score_rope_kernel(void* qkv_, const float* rope, int b, int Tn, int H, int dim, int t0) {
    const long total = (long)b * Tn * H * 32;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        const int pr = (int)(i % 32); const int h = (int)((i / 32) % H); const int t = (int)((i / (32L * H)) % Tn); const long bb = i / (32L * H * Tn);
        T* row = (T*)qkv_ + (bb * Tn + t) * 3 * dim;
        const float cs = rope[((long)(t + t0) * 32 + pr) * 2], sn = rope[((long)(t + t0) * 32 + pr) * 2 + 1];
        const float q0 = ET<T>::ld(row + h * 64 + 2 * pr), q1 = ET<T>::ld(row + h * 64 + 2 * pr + 1);
        const float k0 = ET<T>::ld(row + dim + h * 64 + 2 * pr), k1 = ET<T>::ld(row + dim + h * 64 + 2 * pr + 1);
        ET<T>::st(row + h * 64 + 2 * pr, q0 * cs - q1 * sn); ET<T>::st(row + h * 64 + 2 * pr + 1, q1 * cs + q0 * sn);
        ET<T>::st(row + dim + h * 64 + 2 * pr, k0 * cs - k1 * sn); ET<T>::st(row + dim + h * 64 + 2 * pr + 1, k1 * cs + k0 * sn);
    }
}
extern "C" void car_launch_score_rope(int mode, void* qkv, const float* rope, int b, int Tn, int H, int dim, int t0, hipStream_t st) {
    const long total = (long)b * Tn * H * 32; int g = (int)((total + 255) / 256); if (g > 4096) g = 4096;
    if (mode == 1) hipLaunchKernelGGL(score_rope_kernel<bf16_t>, dim3(g), dim3(256), 0, st, qkv, rope, b, Tn, H, dim, t0);
    else hipLaunchKernelGGL(score_rope_kernel<float>, dim3(g), dim3(256), 0, st, qkv, rope, b, Tn, H, dim, t0);
}

// out[s][i] for the chunk's sequences: the text-pad mask of image img0 + s % ng over the window columns [t0, t0 + Tv) (all ones without a mask), ones over the
// image rows — the pad rule stays folded into the causal mask (generate.py:184-193)
__global__ void score_mask_kernel(const int64_t* emb_mask, unsigned char* out, int nseq, int ng, int img0, int T, int t0, int Tv, int Ts) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)nseq * Ts) return;
    const int s = (int)(i / Ts), c = (int)(i - (long)s * Ts);
    out[i] = (c < Tv && emb_mask) ? (unsigned char)(emb_mask[(long)(img0 + s % ng) * T + t0 + c] != 0) : (unsigned char)1;
}
extern "C" void car_launch_score_mask(const int64_t* emb_mask, unsigned char* out, int nseq, int ng, int img0, int T, int t0, int Tv, int Ts, hipStream_t st) {
    const long n = (long)nseq * Ts;
    hipLaunchKernelGGL(score_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, emb_mask, out, nseq, ng, img0, T, t0, Tv, Ts);
}
