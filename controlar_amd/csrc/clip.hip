// clip.hip — kernels specific to the CLIP score (evaluations/t2i/evaluation.py:129-176: compute_clip_score).  The two towers themselves are GEMMs, LayerNorm
// and attention from gemm.hip / ops.hip / attn.hip (car_clip_encode_image / car_clip_encode_text in engine_clip.hip; quick-GELU is ACT_QUICK_GELU of the
// shared GEMM epilogue); what is CLIP-only lives here:
//   clip_requant            the script's ToTensor / Normalize(0.5, 0.5) / tensor2pil round trip of an 8-bit image as a 256-entry table (built on the host)
//   clip_pixels_to_patches  centre crop by offset, u/255, (x - mean)/std — each step rounded to fp32 once — written straight into the patch matrix of
//                           the bias-free patch convolution (columns (c, py, px)), and optionally as pixel_values
//   clip_text_embed         token_embedding[id] + position_embedding[t]; an id outside [0, vocab) reads row 0 and raises the sticky flag
//   clip_pool               per sequence the row at the first position of the largest id (text) or row 0 (vision): LayerNorm and projection then run on B rows
//   clip_cosine / clip_mean F.cosine_similarity(dim=1, eps) in fp32, one wave per pair; the fp64 mean of the first n scores in one block, no atomics
#include "car_common.h"
#include "kernel_params.h"
#include <string.h>

#define LAUNCH_T(mode, KERNEL, grid, block, st, ...)                                          \
    do {                                                                                      \
        if ((mode) == 1) hipLaunchKernelGGL((KERNEL<bf16_t>), grid, block, 0, st, __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<float>), grid, block, 0, st, __VA_ARGS__);            \
    } while (0)

// dst[i] = table[src[i]], four bytes per thread (dst == src is allowed).  The 256-entry table travels in the kernel arguments.  VEC: both pointers are
// 4-byte aligned.
struct ClipRequantTab { unsigned char t[256]; };
template <bool VEC>
__global__ __launch_bounds__(256) void clip_requant_kernel(const unsigned char* src, unsigned char* dst, ClipRequantTab table, long n) {
    __shared__ unsigned char tab[256];
    tab[threadIdx.x] = table.t[threadIdx.x];
    __syncthreads();
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (VEC && i + 4 <= n) {
        const unsigned v = *(const unsigned*)(src + i);
        *(unsigned*)(dst + i) = (unsigned)tab[v & 255] | ((unsigned)tab[(v >> 8) & 255] << 8) | ((unsigned)tab[(v >> 16) & 255] << 16) | ((unsigned)tab[v >> 24] << 24);
        return;
    }
    for (long j = i; j < i + 4 && j < n; ++j) dst[j] = tab[src[j]];
}
// `host_table`: 256 bytes on the host
extern "C" void car_launch_clip_requant(const unsigned char* src, unsigned char* dst, const unsigned char* host_table, long n, hipStream_t st) {
    ClipRequantTab t; memcpy(t.t, host_table, 256);
    const dim3 g((unsigned)((n + 1023) / 1024));
    if ((((uintptr_t)src | (uintptr_t)dst) & 3) == 0) hipLaunchKernelGGL(clip_requant_kernel<true>, g, dim3(256), 0, st, src, dst, t, n);
    else hipLaunchKernelGGL(clip_requant_kernel<false>, g, dim3(256), 0, st, src, dst, t, n);
}

// One thread per value of the cropped image, x fastest: the stores to the patch matrix and to pixel_values run along px / x.
template <typename T>
__global__ __launch_bounds__(256) void clip_pixels_to_patches_kernel(ClipPatchP p) {
    const int n = p.n_px, pp = p.patch * p.patch;
    const long total = (long)p.B * 3 * n * n;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int x = (int)(i % n), y = (int)((i / n) % n), c = (int)((i / ((long)n * n)) % 3); const long b = i / ((long)3 * n * n);
        const unsigned char u = p.src[((b * p.Hr + p.top + y) * p.Wr + p.left + x) * 3 + c];
        // ToTensor: u / 255; Normalize: (x - mean) / std.  The intrinsics keep every step a single fp32 rounding (no contraction, IEEE division).
        const float v = __fdiv_rn(__fsub_rn(__fdiv_rn((float)u, 255.0f), p.mean[c]), p.std[c]);
        if (p.pixel_values) p.pixel_values[i] = v;
        const int gy = y / p.patch, py = y - gy * p.patch, gx = x / p.patch, px = x - gx * p.patch;
        ET<T>::st((T*)p.patches + ((b * p.g + gy) * p.g + gx) * p.Kp + c * pp + py * p.patch + px, v);
    }
    const int pad = p.Kp - 3 * pp;
    if (pad > 0) {
        const long rows = (long)p.B * p.g * p.g;
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < rows * pad; i += stride)
            ET<T>::st((T*)p.patches + (i / pad) * p.Kp + 3 * pp + (int)(i % pad), 0.f);
    }
}
extern "C" void car_launch_clip_pixels_to_patches(int mode, const ClipPatchP* p, hipStream_t st) {
    const long total = (long)p->B * 3 * p->n_px * p->n_px;
    int g = (int)((total + 255) / 256); if (g > 8192) g = 8192; if (g < 1) g = 1;
    LAUNCH_T(mode, clip_pixels_to_patches_kernel, dim3(g), dim3(256), st, *p);
}

// h[b, t] = token_embedding[ids[b, t]] + position_embedding[t]   (CLIPTextEmbeddings.forward)
template <typename T>
__global__ __launch_bounds__(256) void clip_text_embed_kernel(const long long* ids, const void* tok_, const void* pos_, void* h_, long B, int Tn, int D, int vocab, int* err_flag) {
    const long total = B * Tn * D;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int d = (int)(i % D); const long r = i / D; const int t = (int)(r % Tn);
        long long id = ids[r];
        if (id < 0 || id >= vocab) { if (d == 0 && err_flag) __hip_atomic_store(err_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); id = 0; }   // host-mapped sticky flag (check_sticky)
        ET<T>::st((T*)h_ + i, ET<T>::ld((const T*)tok_ + id * D + d) + ET<T>::ld((const T*)pos_ + (long)t * D + d));
    }
}
extern "C" void car_launch_clip_text_embed(int mode, const long long* ids, const void* tok, const void* pos, void* h, long B, int T, int D, int vocab, int* err_flag, hipStream_t st) {
    const long total = B * T * D;
    int g = (int)((total + 255) / 256); if (g > 4096) g = 4096; if (g < 1) g = 1;
    LAUNCH_T(mode, clip_text_embed_kernel, dim3(g), dim3(256), st, ids, tok, pos, h, B, T, D, vocab, err_flag);
}

// out[b] = h[b, j]: j = the first position of the largest id of sequence b (ids.argmax(dim=-1); an id outside [0, vocab) counts as 0, as the embedding
// read it), or 0 when ids is NULL (the class row of the vision tower).  One block per sequence; every wave finds j for itself (the same value).
template <typename T>
__global__ __launch_bounds__(256) void clip_pool_kernel(const void* h_, const long long* ids, void* out_, int Tn, int D, int vocab) {
    const long b = blockIdx.x;
    int j = 0;
    if (ids) {
        const int lane = threadIdx.x & 63;
        long long best = -1; int at = 0x7fffffff;
        for (int t = lane; t < Tn; t += 64) {
            long long id = ids[b * Tn + t]; if (id < 0 || id >= vocab) id = 0;
            if (id > best) { best = id; at = t; }          // t ascends within a lane: the first position of the lane's maximum
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const long long ob = __shfl_xor(best, o, 64); const int oa = __shfl_xor(at, o, 64);
            if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
        }
        j = at;
    }
    const T* src = (const T*)h_ + (b * Tn + j) * D; T* dst = (T*)out_ + b * D;
    for (int d = threadIdx.x; d < D; d += blockDim.x) dst[d] = src[d];
}
extern "C" void car_launch_clip_pool(int mode, const void* h, const long long* ids, void* out, int B, int T, int D, int vocab, hipStream_t st) {
    LAUNCH_T(mode, clip_pool_kernel, dim3(B), dim3(256), st, h, ids, out, T, D, vocab);
}

// ATen's cosine_similarity: x / max(||x||, eps) for both vectors, then the dot product.  One wave per pair: a lane sums its elements d = lane, lane + 64,
// ... in order, then the xor butterfly of wave_sum (fixed).
__global__ __launch_bounds__(256) void clip_cosine_kernel(const float* a_, const float* b_, int B, int D, float eps, float* out) {
    const int pair = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (pair >= B) return;
    const float* a = a_ + (long)pair * D; const float* b = b_ + (long)pair * D;
    float sa = 0.f, sb = 0.f;
    for (int d = lane; d < D; d += 64) { sa += a[d] * a[d]; sb += b[d] * b[d]; }
    const float na = fmaxf(sqrtf(wave_sum(sa)), eps), nb = fmaxf(sqrtf(wave_sum(sb)), eps);
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += __fdiv_rn(a[d], na) * __fdiv_rn(b[d], nb);
    s = wave_sum(s);
    if (lane == 0) out[pair] = s;
}
extern "C" void car_launch_clip_cosine(const float* a, const float* b, int B, int D, float eps, float* out, hipStream_t st) {
    hipLaunchKernelGGL(clip_cosine_kernel, dim3((B + 3) / 4), dim3(256), 0, st, a, b, B, D, eps, out);
}

// out[0] = mean(v[0 .. n)) in fp64: thread t sums v[t], v[t + 256], ... in order, then a fixed tree over the 256 partials in LDS.  One block.
__global__ __launch_bounds__(256) void clip_mean_kernel(const float* v, int n, double* out) {
    __shared__ double sm[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)v[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sm[0] / (double)n;
}
extern "C" void car_launch_clip_mean(const float* v, int n, double* out, hipStream_t st) {
    hipLaunchKernelGGL(clip_mean_kernel, dim3(1), dim3(256), 0, st, v, n, out);
}
