// lpips.hip — what judges a VQ reconstruction, on the GPU: the parts of LPIPS (tokenizer/tokenizer_image/lpips.py:83-164) around its VGG-16 trunk, and the
// PSNR and pixel quantiser of the tokenizer evaluation (tokenizer/tokenizer_image/reconstruction_vq_ddp.py:128-155).  The trunk itself is hed.hip's
// hed_conv (the same thirteen 3x3 convolutions, ReLU and fused 2x2 max-pools as ControlNetHED_Apache2), launched by engine_lpips.hip.
//   lpips_to_nhwc   fp32 NCHW image in [-1,1] -> (x - shift[c]) / scale[c] -> T NHWC (ScalingLayer, lpips.py:99-106): a subtraction and a true division,
//                   each rounded to fp32 once.
//   lpips_head      one tap of a chunk of pairs.  C / 8 lanes own one pixel: each holds 8 channels of both images in registers, pass 1 reduces the two
//                   squared norms over the group, pass 2 the weighted squared difference of the normalised features — the difference itself, never
//                   its expansion into three sums, which cancels on nearly equal images — and the group's first lane adds the pixel's value to an
//                   fp64 sum.  Wave shuffle, then LDS: one fp64 partial per workgroup.  fp32 arithmetic per pixel in both modes.
//   lpips_fold      per pair and layer: the partials in index order, the mean over H x W, then the five layers in the order 0..4 (lpips.py:92-96).
//   psnr_sq / psnr_fold   10 log10(data_range^2 / mse), mse the fp64 mean of (a - b)^2 (skimage.metrics.peak_signal_noise_ratio).
//   recon_to_u8     clamp(127.5 x + 128, 0, 255) truncated (reconstruction_vq_ddp.py:144): a product and a sum, each rounded to fp32.
// No atomics anywhere, no workgroup crosses a pair: two calls give the same bits, and pair i alone gives the bits of pair i in a batch.
#include "car_common.h"
#include "lpips_params.h"

// Every product and sum written with an operator below is rounded on its own, as torch rounds its element-wise ops; fmaf is fused where it is written out.
// Under the compiler's default contraction 127.5 x + 128 became one fused multiply-add — also through __fmul_rn / __fadd_rn, whose bodies are compiled
// under that default — which is not the script's quantiser at a bucket edge.
#pragma clang fp contract(off)

__device__ inline double lp_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// block-wide sum for 256 threads; `sm` has 4 doubles.  Fixed order: deterministic.
__device__ inline double lp_block_sum_d(double v, double* sm) {
    v = lp_wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

// grid (blocks, images): image i of `img` (3 planes of HW) -> out + i * out_img
template <typename T>
__global__ __launch_bounds__(256) void lpips_to_nhwc_kernel(const float* __restrict__ img, T* __restrict__ out, long out_img, long HW, float3 shift, float3 scale) {
    const float* src = img + (size_t)blockIdx.y * 3 * HW;
    T* dst = out + (size_t)blockIdx.y * out_img;
    const long n = HW * 3, st = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += st) {          // i = p*3 + c
        const long p = i / 3; const int c = (int)(i - p * 3);
        const float sh = c == 0 ? shift.x : c == 1 ? shift.y : shift.z, sc = c == 0 ? scale.x : c == 1 ? scale.y : scale.z;
        ET<T>::st(dst + i, __fdiv_rn(src[c * HW + p] - sh, sc));
    }
}

// 8 consecutive channels as fp32; p is 16-byte (bf16) or 32-byte (fp32) aligned: maps are 256-byte aligned and C is a multiple of 64
template <typename T> __device__ __forceinline__ void lp_ld8(const T* p, float v[8]);
template <> __device__ __forceinline__ void lp_ld8<float>(const float* p, float v[8]) {
    const float4 x = *(const float4*)p, y = *(const float4*)(p + 4);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; v[4] = y.x; v[5] = y.y; v[6] = y.z; v[7] = y.w;
}
template <> __device__ __forceinline__ void lp_ld8<bf16_t>(const bf16_t* p, float v[8]) {
    const uint4 x = *(const uint4*)p;
    const unsigned w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
}

// sum over the G lanes of a pixel's group (G a power of two <= 64, groups aligned): every lane of the group ends with the same bits
template <int G> __device__ __forceinline__ float lp_group_sum(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// grid (nblk, pairs); G = C / 8
template <typename T, int G>
__global__ __launch_bounds__(256) void lpips_head_kernel(const LpipsHeadP p) {
    __shared__ double sm[4];
    constexpr int NG = 256 / G, C = 8 * G;
    const int tid = threadIdx.x, g = tid / G, j = tid % G;
    const T* __restrict__ a = (const T*)p.act + (size_t)(2 * blockIdx.y) * p.img + j * 8;
    const T* __restrict__ b = a + p.img;
    float w[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = p.lin[j * 8 + e];
    const long p0 = (long)blockIdx.x * (LP_PASSES * NG);
    double acc = 0.0;
#pragma unroll 2
    for (int pass = 0; pass < LP_PASSES; ++pass) {             // uniform trip count: every lane takes part in the shuffles
        const long pix = p0 + (long)pass * NG + g;
        const bool ok = pix < p.P;
        float va[8] = {}, vb[8] = {};
        if (ok) { lp_ld8<T>(a + pix * C, va); lp_ld8<T>(b + pix * C, vb); }
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { sa = fmaf(va[e], va[e], sa); sb = fmaf(vb[e], vb[e], sb); }
        sa = lp_group_sum<G>(sa); sb = lp_group_sum<G>(sb);
        const float da = __fsqrt_rn(sa) + 1e-10f, db = __fsqrt_rn(sb) + 1e-10f;      // the eps outside the root (lpips.py:159-160)
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d = __fdiv_rn(va[e], da) - __fdiv_rn(vb[e], db);
            s = fmaf(w[e], d * d, s);
        }
        s = lp_group_sum<G>(s);
        if (ok && j == 0) acc += (double)s;
    }
    acc = lp_block_sum_d(acc, sm);
    if (tid == 0) p.part[(size_t)blockIdx.y * p.nblk + blockIdx.x] = acc;
}

// one thread per pair
__global__ __launch_bounds__(64) void lpips_fold_kernel(const LpipsFoldP p) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= p.npairs) return;
    double val = 0.0;
#pragma unroll
    for (int l = 0; l < LP_LAYERS; ++l) {
        const double* q = p.part[l] + (size_t)i * p.nblk[l];
        double s = 0.0;
        for (int k = 0; k < p.nblk[l]; ++k) s += q[k];
        s /= p.count[l];
        if (p.layers) p.layers[(size_t)i * LP_LAYERS + l] = s;
        val = l ? val + s : s;
    }
    p.out[i] = val;
}

// ------------------------------------------------------------------------------------- PSNR
__device__ inline float lp_elem(const void* p, int u8, int map, size_t i) {
    const float v = u8 ? (float)((const unsigned char*)p)[i] : ((const float*)p)[i];
    return map == LP_MAP_DIV255 ? __fdiv_rn(v, 255.0f) : map == LP_MAP_HALF ? __fdiv_rn(v + 1.0f, 2.0f) : v;
}
// grid (chunks, B): fp64 sum of (a - b)^2 over a chunk of one image's n elements: psum [B][chunks]
__global__ __launch_bounds__(256) void psnr_sq_kernel(const void* a, int u8_a, int map_a, const void* b, int u8_b, int map_b, long n, long chunk, double* psum) {
    __shared__ double sm[4];
    const size_t base = (size_t)blockIdx.y * n;
    const long i0 = (long)blockIdx.x * chunk, i1 = i0 + chunk < n ? i0 + chunk : n;
    double acc = 0.0;
    for (long i = i0 + threadIdx.x; i < i1; i += 256) {
        const double d = (double)lp_elem(a, u8_a, map_a, base + i) - (double)lp_elem(b, u8_b, map_b, base + i);
        acc += d * d;
    }
    acc = lp_block_sum_d(acc, sm);
    if (threadIdx.x == 0) psum[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}
__global__ __launch_bounds__(64) void psnr_fold_kernel(const double* psum, int chunks, long n, double data_range, double* out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double v = 0.0;
    for (int i = lane; i < chunks; i += 64) v += psum[(size_t)b * chunks + i];
    v = lp_wave_sum_d(v);
    if (lane == 0) {
        const double mse = v / (double)n;
        out[b] = mse == 0.0 ? (double)INFINITY : 10.0 * log10(data_range * data_range / mse);
    }
}

// ------------------------------------------------------------------------------------- the tokenizer script's quantiser
__global__ __launch_bounds__(256) void recon_to_u8_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, long n) {
    const long st = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += st) {
        const float v = 127.5f * x[i] + 128.0f;
        out[i] = (unsigned char)fminf(fmaxf(v, 0.f), 255.f);
    }
}

// ------------------------------------------------------------------------------------- launchers: every one returns the launch status
extern "C" int car_launch_lpips_to_nhwc(int mode, const float* img, void* out, long out_img, long HW, int nimg, const float* shift, const float* scale, hipStream_t st) {
    if (nimg <= 0 || nimg > 65535 || HW <= 0) return (int)hipErrorInvalidValue;
    const long n = HW * 3; int g = (int)((n + 255) / 256); if (g > 1024) g = 1024;
    const float3 sh = make_float3(shift[0], shift[1], shift[2]), sc = make_float3(scale[0], scale[1], scale[2]);
    if (mode == 1) hipLaunchKernelGGL(lpips_to_nhwc_kernel<bf16_t>, dim3(g, nimg), dim3(256), 0, st, img, (bf16_t*)out, out_img, HW, sh, sc);
    else hipLaunchKernelGGL(lpips_to_nhwc_kernel<float>, dim3(g, nimg), dim3(256), 0, st, img, (float*)out, out_img, HW, sh, sc);
    return (int)hipGetLastError();
}
template <typename T> static void lp_head_launch(const LpipsHeadP* p, dim3 grid, hipStream_t st) {
    switch (p->C) {
        case 64: hipLaunchKernelGGL((lpips_head_kernel<T, 8>), grid, dim3(256), 0, st, *p); break;
        case 128: hipLaunchKernelGGL((lpips_head_kernel<T, 16>), grid, dim3(256), 0, st, *p); break;
        case 256: hipLaunchKernelGGL((lpips_head_kernel<T, 32>), grid, dim3(256), 0, st, *p); break;
        default: hipLaunchKernelGGL((lpips_head_kernel<T, 64>), grid, dim3(256), 0, st, *p); break;
    }
}
extern "C" int car_lpips_head_blocks(long P, int C) { const long per = 65536 / C; return (int)((P + per - 1) / per); }
extern "C" int car_launch_lpips_head(int mode, const LpipsHeadP* p, int npairs, hipStream_t st) {
    if ((p->C != 64 && p->C != 128 && p->C != 256 && p->C != 512) || p->P <= 0 || p->P > (1L << 26) || npairs <= 0 || npairs > 32767 ||
        p->nblk != car_lpips_head_blocks(p->P, p->C) || !p->act || !p->lin || !p->part || p->img < p->P * p->C) return (int)hipErrorInvalidValue;
    const dim3 grid(p->nblk, npairs);
    if (mode == 1) lp_head_launch<bf16_t>(p, grid, st); else lp_head_launch<float>(p, grid, st);
    return (int)hipGetLastError();
}
extern "C" int car_launch_lpips_fold(const LpipsFoldP* p, hipStream_t st) {
    if (p->npairs <= 0 || !p->out) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lpips_fold_kernel, dim3((p->npairs + 63) / 64), dim3(64), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int car_launch_psnr(const void* a, int u8_a, int map_a, const void* b, int u8_b, int map_b, int B, long n, long chunk, int chunks, double data_range,
                               double* psum, double* out, hipStream_t st) {
    hipLaunchKernelGGL(psnr_sq_kernel, dim3(chunks, B), dim3(256), 0, st, a, u8_a, map_a, b, u8_b, map_b, n, chunk, psum);
    hipLaunchKernelGGL(psnr_fold_kernel, dim3(B), dim3(64), 0, st, psum, chunks, n, data_range, out);
    return (int)hipGetLastError();
}
extern "C" int car_launch_recon_to_u8(const float* x, unsigned char* out, long n, hipStream_t st) {
    long g = (n + 255) / 256; if (g > 65536) g = 65536;
    hipLaunchKernelGGL(recon_to_u8_kernel, dim3((unsigned)g), dim3(256), 0, st, x, out, n);
    return (int)hipGetLastError();
}
