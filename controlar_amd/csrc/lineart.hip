// lineart.hip — the LineArt control extractor (condition/lineart.py:26-86: LineArt.forward, n_residual_blocks = 3, sigmoid) on the GPU.
// Activations are NHWC in the context's element type T (bf16_t fast / float exact); every convolution in front of an InstanceNorm keeps its raw
// fp32 accumulators until they are normalised (LineArt section).
//   la_to_nhwc     fp32 NCHW photo (raw 0..255 values) -> T NHWC
//   la_conv        implicit GEMM, 64 pixels x 64 channels per block, 4 waves x (16 x 64) on the MFMA step of conv_tile.h, around a single-stage loop.
//                  The A tile is gathered into LDS k-chunk by k-chunk through the tap table of LaConvP: reflection is an index map of that gather,
//                  zero padding a zero fill, stride 2 and the four parity phases of a transposed convolution are (stride, os, py, px).  The epilogue
//                  stores the fp32 tile and its per-channel (mean, M2) over the tile's valid rows — tiles never cross an image.
//   la_fold        per (image, channel): the tile partials combined with Chan's update in a fixed order (lane-strided, then a shuffle tree) -> mean, rstd
//   la_norm        (x - mean) * rstd, optional ReLU, optional skip add -> T
//   la_out7        reflection pad 3 + 7x7 conv 64 -> 1 as a per-pixel reduction (one wave per pixel, lane = channel) + bias + sigmoid, and the control
//                  tensor 1 - 2y on three channels (sample_t2i.py:131-132,141)
// No atomics anywhere: two calls give the same bits, and image i alone gives the bits of image i in a batch.
#include "car_common.h"
#include "kernel_params.h"
#include "conv_tile.h"

template <typename T>
__global__ void la_to_nhwc_kernel(const float* __restrict__ img, T* __restrict__ out, long HW, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x; const long st = (long)gridDim.x * blockDim.x;
    for (; i < n; i += st) {                         // i = (b*HW + p)*3 + c
        const long bp = i / 3; const int c = (int)(i - bp * 3); const long b = bp / HW, p = bp - b * HW;
        ET<T>::st(out + i, img[(b * 3 + c) * HW + p]);
    }
}

__device__ __forceinline__ int la_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

template <typename T>
__global__ __launch_bounds__(256) void la_conv_kernel(const LaConvP p) {
    constexpr int LD = ConvT<T>::LD, NV = 64 * (32 / ConvT<T>::VE) / 256;
    __shared__ __attribute__((aligned(16))) T As[64 * LD];
    __shared__ __attribute__((aligned(16))) T Bs[64 * LD];
    __shared__ __attribute__((aligned(16))) float Cs[64 * CONV_CLD];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int img = blockIdx.z, tile = blockIdx.x, n0 = blockIdx.y * 64;
    const int Mg = p.Hg * p.Wg, m0 = tile * 64;
    const T* __restrict__ in = (const T*)p.in + (long)img * p.in_img;
    const T* __restrict__ w = (const T*)p.w + (long)n0 * p.Kp;
    int rrow[NV], rko[NV], rgy[NV], rgx[NV]; bool rok[NV];
    conv_rows<T, NV>(tid, m0, Mg, p.Wg, rrow, rko, rgy, rgx, rok);
    f32x4 acc[1][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool fast = (p.Cin & 31) == 0;
    // register staging: the global loads of chunk k+1 are issued before the MFMAs of chunk k
    uint4 ra[NV], rb[NV];
    auto load_a = [&](int k0) {                     // a 32-wide k chunk lies inside one tap (Cin % 32 == 0): one 16-B vector per (row, k-slice)
        const int tap = k0 / p.Cin, c0 = k0 - tap * p.Cin;
        const int dy = p.dy[tap], dx = p.dx[tap];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            ra[v] = make_uint4(0u, 0u, 0u, 0u);
            if (rok[v]) {
                int iy = rgy[v] * p.stride + dy, ix = rgx[v] * p.stride + dx;
                if (p.reflect) { iy = la_reflect(iy, p.Hi); ix = la_reflect(ix, p.Wi); }
                if (iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi) ra[v] = *(const uint4*)(in + ((long)iy * p.Wi + ix) * p.Cin + c0 + rko[v]);
            }
        }
    };
    auto load_b = [&](int k0) {
#pragma unroll
        for (int v = 0; v < NV; ++v) rb[v] = *(const uint4*)(w + (long)rrow[v] * p.Kp + k0 + rko[v]);
    };
    if (fast) load_a(0);
    load_b(0);
    for (int k0 = 0; k0 < p.Kp; k0 += 32) {
        if (fast) {
#pragma unroll
            for (int v = 0; v < NV; ++v) *(uint4*)&As[rrow[v] * LD + rko[v]] = ra[v];
        } else {                                      // Cin = 3 (model0): element-wise gather, k = tap*Cin + ci, zero beyond K
            for (int e = tid; e < 64 * 32; e += 256) {
                const int row = e >> 5, kk = e & 31, k = k0 + kk, m = m0 + row;
                T val = (T)0;
                if (k < p.K && m < Mg) {
                    const int tap = k / p.Cin, ci = k - tap * p.Cin, gy = m / p.Wg, gx = m - gy * p.Wg;
                    int iy = gy * p.stride + p.dy[tap], ix = gx * p.stride + p.dx[tap];
                    if (p.reflect) { iy = la_reflect(iy, p.Hi); ix = la_reflect(ix, p.Wi); }
                    if (iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi) val = in[((long)iy * p.Wi + ix) * p.Cin + ci];
                }
                As[row * LD + kk] = val;
            }
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) *(uint4*)&Bs[rrow[v] * LD + rko[v]] = rb[v];
        __syncthreads();
        if (k0 + 32 < p.Kp) { if (fast) load_a(k0 + 32); load_b(k0 + 32); }
        conv_mfma_step<T, 1>(As + (16 * wv + (lane & 15)) * LD, Bs + (lane & 15) * LD, lane, acc);
        __syncthreads();
    }
    conv_spill<1>(Cs, 16 * wv, lane, acc);
    __syncthreads();
    const int rows = Mg - m0 < 64 ? Mg - m0 : 64;
    float* __restrict__ raw = p.raw + (long)img * p.raw_img;
    for (int i = tid; i < 64 * 16; i += 256) {
        const int row = i >> 4, c4 = (i & 15) * 4;
        if (row < rows) {
            const int m = m0 + row, gy = m / p.Wg, gx = m - gy * p.Wg;
            const long o = ((long)(gy * p.os + p.py) * p.Wout + (gx * p.os + p.px)) * p.N + n0 + c4;
            *(float4*)&raw[o] = *(const float4*)&Cs[row * CONV_CLD + c4];
        }
    }
    if (tid < 64) {                                   // (mean, M2) of this tile's column, two passes over the fp32 tile, fixed order
        float s = 0.f;
        for (int r = 0; r < rows; ++r) s += Cs[r * CONV_CLD + tid];
        const float mean = s / (float)rows;
        float m2 = 0.f;
        for (int r = 0; r < rows; ++r) { const float d = Cs[r * CONV_CLD + tid] - mean; m2 += d * d; }
        const long slot = (long)img * p.tiles_img + p.tile0 + tile;
        ((float2*)p.part)[slot * p.N + n0 + tid] = make_float2(mean, m2);
        if (tid == 0 && blockIdx.y == 0) p.cnt[slot] = rows;
    }
}

// Chan et al.: (n, mean, M2) of the union of two sets
__device__ __forceinline__ void la_combine(float& n, float& mean, float& m2, float nb, float mb, float qb) {
    if (nb > 0.f) {
        if (n == 0.f) { n = nb; mean = mb; m2 = qb; }
        else { const float t = n + nb, d = mb - mean; mean += d * (nb / t); m2 += qb + d * d * (n * nb / t); n = t; }
    }
}
__global__ __launch_bounds__(64) void la_fold_kernel(const float2* __restrict__ part, const int* __restrict__ cnt, float2* __restrict__ stats, int tiles_img, int N, float eps) {
    const int n = blockIdx.x, img = blockIdx.y, lane = threadIdx.x;
    float cn = 0.f, mean = 0.f, m2 = 0.f;
    for (int t = lane; t < tiles_img; t += 64) {
        const long slot = (long)img * tiles_img + t;
        const float2 pb = part[slot * N + n];
        la_combine(cn, mean, m2, (float)cnt[slot], pb.x, pb.y);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float nb = __shfl_down(cn, o, 64); const float mb = __shfl_down(mean, o, 64), qb = __shfl_down(m2, o, 64);
        if (lane + o >= 64) nb = 0.f;
        la_combine(cn, mean, m2, nb, mb, qb);
    }
    if (lane == 0) stats[(long)img * N + n] = make_float2(mean, 1.0f / sqrtf(m2 / cn + eps));      // biased variance (nn.InstanceNorm2d)
}

template <typename T>
__global__ void la_norm_kernel(const float* __restrict__ raw, const float2* __restrict__ stats, const T* __restrict__ skip, T* __restrict__ out,
                               long n_img, long raw_img, long act_img, int N, int relu) {
    const int img = blockIdx.y;
    const float* r = raw + (long)img * raw_img; const float2* st = stats + (long)img * N;
    const T* sk = skip ? skip + (long)img * act_img : nullptr; T* o = out + (long)img * act_img;
    long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; const long step = (long)gridDim.x * blockDim.x * 4;
    for (; i < n_img; i += step) {                   // N % 4 == 0: the four values are channels c .. c+3 of one pixel
        const int c = (int)(i % N);
        const float4 x = *(const float4*)&r[i];
        const float xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float2 s = st[c + e];
            float v = (xv[e] - s.x) * s.y;
            if (relu) v = fmaxf(v, 0.f);
            if (sk) v += ET<T>::ld(sk + i + e);
            ET<T>::st(o + i + e, v);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void la_out7_kernel(const T* __restrict__ in, const T* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out,
                                                      T* __restrict__ control, int H, int W, long act_img) {
    __shared__ float ws[49 * 64];
    for (int i = threadIdx.x; i < 49 * 64; i += 256) ws[i] = ET<T>::ld(w + i);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, img = blockIdx.y;
    const T* x = in + (long)img * act_img;
    const long P = (long)H * W;
    const float b0 = bias[0];
    for (long pix = (long)blockIdx.x * 4 + wv; pix < P; pix += (long)gridDim.x * 4) {
        const int y = (int)(pix / W), xx = (int)(pix - (long)y * W);
        float acc = 0.f;
        for (int ky = 0; ky < 7; ++ky) {
            const int iy = la_reflect(y + ky - 3, H);
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const int ix = la_reflect(xx + kx - 3, W);
                acc += ET<T>::ld(x + ((long)iy * W + ix) * 64 + lane) * ws[(ky * 7 + kx) * 64 + lane];
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) {
            const float v = 1.0f / (1.0f + expf(-(acc + b0)));
            if (out) out[(long)img * P + pix] = v;
            if (control) {
                const float cv = 1.0f - 2.0f * v;     // 1 - y, *255, 2*(x/255 - 0.5)
                T* c = control + (long)img * 3 * P + pix;
                ET<T>::st(c, cv); ET<T>::st(c + P, cv); ET<T>::st(c + 2 * P, cv);
            }
        }
    }
}

// ------------------------------------------------------------------------------------- launchers: every one returns the launch status
extern "C" int car_launch_la_to_nhwc(int mode, const float* img, void* out, int B, long HW, hipStream_t st) {
    const long n = (long)B * HW * 3; int g = (int)((n + 255) / 256); if (g > 8192) g = 8192;
    if (mode == 1) hipLaunchKernelGGL(la_to_nhwc_kernel<bf16_t>, dim3(g), dim3(256), 0, st, img, (bf16_t*)out, HW, n);
    else hipLaunchKernelGGL(la_to_nhwc_kernel<float>, dim3(g), dim3(256), 0, st, img, (float*)out, HW, n);
    return (int)hipGetLastError();
}
extern "C" int car_launch_la_conv(int mode, const LaConvP* p, int nimg, hipStream_t st) {
    const int tiles = (p->Hg * p->Wg + 63) / 64;
    if (p->N % 64 || p->Kp % 32 || p->ntaps > 49 || tiles <= 0 || nimg <= 0 || nimg > 65535) return (int)hipErrorInvalidValue;
    const dim3 grid(tiles, p->N / 64, nimg);
    if (mode == 1) hipLaunchKernelGGL(la_conv_kernel<bf16_t>, grid, dim3(256), 0, st, *p);
    else hipLaunchKernelGGL(la_conv_kernel<float>, grid, dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int car_launch_la_fold(const float* part, const int* cnt, float* stats, int tiles_img, int N, int nimg, float eps, hipStream_t st) {
    hipLaunchKernelGGL(la_fold_kernel, dim3(N, nimg), dim3(64), 0, st, (const float2*)part, cnt, (float2*)stats, tiles_img, N, eps);
    return (int)hipGetLastError();
}
extern "C" int car_launch_la_norm(int mode, const float* raw, const float* stats, const void* skip, void* out, long n_img, long raw_img, long act_img,
                                  int N, int relu, int nimg, hipStream_t st) {
    int g = (int)((n_img / 4 + 255) / 256); if (g > 4096) g = 4096; if (g < 1) g = 1;
    if (mode == 1) hipLaunchKernelGGL(la_norm_kernel<bf16_t>, dim3(g, nimg), dim3(256), 0, st, raw, (const float2*)stats, (const bf16_t*)skip, (bf16_t*)out, n_img, raw_img, act_img, N, relu);
    else hipLaunchKernelGGL(la_norm_kernel<float>, dim3(g, nimg), dim3(256), 0, st, raw, (const float2*)stats, (const float*)skip, (float*)out, n_img, raw_img, act_img, N, relu);
    return (int)hipGetLastError();
}
extern "C" int car_launch_la_out7(int mode, const void* in, const void* w, const float* bias, float* out, void* control, int H, int W, long act_img, int nimg, hipStream_t st) {
    const long P = (long)H * W; int g = (int)((P + 3) / 4); if (g > 2048) g = 2048;
    if (mode == 1) hipLaunchKernelGGL(la_out7_kernel<bf16_t>, dim3(g, nimg), dim3(256), 0, st, (const bf16_t*)in, (const bf16_t*)w, bias, out, (bf16_t*)control, H, W, act_img);
    else hipLaunchKernelGGL(la_out7_kernel<float>, dim3(g, nimg), dim3(256), 0, st, (const float*)in, (const float*)w, bias, out, (float*)control, H, W, act_img);
    return (int)hipGetLastError();
}
