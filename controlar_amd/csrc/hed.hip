// hed.hip — the HED edge extractor (condition/hed.py:17-81: ControlNetHED_Apache2 + HEDdetector.__call__) on the GPU.
// Activations are NHWC in the context's element type T (bf16_t fast / float exact), accumulators fp32 (HED section).
//   hed_to_nhwc    fp32 NCHW image (raw 0..255 values) minus norm[c] -> T NHWC.  The subtraction lives here and nowhere else: the first conv pads
//                  the DIFFERENCE with zeros, so norm cannot move into that conv's bias.
//   hed_conv       3x3 / stride 1 / zero pad implicit GEMM on the shared tile loop (conv_tile.h: 128 pixels x 64 channels per block, two LDS stages).
//                  pool = 1 reads the input through a 2x2 / stride-2 max-pool in the gather (floor: an odd last row or column is never addressed).  The epilogue adds the bias, applies ReLU, stores T, and — in the last conv of a block — reduces the T-rounded
//                  64-channel slice against projection.weight into an fp32 partial per (channel block, pixel).
//   hed_fuse       per output pixel: the five side maps (partials summed in channel-block order + bias) up-sampled bilinearly as ATen does
//                  (align_corners = False), mean in stack order, sigmoid, x255, clamp; optional control tensor 2*(edge/255 - 0.5) on three channels.
// No atomics anywhere and no tile crosses an image: two calls give the same bits, and image i alone gives the bits of image i in a batch.
#include "car_common.h"
#include "kernel_params.h"
#include "conv_tile.h"

template <typename T>
__global__ void hed_to_nhwc_kernel(const float* __restrict__ img, const float* __restrict__ norm, T* __restrict__ out, long HW, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x; const long st = (long)gridDim.x * blockDim.x;
    for (; i < n; i += st) {                         // i = p*3 + c of one image
        const long p = i / 3; const int c = (int)(i - p * 3);
        ET<T>::st(out + i, img[c * HW + p] - norm[c]);
    }
}

// element-wise maximum of two 16-byte vectors of T
template <typename T> __device__ __forceinline__ uint4 hed_vmax(uint4 a, uint4 b);
template <> __device__ __forceinline__ uint4 hed_vmax<float>(uint4 a, uint4 b) {
    return make_uint4(__float_as_uint(fmaxf(__uint_as_float(a.x), __uint_as_float(b.x))), __float_as_uint(fmaxf(__uint_as_float(a.y), __uint_as_float(b.y))),
                      __float_as_uint(fmaxf(__uint_as_float(a.z), __uint_as_float(b.z))), __float_as_uint(fmaxf(__uint_as_float(a.w), __uint_as_float(b.w))));
}
__device__ __forceinline__ unsigned hed_max2bf(unsigned a, unsigned b) {          // two bf16 per word: a bf16 is the upper half of its fp32
    const float hi = fmaxf(__uint_as_float(a & 0xffff0000u), __uint_as_float(b & 0xffff0000u));
    const float lo = fmaxf(__uint_as_float(a << 16), __uint_as_float(b << 16));
    return (__float_as_uint(hi) & 0xffff0000u) | (__float_as_uint(lo) >> 16);
}
template <> __device__ __forceinline__ uint4 hed_vmax<bf16_t>(uint4 a, uint4 b) {
    return make_uint4(hed_max2bf(a.x, b.x), hed_max2bf(a.y, b.y), hed_max2bf(a.z, b.z), hed_max2bf(a.w, b.w));
}

// The A-tile gather of hed_conv (conv_tile.h): zero pad 1, optionally through the 2x2 / stride-2 max-pool, and the element-wise path of Cin = 3.
template <typename T>
struct HedGather {
    static constexpr bool HAS_FILL = true, PARTIAL_N = false;      // N % 64 == 0
    const HedConvP& p; const T* __restrict__ in;
    __device__ __forceinline__ int cin() const { return p.Cin; }
    __device__ __forceinline__ int stride() const { return 1; }
    __device__ __forceinline__ bool vectors() const { return (p.Cin & 31) == 0; }
    __device__ __forceinline__ bool inside(int iy, int ix) const { return iy >= 0 && iy < p.H && ix >= 0 && ix < p.W; }
    __device__ __forceinline__ uint4 vec(int iy, int ix, int c) const {
        if (p.pool) {                                 // (2iy+1, 2ix+1) <= (Hi-1, Wi-1) because H = Hi/2, W = Wi/2 (floor)
            const T* s = in + ((long)(2 * iy) * p.Wi + 2 * ix) * p.Cin + c;
            const uint4 t0 = *(const uint4*)s, t1 = *(const uint4*)(s + p.Cin);
            const uint4 t2 = *(const uint4*)(s + (long)p.Wi * p.Cin), t3 = *(const uint4*)(s + (long)p.Wi * p.Cin + p.Cin);
            return hed_vmax<T>(hed_vmax<T>(t0, t1), hed_vmax<T>(t2, t3));
        }
        return *(const uint4*)(in + ((long)iy * p.Wi + ix) * p.Cin + c);
    }
    __device__ __forceinline__ void fill(T* A, int k0, int m0, int M, int tid) const {       // Cin = 3 (block1.convs.0, never pooled): zero beyond K
        constexpr int LD = ConvT<T>::LD;
        for (int e = tid; e < 128 * 32; e += 256) {
            const int row = e >> 5, kk = e & 31, k = k0 + kk, m = m0 + row;
            T val = (T)0;
            if (k < p.K && m < M) {
                const int tap = k / p.Cin, ci = k - tap * p.Cin, gy = m / p.W, gx = m - gy * p.W;
                const int iy = gy + tap / 3 - 1, ix = gx + tap % 3 - 1;
                if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) val = in[((long)iy * p.Wi + ix) * p.Cin + ci];
            }
            A[row * LD + kk] = val;
        }
    }
};

template <typename T>
__global__ __launch_bounds__(256) void hed_conv_kernel(const HedConvP p) {
    __shared__ __attribute__((aligned(16))) char smem[ConvTile128<T>::SMEM_BYTES];
    const int tid = threadIdx.x;
    const int img = blockIdx.z, n0 = blockIdx.y * 64, m0 = blockIdx.x * 128;
    const int M = p.H * p.W;
    const HedGather<T> g{p, (const T*)p.in + (long)img * p.in_img};
    conv_tile_128x64<T>(smem, g, (const T*)p.w + (long)n0 * p.Kp, 64, p.Kp, m0, M, p.W);
    const float* const Cs = (const float*)smem;
    const int rows = M - m0 < 128 ? M - m0 : 128;
    T* __restrict__ out = (T*)p.out + (long)img * p.out_img;
    const T* __restrict__ proj = (const T*)p.proj;
    float* __restrict__ part = p.part ? p.part + (long)img * p.part_img + (long)blockIdx.y * M : nullptr;
#pragma unroll 2
    for (int it = 0; it < 8; ++it) {                  // 128 rows x 16 four-channel groups; the 16 groups of a row are 16 consecutive lanes
        const int idx = tid + it * 256, row = idx >> 4, c4 = (idx & 15) * 4;
        const bool ok = row < rows;
        const float4 x = *(const float4*)&Cs[row * CONV_CLD + c4];
        const float4 b = *(const float4*)&p.bias[n0 + c4];
        float v[4] = {x.x + b.x, x.y + b.y, x.z + b.z, x.w + b.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = ET<T>::rnd(v[e] > 0.f ? v[e] : 0.f);
        if (ok) conv_store4(out + (long)(m0 + row) * p.N + n0 + c4, v[0], v[1], v[2], v[3]);
        if (part) {                                   // uniform over the block: every lane takes part in the shuffles
            const float s = conv_proj16(v[0], v[1], v[2], v[3], proj + n0 + c4, ok);
            if (ok && (idx & 15) == 0) part[m0 + row] = s;
        }
    }
}

// one side map at (y, x) of the output grid: ATen's upsample_bilinear2d with align_corners = False
__device__ __forceinline__ float hed_side(const float* __restrict__ part, int nblk, float bias, int Hl, int Wl, int H, int W, int y, int x) {
    const float sh = (float)Hl / (float)H, sw = (float)Wl / (float)W;
    const float sy = fmaxf(sh * ((float)y + 0.5f) - 0.5f, 0.f), sx = fmaxf(sw * ((float)x + 0.5f) - 0.5f, 0.f);
    int y0 = (int)sy, x0 = (int)sx;
    y0 = y0 < Hl - 1 ? y0 : Hl - 1; x0 = x0 < Wl - 1 ? x0 : Wl - 1;
    const int y1 = y0 < Hl - 1 ? y0 + 1 : y0, x1 = x0 < Wl - 1 ? x0 + 1 : x0;
    const float ly1 = sy - (float)y0, ly0 = 1.f - ly1, lx1 = sx - (float)x0, lx0 = 1.f - lx1;
    const long P = (long)Hl * Wl;
    float v00 = 0.f, v01 = 0.f, v10 = 0.f, v11 = 0.f;
    for (int b = 0; b < nblk; ++b) {                  // channel blocks in index order: the sum is fixed by the shape
        const float* q = part + b * P;
        v00 += q[(long)y0 * Wl + x0]; v01 += q[(long)y0 * Wl + x1]; v10 += q[(long)y1 * Wl + x0]; v11 += q[(long)y1 * Wl + x1];
    }
    v00 += bias; v01 += bias; v10 += bias; v11 += bias;
    return ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
}

template <typename T>
__global__ __launch_bounds__(256) void hed_fuse_kernel(const HedFuseP p) {
    const int img = blockIdx.y; const long P = (long)p.H * p.W;
    const long pix = (long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= P) return;
    const int y = (int)(pix / p.W), x = (int)(pix - (long)y * p.W);
    float s = 0.f;
#pragma unroll
    for (int l = 0; l < 5; ++l) s += hed_side(p.part[l] + (long)img * p.part_img[l], p.nblk[l], p.bias[l][0], p.H >> l, p.W >> l, p.H, p.W, y, x);
    const float m = s / 5.0f;
    float e = 1.0f / (1.0f + expf(-m)) * 255.0f;
    e = fminf(fmaxf(e, 0.f), 255.f);
    if (p.out) p.out[(long)img * P + pix] = e;
    if (p.control) {
        const float cv = 2.0f * (__fdiv_rn(e, 255.0f) - 0.5f);       // sample_t2i.py:128,141 in that order, rounded once
        T* c = (T*)p.control + (long)img * 3 * P + pix;
        ET<T>::st(c, cv); ET<T>::st(c + P, cv); ET<T>::st(c + 2 * P, cv);
    }
}

// ------------------------------------------------------------------------------------- launchers: every one returns the launch status
extern "C" int car_launch_hed_to_nhwc(int mode, const float* img, const float* norm, void* out, long HW, hipStream_t st) {
    const long n = HW * 3; int g = (int)((n + 255) / 256); if (g > 8192) g = 8192;
    if (mode == 1) hipLaunchKernelGGL(hed_to_nhwc_kernel<bf16_t>, dim3(g), dim3(256), 0, st, img, norm, (bf16_t*)out, HW, n);
    else hipLaunchKernelGGL(hed_to_nhwc_kernel<float>, dim3(g), dim3(256), 0, st, img, norm, (float*)out, HW, n);
    return (int)hipGetLastError();
}
extern "C" int car_launch_hed_conv(int mode, const HedConvP* p, int nimg, hipStream_t st) {
    const long M = (long)p->H * p->W; const long tiles = (M + 127) / 128;
    if (p->N % 64 || p->Kp % 32 || p->K > p->Kp || p->K != 9 * p->Cin || ((p->Cin & 31) && (p->pool || p->Kp != 32)) || p->H <= 0 || p->W <= 0 ||
        tiles > 0x7fffffffL / 128 || nimg <= 0 || nimg > 65535 || p->N / 64 > 65535) return (int)hipErrorInvalidValue;
    if (p->pool ? (p->H != p->Hi / 2 || p->W != p->Wi / 2) : (p->H != p->Hi || p->W != p->Wi)) return (int)hipErrorInvalidValue;
    if (!p->in || !p->w || !p->bias || !p->out || (p->part && !p->proj)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles, p->N / 64, nimg);
    if (mode == 1) hipLaunchKernelGGL(hed_conv_kernel<bf16_t>, grid, dim3(256), 0, st, *p);
    else hipLaunchKernelGGL(hed_conv_kernel<float>, grid, dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int car_launch_hed_fuse(int mode, const HedFuseP* p, int nimg, hipStream_t st) {
    const long P = (long)p->H * p->W;
    if ((p->H >> 4) <= 0 || (p->W >> 4) <= 0 || nimg <= 0 || nimg > 65535 || (!p->out && !p->control)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((P + 255) / 256), nimg);
    if (mode == 1) hipLaunchKernelGGL(hed_fuse_kernel<bf16_t>, grid, dim3(256), 0, st, *p);
    else hipLaunchKernelGGL(hed_fuse_kernel<float>, grid, dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
