// dpt.hip — neck and head of the DPT depth estimator (transformers modeling_dpt.py: DPTReassembleStage, DPTNeck.convs, DPTFeatureFusionStage,
// DPTDepthEstimationHead) on the GPU.  Activations are NHWC in the context's element type T (bf16_t fast / float exact), accumulators fp32, the
// final map fp32 (DPT section).  The ViT backbone and every 1x1 convolution run on gemm.hip / attn.hip / ops.hip (engine_depth.hip).
//   dpt_patchify   fp32 NCHW pixel_values -> T patch matrix [image*token][3*16*16], k = (c, py, px) as Conv2d(3, D, 16, 16).weight flattens.
//   dpt_conv       3x3 / pad 1 / stride 1 or 2 implicit GEMM on the shared tile loop (conv_tile.h: 128 pixels x 64 channels per block, two LDS
//                  stages).  Switches: ReLU on the input inside the gather (the pre-activation of a
//                  residual conv unit), optional bias, up to two residual addends, ReLU on the output, and — for the head's last conv — the
//                  32 -> 1 projection + ReLU folded into the epilogue (fp32 map out).  N need not be a multiple of 64: rows of the weight tile
//                  beyond N are zero, their outputs are never stored.
//   dpt_shuffle    the store side of a ConvTranspose2d whose kernel equals its stride: GEMM output [pixel][(ky, kx, c)] -> NHWC [k*g][k*g][C].
//   dpt_up2        bilinear x2, align_corners = True, as ATen computes it (source index = dst * (in-1)/(out-1) in fp32).
//   dpt_max, dpt_control   per-image maximum of the map (one block per image, fixed order) and the control tensor 2*(d/max - 0.5).
// No atomics anywhere and no tile crosses an image: two calls give the same bits, and image i alone gives the bits of image i in a batch.
#include "car_common.h"
#include "kernel_params.h"
#include "conv_tile.h"

// 16 bytes of T <-> fp32
__device__ __forceinline__ void dpt_ldv(const bf16_t* p, float (&v)[8]) {
    const uint4 u = *(const uint4*)p; const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[2 * e] = __uint_as_float(w[e] << 16); v[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u); }
}
__device__ __forceinline__ void dpt_ldv(const float* p, float (&v)[4]) { const float4 u = *(const float4*)p; v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w; }
__device__ __forceinline__ void dpt_stv(bf16_t* p, const float (&v)[8]) {
    *(uint4*)p = make_uint4((unsigned)f2bf(v[0]) | ((unsigned)f2bf(v[1]) << 16), (unsigned)f2bf(v[2]) | ((unsigned)f2bf(v[3]) << 16),
                            (unsigned)f2bf(v[4]) | ((unsigned)f2bf(v[5]) << 16), (unsigned)f2bf(v[6]) | ((unsigned)f2bf(v[7]) << 16));
}
__device__ __forceinline__ void dpt_stv(float* p, const float (&v)[4]) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }

template <typename T>
__global__ void dpt_patchify_kernel(const float* __restrict__ img, T* __restrict__ out, int S, int g, long total) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x; const long st = (long)gridDim.x * blockDim.x;
    const long n = (long)g * g, plane = (long)S * S;
    for (; i < total; i += st) {                     // i = (image*n + token)*768 + k
        const long row = i / 768; const int k = (int)(i - row * 768);
        const long b = row / n; const int r = (int)(row - b * n), gy = r / g, gx = r - gy * g;
        const int c = k >> 8, py = (k >> 4) & 15, px = k & 15;
        ET<T>::st(out + i, img[(b * 3 + c) * plane + (long)(gy * 16 + py) * S + gx * 16 + px]);
    }
}

// max(x, 0) on a 16-byte vector of T
template <typename T> __device__ __forceinline__ uint4 dpt_vrelu(uint4 a);
template <> __device__ __forceinline__ uint4 dpt_vrelu<float>(uint4 a) {
    return make_uint4(__float_as_uint(fmaxf(__uint_as_float(a.x), 0.f)), __float_as_uint(fmaxf(__uint_as_float(a.y), 0.f)),
                      __float_as_uint(fmaxf(__uint_as_float(a.z), 0.f)), __float_as_uint(fmaxf(__uint_as_float(a.w), 0.f)));
}
__device__ __forceinline__ unsigned dpt_relu2bf(unsigned w) {      // two bf16 per word: clear every half whose sign bit is set
    const unsigned neg = ((w >> 15) & 0x00010001u) * 0xffffu;
    return w & ~neg;
}
template <> __device__ __forceinline__ uint4 dpt_vrelu<bf16_t>(uint4 a) {
    return make_uint4(dpt_relu2bf(a.x), dpt_relu2bf(a.y), dpt_relu2bf(a.z), dpt_relu2bf(a.w));
}

// The A-tile gather of dpt_conv (conv_tile.h): zero pad 1, stride 1 or 2, optionally max(x, 0).  Cin % 32 == 0: every chunk is vectors.
template <typename T>
struct DptGather {
    static constexpr bool HAS_FILL = false, PARTIAL_N = true;
    const DptConvP& p; const T* __restrict__ in;
    __device__ __forceinline__ int cin() const { return p.Cin; }
    __device__ __forceinline__ int stride() const { return p.stride; }
    __device__ __forceinline__ bool inside(int iy, int ix) const { return iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi; }
    __device__ __forceinline__ uint4 vec(int iy, int ix, int c) const {
        const uint4 t = *(const uint4*)(in + ((long)iy * p.Wi + ix) * p.Cin + c);
        return p.relu_in ? dpt_vrelu<T>(t) : t;
    }
};

template <typename T>
__global__ __launch_bounds__(256) void dpt_conv_kernel(const DptConvP p) {
    __shared__ __attribute__((aligned(16))) char smem[ConvTile128<T>::SMEM_BYTES];
    const int tid = threadIdx.x;
    const int img = blockIdx.z, n0 = blockIdx.y * 64, m0 = blockIdx.x * 128;
    const int M = p.H * p.W;
    const DptGather<T> g{p, (const T*)p.in + (long)img * p.in_img};
    conv_tile_128x64<T>(smem, g, (const T*)p.w + (long)n0 * p.K, p.N - n0, p.K, m0, M, p.W);      // rows of the 64-channel tile beyond N read as zero
    const float* const Cs = (const float*)smem;
    const int rows = M - m0 < 128 ? M - m0 : 128;
    T* __restrict__ out = p.out ? (T*)p.out + (long)img * p.out_img : nullptr;
    const T* __restrict__ r1 = p.res1 ? (const T*)p.res1 + (long)img * p.res1_img : nullptr;
    const T* __restrict__ r2 = p.res2 ? (const T*)p.res2 + (long)img * p.res2_img : nullptr;
    const T* __restrict__ proj = (const T*)p.proj;
    float* __restrict__ map = proj ? p.map + (long)img * p.map_img : nullptr;
#pragma unroll 2
    for (int it = 0; it < 8; ++it) {                  // 128 rows x 16 four-channel groups; the 16 groups of a row are 16 consecutive lanes
        const int idx = tid + it * 256, row = idx >> 4, c4 = (idx & 15) * 4;
        const bool ok = row < rows && n0 + c4 < p.N;  // N % 4 == 0: a group lies inside N or outside it
        const float4 x = *(const float4*)&Cs[row * CONV_CLD + c4];
        float v[4] = {x.x, x.y, x.z, x.w};
        if (ok) {
            const long o = (long)(m0 + row) * p.N + n0 + c4;
            if (p.bias) { const float4 b = *(const float4*)&p.bias[n0 + c4]; v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w; }
            if (r1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += ET<T>::ld(r1 + o + e);
            }
            if (r2) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += ET<T>::ld(r2 + o + e);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = ET<T>::rnd(p.relu_out && v[e] < 0.f ? 0.f : v[e]);
            if (out) conv_store4(out + o, v[0], v[1], v[2], v[3]);
        }
        if (proj) {                                   // uniform over the block: every lane takes part in the shuffles
            float s = conv_proj16(v[0], v[1], v[2], v[3], proj + n0 + c4, ok);
            if (row < rows && (idx & 15) == 0) { s += p.proj_bias[0]; map[m0 + row] = s > 0.f ? s : 0.f; }
        }
    }
}

// GEMM output of a ConvTranspose2d with kernel = stride = k: in [image*g*g][(ky*k + kx)*C + c] -> out [image][g*k][g*k][C]
template <typename T>
__global__ void dpt_shuffle_kernel(const T* __restrict__ in, T* __restrict__ out, int g, int k, int C, long nvec) {
    constexpr int VE = ConvT<T>::VE;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x; const long st = (long)gridDim.x * blockDim.x;
    const int cv = C / VE, rowv = k * k * cv, gk = g * k;
    for (; i < nvec; i += st) {
        const long row = i / rowv; const int q = (int)(i - row * rowv), tap = q / cv, c = (q - tap * cv) * VE, ky = tap / k, kx = tap - ky * k;
        const long b = row / ((long)g * g); const int r = (int)(row - b * g * g), y = r / g, x = r - y * g;
        *(uint4*)(out + ((b * gk + y * k + ky) * gk + x * k + kx) * C + c) = *(const uint4*)(in + i * VE);
    }
}

// bilinear x2, align_corners = True (ATen upsample_bilinear2d): in [image][h][w][C] -> out [image][2h][2w][C]
template <typename T>
__global__ void dpt_up2_kernel(const T* __restrict__ in, T* __restrict__ out, int h, int w, int C, long nvec) {
    constexpr int VE = ConvT<T>::VE;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x; const long st = (long)gridDim.x * blockDim.x;
    const int cv = C / VE, Ho = 2 * h, Wo = 2 * w;
    const float sh = (float)(h - 1) / (float)(Ho - 1), sw = (float)(w - 1) / (float)(Wo - 1);
    for (; i < nvec; i += st) {
        const long pix = i / cv; const int c = (int)(i - pix * cv) * VE;
        const long b = pix / ((long)Ho * Wo); const int r = (int)(pix - b * Ho * Wo), oy = r / Wo, ox = r - oy * Wo;
        const float sy = sh * (float)oy, sx = sw * (float)ox;
        int y0 = (int)sy, x0 = (int)sx;
        y0 = y0 < h - 1 ? y0 : h - 1; x0 = x0 < w - 1 ? x0 : w - 1;
        const int y1 = y0 < h - 1 ? y0 + 1 : y0, x1 = x0 < w - 1 ? x0 + 1 : x0;
        const float ly1 = fminf(fmaxf(sy - (float)y0, 0.f), 1.f), ly0 = 1.f - ly1, lx1 = fminf(fmaxf(sx - (float)x0, 0.f), 1.f), lx0 = 1.f - lx1;
        const T* s = in + b * h * w * C + c;
        float v00[VE], v01[VE], v10[VE], v11[VE], o[VE];
        dpt_ldv(s + ((long)y0 * w + x0) * C, v00); dpt_ldv(s + ((long)y0 * w + x1) * C, v01);
        dpt_ldv(s + ((long)y1 * w + x0) * C, v10); dpt_ldv(s + ((long)y1 * w + x1) * C, v11);
#pragma unroll
        for (int e = 0; e < VE; ++e) o[e] = ly0 * (lx0 * v00[e] + lx1 * v01[e]) + ly1 * (lx0 * v10[e] + lx1 * v11[e]);
        dpt_stv(out + i * VE, o);
    }
}

// mx[image] = max over the image's map (values >= 0: the order of a maximum changes no bit)
__global__ __launch_bounds__(1024) void dpt_max_kernel(const float* __restrict__ map, long map_img, float* __restrict__ mx, long P) {
    __shared__ float sm[17];
    const float* m = map + (long)blockIdx.x * map_img;
    float v = 0.f;
    for (long i = threadIdx.x; i < P; i += 1024) v = fmaxf(v, m[i]);
    v = block_max(v, sm);
    if (threadIdx.x == 0) mx[blockIdx.x] = v;
}

template <typename T>
__global__ __launch_bounds__(256) void dpt_control_kernel(const float* __restrict__ map, long map_img, const float* __restrict__ mx, T* __restrict__ control, long P) {
    const int img = blockIdx.y; const long pix = (long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= P) return;
    const float m = mx[img], d = map[(long)img * map_img + pix];
    const float cv = m > 0.f ? 2.0f * (__fdiv_rn(d, m) - 0.5f) : -1.0f;      // an all-zero map: -1 where the reference's 0/0 gives NaN
    T* c = control + (long)img * 3 * P + pix;
    ET<T>::st(c, cv); ET<T>::st(c + P, cv); ET<T>::st(c + 2 * P, cv);
}

// ------------------------------------------------------------------------------------- launchers: every one returns the launch status
static inline int dpt_grid(long n) { long g = (n + 255) / 256; return (int)(g > 16384 ? 16384 : (g < 1 ? 1 : g)); }

extern "C" int car_launch_dpt_patchify(int mode, const float* img, void* out, int nimg, int S, hipStream_t st) {
    if (!img || !out || nimg <= 0 || S < 16 || S % 16) return (int)hipErrorInvalidValue;
    const int g = S / 16; const long total = (long)nimg * g * g * 768;
    if (mode == 1) hipLaunchKernelGGL(dpt_patchify_kernel<bf16_t>, dim3(dpt_grid(total)), dim3(256), 0, st, img, (bf16_t*)out, S, g, total);
    else hipLaunchKernelGGL(dpt_patchify_kernel<float>, dim3(dpt_grid(total)), dim3(256), 0, st, img, (float*)out, S, g, total);
    return (int)hipGetLastError();
}
extern "C" int car_launch_dpt_conv(int mode, const DptConvP* p, int nimg, hipStream_t st) {
    const long M = (long)p->H * p->W; const long tiles = (M + 127) / 128;
    if (p->Cin <= 0 || p->Cin % 32 || p->N <= 0 || p->N % 4 || p->K != 9 * p->Cin || p->H <= 0 || p->W <= 0 || (p->stride != 1 && p->stride != 2) ||
        tiles > 0x7fffffffL / 128 || nimg <= 0 || nimg > 65535 || (p->N + 63) / 64 > 65535) return (int)hipErrorInvalidValue;
    if (p->stride == 1 ? (p->H != p->Hi || p->W != p->Wi) : (p->H != (p->Hi - 1) / 2 + 1 || p->W != (p->Wi - 1) / 2 + 1)) return (int)hipErrorInvalidValue;
    if (!p->in || !p->w || (!p->out && !p->proj) || (p->proj && (!p->map || !p->proj_bias || p->N > 64))) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles, (unsigned)((p->N + 63) / 64), nimg);
    if (mode == 1) hipLaunchKernelGGL(dpt_conv_kernel<bf16_t>, grid, dim3(256), 0, st, *p);
    else hipLaunchKernelGGL(dpt_conv_kernel<float>, grid, dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int car_launch_dpt_shuffle(int mode, const void* in, void* out, int nimg, int g, int k, int C, hipStream_t st) {
    const int VE = mode == 1 ? 8 : 4;
    if (!in || !out || nimg <= 0 || g <= 0 || k <= 0 || C <= 0 || C % VE) return (int)hipErrorInvalidValue;
    const long nvec = (long)nimg * g * g * k * k * (C / VE);
    if (mode == 1) hipLaunchKernelGGL(dpt_shuffle_kernel<bf16_t>, dim3(dpt_grid(nvec)), dim3(256), 0, st, (const bf16_t*)in, (bf16_t*)out, g, k, C, nvec);
    else hipLaunchKernelGGL(dpt_shuffle_kernel<float>, dim3(dpt_grid(nvec)), dim3(256), 0, st, (const float*)in, (float*)out, g, k, C, nvec);
    return (int)hipGetLastError();
}
extern "C" int car_launch_dpt_up2(int mode, const void* in, void* out, int nimg, int h, int w, int C, hipStream_t st) {
    const int VE = mode == 1 ? 8 : 4;
    if (!in || !out || nimg <= 0 || h <= 0 || w <= 0 || C <= 0 || C % VE) return (int)hipErrorInvalidValue;
    const long nvec = (long)nimg * 4 * h * w * (C / VE);
    if (mode == 1) hipLaunchKernelGGL(dpt_up2_kernel<bf16_t>, dim3(dpt_grid(nvec)), dim3(256), 0, st, (const bf16_t*)in, (bf16_t*)out, h, w, C, nvec);
    else hipLaunchKernelGGL(dpt_up2_kernel<float>, dim3(dpt_grid(nvec)), dim3(256), 0, st, (const float*)in, (float*)out, h, w, C, nvec);
    return (int)hipGetLastError();
}
extern "C" int car_launch_dpt_max(const float* map, long map_img, float* mx, int nimg, long P, hipStream_t st) {
    if (!map || !mx || nimg <= 0 || P <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(dpt_max_kernel, dim3(nimg), dim3(1024), 0, st, map, map_img, mx, P);
    return (int)hipGetLastError();
}
extern "C" int car_launch_dpt_control(int mode, const float* map, long map_img, const float* mx, void* control, int nimg, long P, hipStream_t st) {
    if (!map || !mx || !control || nimg <= 0 || nimg > 65535 || P <= 0) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((P + 255) / 256), nimg);
    if (mode == 1) hipLaunchKernelGGL(dpt_control_kernel<bf16_t>, grid, dim3(256), 0, st, map, map_img, mx, (bf16_t*)control, P);
    else hipLaunchKernelGGL(dpt_control_kernel<float>, grid, dim3(256), 0, st, map, map_img, mx, (float*)control, P);
    return (int)hipGetLastError();
}
