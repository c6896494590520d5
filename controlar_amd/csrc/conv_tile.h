// conv_tile.h — the NHWC implicit-GEMM convolution tile on the matrix cores, once, for hed.hip, dpt.hip and lineart.hip (device code only).
// A block computes pixels x 64 output channels; a wave owns MI blocks of 16 pixels x 64 channels (MI x 4 accumulator tiles) on v_mfma_f32_16x16x32_bf16 /
// v_mfma_f32_16x16x4_f32.  k = tap*Cin + ci runs in chunks of 32 staged in LDS as A [pixel][32] and B [channel][32], rows padded to ConvT<T>::LD; the fp32
// tile then goes through Cs [pixel][CONV_CLD] into a vector epilogue: a lane owns 4 consecutive channels of a pixel, the 16 lanes of a pixel are consecutive.
//   conv_rows          which (row, k-slice) 16-byte vectors of a chunk a thread loads, and the output pixel of each
//   conv_mfma_step     the MFMAs of one staged chunk           conv_spill      accumulators -> Cs
//   conv_store4        the 4-channel group store               conv_proj16     a folded 1x1 projection: 4 channels per lane, 16-lane shuffle reduction
//   conv_tile_128x64   the pipelined main loop of hed_conv / dpt_conv: 128 pixels x 64 channels, four waves of 32 x 64, two LDS stages (the global loads of
//                      chunk k+1 fly over the MFMAs of chunk k, one barrier per chunk).  What differs between the networks is the gather of the A tile, a
//                      policy type resolved at compile time, and the epilogue, which stays in the kernel.  la_conv keeps its own single-stage loop (MI = 1).
#pragma once
#include "car_common.h"

template <typename T> struct ConvT;
template <> struct ConvT<bf16_t> { static constexpr int LD = 40, VE = 8; };   // LDS row stride in elements (80 B: 16-B aligned, off the 64-B period); elements per 16 B
template <> struct ConvT<float>  { static constexpr int LD = 36, VE = 4; };
constexpr int CONV_CLD = 68;                                                  // row stride of Cs in floats

// Thread `tid` of 256 loads NV vectors of a ROWS x 32 chunk: vector v is k-slice rko[v] of tile row rrow[v], which is output pixel (rgy, rgx) of the W-wide
// grid if rok[v] (m0 + row < M), else nothing.
template <typename T, int NV>
__device__ __forceinline__ void conv_rows(int tid, int m0, int M, int W, int (&rrow)[NV], int (&rko)[NV], int (&rgy)[NV], int (&rgx)[NV], bool (&rok)[NV]) {
    constexpr int VE = ConvT<T>::VE, VPR = 32 / VE;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int vi = tid + v * 256;
        rrow[v] = vi / VPR; rko[v] = (vi % VPR) * VE;
        const int m = m0 + rrow[v];
        rok[v] = m < M;
        rgy[v] = rok[v] ? m / W : 0; rgx[v] = rok[v] ? m - rgy[v] * W : 0;
    }
}

// One staged chunk: A points at this lane's row (lane & 15) of the wave's first 16-row block, B at row (lane & 15) of the 64-channel tile.
template <typename T, int MI>
__device__ __forceinline__ void conv_mfma_step(const T* A, const T* B, int lane, f32x4 (&acc)[MI][4]) {
    constexpr int LD = ConvT<T>::LD;
    if constexpr (ET<T>::mode == 1) {
        bf16x8 a[MI];
#pragma unroll
        for (int i = 0; i < MI; ++i) a[i] = *(const bf16x8*)&A[16 * i * LD + 8 * (lane >> 4)];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bf16x8 b = *(const bf16x8*)&B[16 * j * LD + 8 * (lane >> 4)];
#pragma unroll
            for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b, acc[i][j], 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            float a[MI];
#pragma unroll
            for (int i = 0; i < MI; ++i) a[i] = A[16 * i * LD + 4 * ks + (lane >> 4)];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float b = B[16 * j * LD + 4 * ks + (lane >> 4)];
#pragma unroll
                for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b, acc[i][j], 0, 0, 0);
            }
        }
    }
}

// accumulators: col = lane & 15, row = 4 * (lane >> 4) + r; row0 is the wave's first row of Cs
template <int MI>
__device__ __forceinline__ void conv_spill(float* Cs, int row0, int lane, const f32x4 (&acc)[MI][4]) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) Cs[(row0 + 16 * i + 4 * (lane >> 4) + r) * CONV_CLD + 16 * j + (lane & 15)] = acc[i][j][r];
}

// the four values travel by value (conv_proj16 too): through an array reference f2bf's NaN select became four branches in the bf16 epilogue
template <typename T>
__device__ __forceinline__ void conv_store4(T* o, float v0, float v1, float v2, float v3) {
    if constexpr (ET<T>::mode == 1) *(uint2*)o = make_uint2((unsigned)f2bf(v0) | ((unsigned)f2bf(v1) << 16), (unsigned)f2bf(v2) | ((unsigned)f2bf(v3) << 16));
    else *(float4*)o = make_float4(v0, v1, v2, v3);
}

// sum over the 64 channels of a pixel of v * proj: this lane's 4 channels (proj points at them; nothing if !ok), then the 16 lanes of the pixel.
// Every lane of the wave must take part in the shuffles.
template <typename T>
__device__ __forceinline__ float conv_proj16(float v0, float v1, float v2, float v3, const T* proj, bool ok) {
    float s = 0.f;
    if (ok) {
        const float v[4] = {v0, v1, v2, v3};
#pragma unroll
        for (int e = 0; e < 4; ++e) s += v[e] * ET<T>::ld(proj + e);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

template <typename T> struct ConvTile128 {
    static constexpr int LD = ConvT<T>::LD, VE = ConvT<T>::VE, NA = 128 * (32 / VE) / 256, NB = 64 * (32 / VE) / 256, ABUF = 128 * LD, BBUF = 64 * LD;
    static constexpr int STAGE_BYTES = 2 * (ABUF + BBUF) * (int)sizeof(T), CS_BYTES = 128 * CONV_CLD * 4;
    static constexpr int SMEM_BYTES = STAGE_BYTES > CS_BYTES ? STAGE_BYTES : CS_BYTES;       // As [2][128][LD] | Bs [2][64][LD], overlaid by Cs [128][CONV_CLD]
};

// The 3x3 / pad 1 main loop of a 256-thread block: pixels m0 .. m0 + 127 of the M = H x W output grid of one image against 64 rows of the weight image
// `w` ([row][Kp], k = tap*Cin + ci, Kp a multiple of 32; where G::PARTIAL_N, rows from wrows on read as zero).  Returns with the fp32 tile in Cs = (float*)smem behind a barrier.
// The gather policy G, resolved at compile time:
//   G::PARTIAL_N                        whether the weight image may end inside the 64-row tile (N not a multiple of 64)
//   int  cin()                          input channels; where vectors() holds a multiple of 32, so a chunk lies inside one tap
//   int  stride()                       output pixel (gy, gx) has its centre tap at input (gy * stride, gx * stride)
//   bool inside(int iy, int ix)         whether input pixel (iy, ix) exists (outside the map the tap reads zero)
//   uint4 vec(int iy, int ix, int c)    the 16 bytes at channels c .. of an input pixel inside the map
//   G::HAS_FILL, bool vectors(), void fill(T* A, int k0, int m0, int M, int tid)    optional: where vectors() is false the block writes chunk k0 of the A
//                                       stage element by element itself (HED's Cin = 3)
template <typename T, typename G>
__device__ __forceinline__ void conv_tile_128x64(char* smem, const G& g, const T* __restrict__ w, int wrows, int Kp, int m0, int M, int W) {
    using C = ConvTile128<T>;
    constexpr int LD = C::LD, NA = C::NA, NB = C::NB, ABUF = C::ABUF, BBUF = C::BBUF;
    T* const As = (T*)smem;
    T* const Bs = As + 2 * ABUF;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int rrow[NA], rko[NA], rgy[NA], rgx[NA]; bool rok[NA];
    conv_rows<T, NA>(tid, m0, M, W, rrow, rko, rgy, rgx, rok);
#pragma unroll
    for (int v = 0; v < NA; ++v) { rgy[v] *= g.stride(); rgx[v] *= g.stride(); }             // centre tap in input coordinates
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bool vecs = true;
    if constexpr (G::HAS_FILL) vecs = g.vectors();
    uint4 ra[NA], rb[NB];
    auto load = [&](int k0) {
        if (vecs) {
            const int tap = k0 / g.cin(), c0 = k0 - tap * g.cin();
            const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
#pragma unroll
            for (int v = 0; v < NA; ++v) {
                ra[v] = make_uint4(0u, 0u, 0u, 0u);
                const int iy = rgy[v] + dy, ix = rgx[v] + dx;
                if (rok[v] && g.inside(iy, ix)) ra[v] = g.vec(iy, ix, c0 + rko[v]);
            }
        }
#pragma unroll
        for (int v = 0; v < NB; ++v) rb[v] = !G::PARTIAL_N || rrow[v] < wrows ? *(const uint4*)(w + (long)rrow[v] * Kp + k0 + rko[v]) : make_uint4(0u, 0u, 0u, 0u);
    };
    auto stage = [&](int k0, int buf) {
        T* A = As + buf * ABUF; T* B = Bs + buf * BBUF;
        if (vecs) {
#pragma unroll
            for (int v = 0; v < NA; ++v) *(uint4*)&A[rrow[v] * LD + rko[v]] = ra[v];
        } else if constexpr (G::HAS_FILL) g.fill(A, k0, m0, M, tid);
#pragma unroll
        for (int v = 0; v < NB; ++v) *(uint4*)&B[rrow[v] * LD + rko[v]] = rb[v];
    };
    load(0);
    stage(0, 0);
    __syncthreads();
    int cur = 0;
    for (int k0 = 0; k0 < Kp; k0 += 32) {
        const bool more = k0 + 32 < Kp;
        if (more) load(k0 + 32);
        conv_mfma_step<T, 2>(As + cur * ABUF + (32 * wv + (lane & 15)) * LD, Bs + cur * BBUF + (lane & 15) * LD, lane, acc);
        if (more) stage(k0 + 32, cur ^ 1);            // the other stage: its last readers passed the barrier that ended the previous chunk
        __syncthreads();
        cur ^= 1;
    }
    conv_spill<2>((float*)smem, 32 * wv, lane, acc);  // Cs overlays the stages: every wave is past the loop's last barrier
    __syncthreads();
}
