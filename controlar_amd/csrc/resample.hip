// resample.hip — Pillow's 8-bit image resampler (ImagingResample, modes L and RGB) on the GPU: the PIL resize in front of every condition extractor
// (sample_t2i_MR.py:37-49, dataset/augmentation.py:8-26, sample_t2i.py:135, demo/model.py:127,221, condition/utils.py:28-38).  Pillow's arithmetic is
// integer on host-computed fixed-point tables (resample_tab.h), so the result is bit-identical to Pillow's: a horizontal pass into a uint8 intermediate
// (that rounding is part of the result), then a vertical pass.  Two kernels with the intermediate in global memory: threads run along the interleaved
// row (x fastest) in both passes, each owns 4 consecutive bytes, taps come through the cache (the vertical pass reads one wave-uniform coefficient row).
//   pass 0  horizontal: byte loads of the taps (stride C), one dword store per thread into the 4-byte-pitched intermediate.  When the pass feeds the
//           vertical one and a tile's source span fits in LDS, resample_h_lds_kernel does it instead: a block stages the span of 64 output pixels for
//           up to 16 source rows in LDS with dword loads, a thread owns one output pixel (its taps are loaded once for all its rows and channels,
//           the pixels come from LDS) and the tile leaves as dwords.  Same sums, same bits; the call takes half the time of the byte gather at
//           1024^2 -> 512^2, B = 16 (profiles/resize_time.jsonl).
//   pass 1  vertical:   dword loads of the intermediate, 4 sums per thread
//   pass 2  copy:       both axes untouched (Pillow returns a copy)
// The last pass of a call carries the epilogue: the dense uint8 image and / or the control tensor and / or the fp32 NCHW tensor (kernel_params.h).
#include "car_common.h"
#include "kernel_params.h"

__device__ __forceinline__ int rs_clip8(int acc) {
    acc >>= 22;                                   // arithmetic shift: a negative sum clamps to 0
    return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}

template <int PASS, typename T>
__global__ __launch_bounds__(256) void resample_kernel(const ResampleP p) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= p.nq) return;
    const int e0 = q * 4, C = p.C;
    const long nrow = (long)p.B * p.rows;
    for (long rr = (long)blockIdx.y * 4 + threadIdx.y; rr < nrow; rr += (long)gridDim.y * 4) {
        const int b = (int)(rr / p.rows), r = (int)(rr - (long)b * p.rows);
        const unsigned char* img = p.src + (long)b * p.src_img;
        int v[4] = {0, 0, 0, 0};
        if (PASS == 0) {
            const unsigned char* row = img + (long)(p.src_y0 + r) * p.src_pitch;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = e0 + j;
                if (e < p.row_bytes) {
                    const int x = C == 3 ? e / 3 : e, c = e - x * C;
                    const int xmin = p.bounds[2 * x], n = p.bounds[2 * x + 1];
                    const int* k = p.kk + (long)x * p.ksize;
                    const unsigned char* s = row + (long)xmin * C + c;
                    int acc = 1 << 21;
                    for (int t = 0; t < n; ++t) acc += (int)s[(long)t * C] * k[t];
                    v[j] = rs_clip8(acc);
                }
            }
        } else if (PASS == 1) {
            const int ymin = p.bounds[2 * r], n = p.bounds[2 * r + 1];
            const int* k = p.kk + (long)r * p.ksize;
            const unsigned char* s = img + (long)(ymin - p.src_y0) * p.src_pitch + e0;
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
            if (p.src_aligned && e0 + 4 <= p.src_pitch) {
                for (int t = 0; t < n; ++t) {
                    const unsigned w = *(const unsigned*)(s + (long)t * p.src_pitch);
                    const int kt = k[t];
                    a0 += (int)(w & 255u) * kt; a1 += (int)((w >> 8) & 255u) * kt; a2 += (int)((w >> 16) & 255u) * kt; a3 += (int)(w >> 24) * kt;
                }
            } else {
                const int nv = p.row_bytes - e0;          // >= 1: only valid bytes of the source row are read
                for (int t = 0; t < n; ++t) {
                    const unsigned char* u = s + (long)t * p.src_pitch;
                    const int kt = k[t];
                    a0 += (int)u[0] * kt;
                    if (nv > 1) a1 += (int)u[1] * kt;
                    if (nv > 2) a2 += (int)u[2] * kt;
                    if (nv > 3) a3 += (int)u[3] * kt;
                }
            }
            v[0] = rs_clip8(a0); v[1] = rs_clip8(a1); v[2] = rs_clip8(a2); v[3] = rs_clip8(a3);
        } else {
            const unsigned char* row = img + (long)r * p.src_pitch;
#pragma unroll
            for (int j = 0; j < 4; ++j) if (e0 + j < p.row_bytes) v[j] = row[e0 + j];
        }
        const int nv = p.row_bytes - e0 < 4 ? p.row_bytes - e0 : 4;
        const unsigned pack = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
        if (!p.final) {
            // nv may be <= 0 in the pad quad of the pitch: it stores zeros
            *(unsigned*)(p.tmp + (long)b * p.tmp_img + (long)r * p.tmp_pitch + e0) = nv > 0 ? pack : 0u;
            continue;
        }
        if (nv <= 0) continue;
        if (p.out) {
            unsigned char* o = p.out + ((long)b * p.rows + r) * p.row_bytes + e0;
            if (nv == 4 && ((uintptr_t)o & 3) == 0) *(unsigned*)o = pack;
            else for (int j = 0; j < nv; ++j) o[j] = (unsigned char)v[j];
        }
        if (p.control || p.fout) {
            const long plane = (long)p.rows * p.Wo;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j >= nv) break;
                const int e = e0 + j, x = C == 3 ? e / 3 : e, c = e - x * C;
                const long pix = (long)r * p.Wo + x;
                const float f = (float)v[j];
                const float nrm = 2.0f * (f / 255.0f - 0.5f);      // = (f/255 - 0.5)/0.5 bit for bit: the division is correctly rounded, the doubling exact
                if (p.control) {
                    T* cp = (T*)p.control + (long)b * 3 * plane + pix;
                    if (C == 3) ET<T>::st(cp + c * plane, nrm);
                    else { ET<T>::st(cp, nrm); ET<T>::st(cp + plane, nrm); ET<T>::st(cp + 2 * plane, nrm); }
                }
                if (p.fout) p.fout[((long)b * C + c) * plane + pix] = p.norm ? nrm : f;
            }
        }
    }
}

// The horizontal pass into the intermediate with the source staged in LDS.  Block = 64 output pixels x `rb` source rows (grid.x tiles of RS_TX
// pixels, grid.y strides over the B * ceil(rows / rb) row groups).  Dynamic LDS: rb rows of row_stride bytes, each holding the dwords that cover
// source bytes [s0*C, s1*C) of its row (s0 = first tap of the tile's first pixel, s1 = end of the taps of its last; the bounds are monotone in x),
// then the rb x (RS_TX*C) result tile.  The host guarantees row_stride >= span*C + 6 for every tile and rb*(row_stride + RS_TX*C) <= 48 KiB.
#define RS_TX 64
__global__ __launch_bounds__(256) void resample_h_lds_kernel(const ResampleP p, int rb, int row_stride) {
    extern __shared__ unsigned rs_lds[];
    unsigned char* ls = (unsigned char*)rs_lds;
    const int C = p.C, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ob = RS_TX * C;                                   // bytes of one result row of the tile: a multiple of 4
    unsigned char* lo = ls + (long)rb * row_stride;
    const int X0 = blockIdx.x * RS_TX, nx = p.Wo - X0 < RS_TX ? p.Wo - X0 : RS_TX;
    const int xl = X0 + nx - 1;
    const int s0 = p.bounds[2 * X0], s1 = p.bounds[2 * xl] + p.bounds[2 * xl + 1];
    const int span_bytes = (s1 - s0) * C;
    const int x = X0 + lane;
    const bool live = lane < nx;
    const int xmin = live ? p.bounds[2 * x] : s0, n = live ? p.bounds[2 * x + 1] : 0;
    const int* k = p.kk + (long)(live ? x : X0) * p.ksize;
    int tile_bytes = p.tmp_pitch - X0 * C;                      // what the tile writes of a row of the intermediate: dwords, the pitch's pad included
    if (tile_bytes > ob) tile_bytes = ob;
    const int ndw = tile_bytes >> 2;
    const int gpi = (p.rows + rb - 1) / rb;                     // row groups per image
    const long ngroups = (long)p.B * gpi;
    for (long g = blockIdx.y; g < ngroups; g += gridDim.y) {
        const int b = (int)(g / gpi), r0 = (int)(g - (long)b * gpi) * rb;
        const int nr = p.rows - r0 < rb ? p.rows - r0 : rb;
        const unsigned char* first = p.src + (long)b * p.src_img + (long)(p.src_y0 + r0) * p.src_pitch + (long)s0 * C;
        // stage: wave wv takes rows wv, wv + 4, ...; aligned dwords that cover the row's span (a dword that holds a byte of the image lies in its page)
        for (int j = wv; j < nr; j += 4) {
            const uintptr_t a = (uintptr_t)(first + (long)j * p.src_pitch);
            const unsigned* gsrc = (const unsigned*)(a & ~(uintptr_t)3);
            const int nd = ((int)(a & 3) + span_bytes + 3) >> 2;
            unsigned* dst = (unsigned*)(ls + (long)j * row_stride);
            for (int d = lane; d < nd; d += 64) dst[d] = gsrc[d];
        }
        __syncthreads();
        // sums: this thread's pixel for rows wv, wv + 4, wv + 8, wv + 12 (those below rb), all channels; a tap is loaded once for all of them
        int acc[4][3];
        const unsigned char* lrow[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = wv + 4 * i < rb ? wv + 4 * i : 0;    // rows past rb re-read row 0 (never stored); rows in [nr, rb) hold stale bytes (never stored)
            const uintptr_t a = (uintptr_t)(first + (long)j * p.src_pitch);
            lrow[i] = ls + (long)j * row_stride + (int)(a & 3) + (xmin - s0) * C;
            acc[i][0] = acc[i][1] = acc[i][2] = 1 << 21;
        }
        for (int t = 0; t < n; ++t) {
            const int kt = k[t];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned char* q = lrow[i] + t * C;
                acc[i][0] += (int)q[0] * kt;
                if (C == 3) { acc[i][1] += (int)q[1] * kt; acc[i][2] += (int)q[2] * kt; }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = wv + 4 * i;
            if (j < rb) {
                unsigned char* o = lo + (long)j * ob + lane * C;
                o[0] = live ? (unsigned char)rs_clip8(acc[i][0]) : (unsigned char)0;
                if (C == 3) { o[1] = live ? (unsigned char)rs_clip8(acc[i][1]) : (unsigned char)0; o[2] = live ? (unsigned char)rs_clip8(acc[i][2]) : (unsigned char)0; }
            }
        }
        __syncthreads();
        for (int i = tid; i < nr * ndw; i += 256) {
            const int j = i / ndw, d = i - j * ndw;
            *(unsigned*)(p.tmp + (long)b * p.tmp_img + (long)(r0 + j) * p.tmp_pitch + (long)X0 * C + 4 * d) = ((const unsigned*)(lo + (long)j * ob))[d];
        }
        __syncthreads();
    }
}

extern "C" void car_launch_resample_h_lds(const ResampleP* p, int rb, int row_stride, hipStream_t st) {
    const long ngroups = (long)p->B * ((p->rows + rb - 1) / rb);
    if (ngroups <= 0 || p->Wo <= 0) return;
    const dim3 grid((unsigned)((p->Wo + RS_TX - 1) / RS_TX), (unsigned)(ngroups > 65535 ? 65535 : ngroups));
    const size_t lds = (size_t)rb * ((size_t)row_stride + (size_t)RS_TX * p->C);
    hipLaunchKernelGGL(resample_h_lds_kernel, grid, dim3(256), lds, st, *p, rb, row_stride);
}

template <typename T>
static void launch_pass(int pass, const ResampleP& p, dim3 grid, hipStream_t st) {
    if (pass == 0) hipLaunchKernelGGL((resample_kernel<0, T>), grid, dim3(64, 4), 0, st, p);
    else if (pass == 1) hipLaunchKernelGGL((resample_kernel<1, T>), grid, dim3(64, 4), 0, st, p);
    else hipLaunchKernelGGL((resample_kernel<2, T>), grid, dim3(64, 4), 0, st, p);
}

extern "C" void car_launch_resample(int mode, int pass, const ResampleP* p, hipStream_t st) {
    const long nrow = (long)p->B * p->rows;
    if (nrow <= 0 || p->nq <= 0) return;
    const long gy = (nrow + 3) / 4;
    const dim3 grid((unsigned)((p->nq + 63) / 64), (unsigned)(gy > 65535 ? 65535 : gy));
    if (mode == 1) launch_pass<bf16_t>(pass, *p, grid, st);
    else launch_pass<float>(pass, *p, grid, st);
}
