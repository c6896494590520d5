// metrics.hip — the control-consistency metrics of evaluations/{hed,lineart}_ssim.py, canny_f1score.py, depth_rmse.py and autoregressive/test/metric.py
// on the device: multi-scale SSIM (one fused launch per scale and one fold), binary F1 from integer counts, RMSE with the per-image 255/max scaling, and
// the save_image pixel quantiser in front of the extractors.  No atomics anywhere: every reduction is a wave shuffle, then LDS, then one partial per block,
// folded per image in a fixed order by a last launch — a result depends neither on the launch nor on what else is in the batch.  Accumulation is fp64
// throughout (the variance E[p^2] - mu^2 of a soft edge map cancels to nothing in fp32); pixels travel as fp32.
#include "car_common.h"
#include "metrics_params.h"

__device__ inline double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// block-wide sum for 256 threads; `sm` has 4 doubles.  Fixed order: deterministic.
__device__ inline double block_sum_d(double v, double* sm) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

__device__ inline float ld_pix(const void* p, int dt, size_t i) { return dt == MT_U8 ? (float)((const unsigned char*)p)[i] : ((const float*)p)[i]; }

// ------------------------------------------------------------------------------------- MS-SSIM
// One scale.  A workgroup owns a 32 x 32 tile of the cropped SSIM map of one plane.  Output (y, x) of that map is the 11 x 11 window over input rows
// y .. y+10, columns x .. x+10: the crop of 5 equals the reflect padding of 5, so no kept pixel's window touches the padding and the kernel is a plain
// valid convolution.  The 42 x 42 halo tile of both images is staged in LDS once (clip(v * scale, 0, 1) applied on the way in); the five maps p, t, p^2, t^2,
// p*t are row-filtered into LDS and column-filtered from there in two strips of 16 output rows (26 filtered rows each: 33 KB instead of 54 KB for the
// whole tile), so nothing but the two images is read from memory and nothing but one (ssim, cs) pair per tile and the pooled images is written.
// The same tile feeds avg_pool2d(2): a workgroup pools its own 32 x 32 inputs, the last one of a row or column its whole halo, which reaches the image's edge.
__global__ __launch_bounds__(256) void ms_ssim_scale_kernel(const MsScaleP a) {
    __shared__ float sp[MS_HALO][MS_HALO], st[MS_HALO][MS_HALO];
    __shared__ double R[5][MS_STRIP + MS_K - 1][MS_T];
    __shared__ double red[2][4];
    const int tid = threadIdx.x;
    const int ntile = a.tiles_x * a.tiles_y;
    const long plane = blockIdx.x / ntile;
    const int tile = (int)(blockIdx.x - plane * ntile), ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int y0 = ty * MS_T, x0 = tx * MS_T;
    const size_t base = (size_t)plane * a.H * a.W;
    for (int i = tid; i < MS_HALO * MS_HALO; i += 256) {
        const int r = i / MS_HALO, c = i - r * MS_HALO, gy = y0 + r, gx = x0 + c;
        float vp = 0.f, vt = 0.f;
        if (gy < a.H && gx < a.W) {
            const size_t at = base + (size_t)gy * a.W + gx;
            vp = (float)fmin(fmax((double)ld_pix(a.p, a.dt_p, at) * a.scale_p, 0.0), 1.0);
            vt = (float)fmin(fmax((double)ld_pix(a.t, a.dt_t, at) * a.scale_t, 0.0), 1.0);
        }
        sp[r][c] = vp; st[r][c] = vt;
    }
    __syncthreads();
    if (a.next_p) {
        const int pr = ty == a.tiles_y - 1 ? MS_HALO / 2 : MS_T / 2, pc = tx == a.tiles_x - 1 ? MS_HALO / 2 : MS_T / 2;
        for (int i = tid; i < pr * pc; i += 256) {
            const int py = i / pc, px = i - py * pc, gy = y0 / 2 + py, gx = x0 / 2 + px;
            if (gy < a.Hn && gx < a.Wn) {          // 2 gy + 1 < H, 2 gx + 1 < W: floor pooling drops an odd last row or column
                const size_t at = (size_t)plane * a.Hn * a.Wn + (size_t)gy * a.Wn + gx;
                a.next_p[at] = (float)((((double)sp[2 * py][2 * px] + sp[2 * py][2 * px + 1]) + sp[2 * py + 1][2 * px] + sp[2 * py + 1][2 * px + 1]) * 0.25);
                a.next_t[at] = (float)((((double)st[2 * py][2 * px] + st[2 * py][2 * px + 1]) + st[2 * py + 1][2 * px] + st[2 * py + 1][2 * px + 1]) * 0.25);
            }
        }
    }
    double g[MS_K];
#pragma unroll
    for (int k = 0; k < MS_K; ++k) g[k] = a.g[k];
    const int c = tid & (MS_T - 1), grp = tid >> 5;          // column pass: column c, output rows 2 grp and 2 grp + 1 of the strip
    double s_ssim = 0.0, s_cs = 0.0;
    for (int strip = 0; strip < MS_T / MS_STRIP; ++strip) {
        const int r0 = strip * MS_STRIP;
        if (strip) __syncthreads();                          // the previous strip's column pass has read R
        for (int i = tid; i < (MS_STRIP + MS_K - 1) * MS_T; i += 256) {
            const int r = i / MS_T, cc = i - r * MS_T;
            double mp = 0, mt = 0, epp = 0, ett = 0, ept = 0;
#pragma unroll
            for (int k = 0; k < MS_K; ++k) {
                const double p = sp[r0 + r][cc + k], t = st[r0 + r][cc + k], gp = g[k] * p, gt = g[k] * t;
                mp += gp; mt += gt; epp += gp * p; ett += gt * t; ept += gp * t;
            }
            R[0][r][cc] = mp; R[1][r][cc] = mt; R[2][r][cc] = epp; R[3][r][cc] = ett; R[4][r][cc] = ept;
        }
        __syncthreads();
        double acc[2][5] = {};
#pragma unroll
        for (int k = 0; k < MS_K + 1; ++k) {
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                const double v = R[m][2 * grp + k][c];
                if (k < MS_K) acc[0][m] += g[k] * v;
                if (k > 0) acc[1][m] += g[k - 1] * v;
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int y = y0 + r0 + 2 * grp + j, x = x0 + c;
            if (y < a.H - (MS_K - 1) && x < a.W - (MS_K - 1)) {
                const double mp = acc[j][0], mt = acc[j][1];
                const double vp = fmax(acc[j][2] - mp * mp, 0.0), vt = fmax(acc[j][3] - mt * mt, 0.0), cov = acc[j][4] - mp * mt;
                const double cs = (2.0 * cov + MS_C2) / (vp + vt + MS_C2);
                s_cs += cs;
                s_ssim += (2.0 * mp * mt + MS_C1) / (mp * mp + mt * mt + MS_C1) * cs;
            }
        }
    }
    s_ssim = wave_sum_d(s_ssim); s_cs = wave_sum_d(s_cs);
    if ((tid & 63) == 0) { red[0][tid >> 6] = s_ssim; red[1][tid >> 6] = s_cs; }
    __syncthreads();
    if (tid == 0) {
        double* o = a.part + (size_t)blockIdx.x * 2;         // [plane][tile][2]
        o[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        o[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

// One wave per image: folds the C * tiles partial pairs of every scale (lane l takes entries l, l + 64, ..., then the shuffle tree), takes the means,
// relu, and the product of the powers.
__global__ __launch_bounds__(64) void ms_ssim_fold_kernel(const MsFoldP a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double result = 1.0;
    for (int s = 0; s < MS_SCALES; ++s) {
        const long n = (long)a.C * a.ntile[s];
        const double* part = a.part + a.off[s] + (size_t)b * n * 2;
        double ss = 0.0, sc = 0.0;
        for (long i = lane; i < n; i += 64) { ss += part[2 * i]; sc += part[2 * i + 1]; }
        ss = fmax(wave_sum_d(ss) / a.count[s], 0.0);
        sc = fmax(wave_sum_d(sc) / a.count[s], 0.0);
        result *= pow(s == MS_SCALES - 1 ? ss : sc, a.beta[s]);
        if (a.table && lane == 0) { a.table[((size_t)b * MS_SCALES + s) * 2] = ss; a.table[((size_t)b * MS_SCALES + s) * 2 + 1] = sc; }
    }
    if (lane == 0) a.out[b] = result;
}

extern "C" void car_launch_ms_ssim_scale(const MsScaleP* p, long planes, hipStream_t st) {
    hipLaunchKernelGGL(ms_ssim_scale_kernel, dim3((unsigned)(planes * p->tiles_x * p->tiles_y)), dim3(256), 0, st, *p);
}
extern "C" void car_launch_ms_ssim_fold(const MsFoldP* p, int B, hipStream_t st) {
    hipLaunchKernelGGL(ms_ssim_fold_kernel, dim3(B), dim3(64), 0, st, *p);
}

// ------------------------------------------------------------------------------------- F1
__device__ inline bool is_positive(float v, int rule, float value) { return rule == MT_RULE_EQ ? v == value : v > value; }

// grid (chunks, B): a block counts TP, FP, FN over its chunk of one image: part [B][chunks][3]
__global__ __launch_bounds__(256) void f1_count_kernel(const void* pred, int dt_p, int rule_p, float val_p, const void* tgt, int dt_t, int rule_t, float val_t,
                                                       long HW, long chunk, unsigned long long* part) {
    __shared__ unsigned long long sm[3][4];
    const size_t base = (size_t)blockIdx.y * HW;
    const long i0 = (long)blockIdx.x * chunk, i1 = i0 + chunk < HW ? i0 + chunk : HW;
    unsigned tp = 0, fp = 0, fn = 0;                         // a thread sees chunk / 256 elements: far below 2^32
    for (long i = i0 + threadIdx.x; i < i1; i += 256) {
        const bool p = is_positive(ld_pix(pred, dt_p, base + i), rule_p, val_p), t = is_positive(ld_pix(tgt, dt_t, base + i), rule_t, val_t);
        tp += p && t; fp += p && !t; fn += !p && t;
    }
    const unsigned long long v[3] = {wave_sum_u64(tp), wave_sum_u64(fp), wave_sum_u64(fn)};
    if ((threadIdx.x & 63) == 0) for (int k = 0; k < 3; ++k) sm[k][threadIdx.x >> 6] = v[k];
    __syncthreads();
    if (threadIdx.x < 3) part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + threadIdx.x] = sm[threadIdx.x][0] + sm[threadIdx.x][1] + sm[threadIdx.x][2] + sm[threadIdx.x][3];
}
__global__ __launch_bounds__(64) void f1_fold_kernel(const unsigned long long* part, int chunks, long long* counts, double* f1) {
    const int b = blockIdx.x, lane = threadIdx.x;
    unsigned long long v[3] = {0, 0, 0};
    for (int i = lane; i < chunks; i += 64) for (int k = 0; k < 3; ++k) v[k] += part[((size_t)b * chunks + i) * 3 + k];
    for (int k = 0; k < 3; ++k) v[k] = wave_sum_u64(v[k]);
    if (lane == 0) {
        if (counts) for (int k = 0; k < 3; ++k) counts[(size_t)b * 3 + k] = (long long)v[k];
        const unsigned long long den = 2 * v[0] + v[1] + v[2];
        if (f1) f1[b] = den ? (double)(2 * v[0]) / (double)den : 0.0;
    }
}
extern "C" void car_launch_f1(const void* pred, int dt_p, int rule_p, float val_p, const void* tgt, int dt_t, int rule_t, float val_t, int B, long HW,
                              long chunk, int chunks, unsigned long long* part, long long* counts, double* f1, hipStream_t st) {
    hipLaunchKernelGGL(f1_count_kernel, dim3(chunks, B), dim3(256), 0, st, pred, dt_p, rule_p, val_p, tgt, dt_t, rule_t, val_t, HW, chunk, part);
    hipLaunchKernelGGL(f1_fold_kernel, dim3(B), dim3(64), 0, st, part, chunks, counts, f1);
}

// ------------------------------------------------------------------------------------- RMSE
// grid (chunks, B): the maximum of a chunk of pred: pmax [B][chunks]
__global__ __launch_bounds__(256) void rmse_max_kernel(const float* pred, long HW, long chunk, float* pmax) {
    __shared__ float sm[17];
    const size_t base = (size_t)blockIdx.y * HW;
    const long i0 = (long)blockIdx.x * chunk, i1 = i0 + chunk < HW ? i0 + chunk : HW;
    float m = -INFINITY;
    for (long i = i0 + threadIdx.x; i < i1; i += 256) m = fmaxf(m, pred[base + i]);
    m = block_max(m, sm);
    if (threadIdx.x == 0) pmax[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = m;
}
// grid (chunks, B): sum of (pred * s - label)^2 over a chunk, s = 255 / max(pred of this image) from pmax, or 1: psum [B][chunks]
__global__ __launch_bounds__(256) void rmse_sq_kernel(const float* pred, const void* label, int dt_l, long HW, long chunk, const float* pmax, double* psum) {
    __shared__ float smf[17];
    __shared__ double smd[4];
    double s = 1.0;
    if (pmax) {
        float m = -INFINITY;
        for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) m = fmaxf(m, pmax[(size_t)blockIdx.y * gridDim.x + i]);
        s = 255.0 / (double)block_max(m, smf);
    }
    const size_t base = (size_t)blockIdx.y * HW;
    const long i0 = (long)blockIdx.x * chunk, i1 = i0 + chunk < HW ? i0 + chunk : HW;
    double acc = 0.0;
    for (long i = i0 + threadIdx.x; i < i1; i += 256) {
        const double d = (double)pred[base + i] * s - (double)ld_pix(label, dt_l, base + i);
        acc += d * d;
    }
    acc = block_sum_d(acc, smd);
    if (threadIdx.x == 0) psum[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}
__global__ __launch_bounds__(64) void rmse_fold_kernel(const double* psum, int chunks, long HW, double* out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double v = 0.0;
    for (int i = lane; i < chunks; i += 64) v += psum[(size_t)b * chunks + i];
    v = wave_sum_d(v);
    if (lane == 0) out[b] = sqrt(v / (double)HW);
}
extern "C" void car_launch_rmse(const float* pred, const void* label, int dt_l, int B, long HW, long chunk, int chunks, int use_max, float* pmax, double* psum,
                                double* out, hipStream_t st) {
    if (use_max) hipLaunchKernelGGL(rmse_max_kernel, dim3(chunks, B), dim3(256), 0, st, pred, HW, chunk, pmax);
    hipLaunchKernelGGL(rmse_sq_kernel, dim3(chunks, B), dim3(256), 0, st, pred, label, dt_l, HW, chunk, use_max ? pmax : (const float*)nullptr, psum);
    hipLaunchKernelGGL(rmse_fold_kernel, dim3(B), dim3(64), 0, st, psum, chunks, HW, out);
}

// ------------------------------------------------------------------------------------- save_image quantiser
// torchvision's save_image(normalize=True, value_range=(-1, 1)): clamp, (x + 1) / 2, * 255, + 0.5, clamp, truncate — each step rounded to fp32 on its
// own as torch's in-place ops round it (no fused multiply-add).  One thread per pixel: three planar reads, three interleaved bytes, three planar floats.
__global__ __launch_bounds__(256) void pixels_to_u8_kernel(const float* x, long HW, unsigned char* out_hwc, float* fout) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const size_t img = (size_t)blockIdx.y * 3 * HW;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float v = x[img + (size_t)ch * HW + i];
        v = fminf(fmaxf(v, -1.f), 1.f);
        v = __fadd_rn(v, 1.f) * 0.5f;
        v = __fadd_rn(__fmul_rn(v, 255.f), 0.5f);
        v = floorf(fminf(fmaxf(v, 0.f), 255.f));
        if (out_hwc) out_hwc[img + (size_t)i * 3 + ch] = (unsigned char)v;
        if (fout) fout[img + (size_t)ch * HW + i] = v;
    }
}
extern "C" void car_launch_pixels_to_u8(const float* x, int B, long HW, unsigned char* out_hwc, float* fout, hipStream_t st) {
    hipLaunchKernelGGL(pixels_to_u8_kernel, dim3((unsigned)((HW + 255) / 256), B), dim3(256), 0, st, x, HW, out_hwc, fout);
}
