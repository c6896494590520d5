// gemm_gather.h — what every GEMM kernel of gemm.hip / gemm_split.hip shares (device code only): the generic epilogue (epi_value) and the A-operand
// gather (make_arow / a_off: plain rows, or the implicit-GEMM 3x3 gather over NHWC activations with zero padding and the optional folded x2 upsample).
#pragma once
#include "car_common.h"

template <typename T>
__device__ __forceinline__ float epi_value(const GemmP& p, const T* bias, const T* scale, const T* R, long zR, int m, long mrow, int n, float v) {
    v *= p.alpha;
    if (p.bias_mode == BIAS_N) v += ET<T>::ld(bias + n);
    else if (p.bias_mode == BIAS_M) v += ET<T>::ld(bias + m);
    v = ET<T>::rnd(v);
    if (p.act == ACT_GELU_ERF) v = ET<T>::rnd(gelu_erf_f(v));
    else if (p.act == ACT_GELU_TANH) v = ET<T>::rnd(gelu_tanh_f(v));
    else if (p.act == ACT_SILU) v = ET<T>::rnd(silu_f(v));
    else if (p.act == ACT_QUICK_GELU) v = ET<T>::rnd(quick_gelu_f(v));
    if (scale) v = ET<T>::rnd(v * ET<T>::ld(scale + n));
    if (R) v = ET<T>::rnd(v + ET<T>::ld(R + zR + mrow * p.ldr + n));
    return v;
}

// ---- A-operand row descriptor (per thread, constant over the K loop)
struct ARow { long base; int y, x; bool ok; };

struct Geo { int M, Cin, Ho, Wo, ups; long lda; int patch; };
// patch order: m = ((b * (Ho/16) + ty) * (Wo/16) + tx) * 256 + py * 16 + px  ->  pixel (b, ty*16 + py, tx*16 + px)
__device__ inline void patch_decode(int Ho, int Wo, int m, int& b, int& y, int& x) {
    const int tw = Wo >> 4, th = Ho >> 4, tile = m >> 8, within = m & 255;
    b = tile / (tw * th); const int t2 = tile - b * (tw * th), ty = t2 / tw, tx = t2 - ty * tw;
    y = ty * 16 + (within >> 4); x = tx * 16 + (within & 15);
}
// row of C / R that GEMM row m addresses (the NHWC pixel index under patch order, m itself otherwise)
__device__ __forceinline__ long out_row(const GemmP& p, int m) {
    if (!p.patch) return m;
    int b, y, x; patch_decode(p.Ho, p.Wo, m, b, y, x);
    return ((long)b * p.Ho + y) * p.Wo + x;
}
template <int AMODE>
__device__ inline ARow make_arow(const Geo p, int m) {
    ARow r; r.ok = m < p.M; r.base = 0; r.y = 0; r.x = 0;
    if (AMODE == AMODE_PLAIN) { r.base = (long)m * p.lda; }
    else {
        const int hw = p.Ho * p.Wo;
        int b = m / hw; const int rem = m - b * hw;
        r.y = rem / p.Wo; r.x = rem - r.y * p.Wo;
        if (AMODE == AMODE_CONV3 && p.patch) patch_decode(p.Ho, p.Wo, m, b, r.y, r.x);
        if (AMODE == AMODE_CONV3S2) r.base = (long)b * (p.Ho * 2) * (p.Wo * 2);
        else r.base = (long)b * (p.Ho >> p.ups) * (p.Wo >> p.ups);   // in pixels
    }
    return r;
}
// element offset of A[m, k] (k multiple of the chunk width), or -1 if the chunk is zero padding
template <int AMODE>
__device__ inline long a_off(const Geo p, const ARow r, int k) {
    if (!r.ok) return -1;
    if (AMODE == AMODE_PLAIN) return r.base + k;
    const int tap = k / p.Cin, c = k - tap * p.Cin;
    if (AMODE == AMODE_CONV3S2) {
        // Downsample (vq_model.py:382-396): F.pad(x, (0,1,0,1)) then conv3x3 stride 2, no padding: taps (2y+ty, 2x+tx), zero past the edge
        const int Hin = p.Ho * 2, Win = p.Wo * 2, yy = 2 * r.y + tap / 3, xx = 2 * r.x + tap % 3;
        if (yy >= Hin || xx >= Win) return -1;
        return (r.base + (long)yy * Win + xx) * p.Cin + c;
    }
    const int yy = r.y + tap / 3 - 1, xx = r.x + tap % 3 - 1;
    if (yy < 0 || yy >= p.Ho || xx < 0 || xx >= p.Wo) return -1;
    return (r.base + (long)(yy >> p.ups) * (p.Wo >> p.ups) + (xx >> p.ups)) * p.Cin + c;
}
// a_off<AMODE_CONV3> for a caller that walks k in order and keeps (tap, c) = (k / Cin, k % Cin) itself: no division per chunk, and no branch (the
// offset of a padded tap is computed and discarded), so that the loads around it stay in one basic block
__device__ __forceinline__ long a_off_conv3(const Geo p, const ARow r, int tap, int c) {
    const int yy = r.y + tap / 3 - 1, xx = r.x + tap % 3 - 1;
    const bool ok = r.ok & (yy >= 0) & (yy < p.Ho) & (xx >= 0) & (xx < p.Wo);
    const long o = (r.base + (long)(yy >> p.ups) * (p.Wo >> p.ups) + (xx >> p.ups)) * p.Cin + c;
    return ok ? o : -1;
}
