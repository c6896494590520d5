// resample_tab.h — the coefficient tables of Pillow's 8-bit resampler (ImagingResample: precompute_coeffs + normalize_coeffs_8bpc), host only: plain
// C++ with no HIP dependence, so that a stand-alone program can exercise it (engine_resize.hip: car_resize, car_debug_resample_coeffs).
// Everything is evaluated in double, in Pillow's order of operations; the tables are what both passes of resample.hip consume.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

// Pillow's own filter codes (Image.Resampling): they are the ABI values of car_resize's `filter`
enum { RS_NEAREST = 0, RS_LANCZOS = 1, RS_BILINEAR = 2, RS_BICUBIC = 3, RS_BOX = 4, RS_HAMMING = 5 };
#define RS_PRECISION_BITS 22

static inline double rs_support(int filter) {
    switch (filter) {
        case RS_LANCZOS: return 3.0;
        case RS_BILINEAR: return 1.0;
        case RS_BICUBIC: return 2.0;
        case RS_BOX: return 0.5;
        case RS_HAMMING: return 1.0;
    }
    return 0.0;
}

static inline double rs_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return std::sin(x) / x;
}

static inline double rs_filter(int filter, double x) {
#ifdef __clang__
#pragma clang fp contract(off)      // the tables are compared bit for bit: no fused multiply-add
#endif
    switch (filter) {
        case RS_LANCZOS: return (-3.0 <= x && x < 3.0) ? rs_sinc(x) * rs_sinc(x / 3) : 0.0;
        case RS_BILINEAR: { if (x < 0.0) x = -x; return x < 1.0 ? 1.0 - x : 0.0; }
        case RS_BICUBIC: {
            const double a = -0.5;
            if (x < 0.0) x = -x;
            if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
            if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
            return 0.0;
        }
        case RS_BOX: return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
        case RS_HAMMING: {
            if (x < 0.0) x = -x;
            if (x == 0.0) return 1.0;
            if (x >= 1.0) return 0.0;
            x = x * M_PI;
            return std::sin(x) / x * (0.54 + 0.46 * std::cos(x));
        }
    }
    return 0.0;
}

static inline bool rs_filter_ok(int filter) { return filter >= RS_LANCZOS && filter <= RS_HAMMING; }

// taps per output index: ((int)ceil(support * max(scale, 1))) * 2 + 1.  Returned as a 64-bit value so that a caller can refuse an absurd scale first.
static inline long long rs_ksize(double in0, double in1, int outSize, int filter) {
    double filterscale = (in1 - in0) / outSize;
    if (filterscale < 1.0) filterscale = 1.0;
    return (long long)std::ceil(rs_support(filter) * filterscale) * 2 + 1;
}

// One axis: kk [outSize][ksize] fixed-point taps (22 fractional bits; taps past xmax are 0), bounds [outSize][2] = (xmin, xmax): output xx is
// (1 << 21) + sum_{x < xmax} in[xmin + x] * kk[xx][x], shifted right by 22 and clamped to 0..255.  0 <= xmin and xmin + xmax <= inSize always.
// Requires rs_filter_ok(filter), inSize > 0, outSize > 0, 0 <= in0 < in1 <= inSize.  Returns ksize.
static inline int rs_coeffs(int inSize, double in0, double in1, int outSize, int filter, std::vector<int32_t>& kk, std::vector<int32_t>& bounds) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double scale = (in1 - in0) / outSize;
    double filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = rs_support(filter) * filterscale;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    kk.assign((size_t)outSize * ksize, 0);
    bounds.assign((size_t)outSize * 2, 0);
    std::vector<double> w((size_t)ksize);
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < outSize; ++xx) {
        const double center = in0 + (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > inSize) xmax = inSize;
        xmax -= xmin;
        if (xmax < 0) xmax = 0;
        if (xmax > ksize) xmax = ksize;          // cannot happen (xmax - xmin <= 2*support + 1 <= ksize); keeps the table write in bounds regardless
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[(size_t)x] = rs_filter(filter, (x + xmin - center + 0.5) * ss);
            ww += w[(size_t)x];
        }
        int32_t* k = &kk[(size_t)xx * ksize];
        for (int x = 0; x < xmax; ++x) {
            double v = w[(size_t)x];
            if (ww != 0.0) v /= ww;
            k[x] = v < 0 ? (int32_t)(-0.5 + v * (1 << RS_PRECISION_BITS)) : (int32_t)(0.5 + v * (1 << RS_PRECISION_BITS));
        }
        bounds[(size_t)xx * 2] = xmin;
        bounds[(size_t)xx * 2 + 1] = xmax;
    }
    return ksize;
}
