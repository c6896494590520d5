// weight_pack.h — the host-side layouts car_load_tensor turns checkpoint tensors into, one function per layout.  Plain C++17 without a HIP include:
// tests/weight_pack_check.cpp builds it with the host compiler and tests/test_weight_pack_cpu.py checks every function against the PyTorch definition
// of the tensor.  Inputs are row-major fp32 as a state dict stores them; every function returns the packed fp32 image (the element type is applied at upload).
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

// K of an implicit-GEMM conv image, padded to the 32-wide k step of the conv kernels (hed.hip, lineart.hip)
inline int conv_kp(int K) { return (K + 31) / 32 * 32; }

// Conv2d weight OIHW [Co,Ci,kh,kw] -> implicit-GEMM image [Co][Kp], k = (ky*kw + kx)*Ci + ci; the tail of a row is zero where Kp > kh*kw*Ci
inline std::vector<float> pack_conv(const float* w, int Co, int Ci, int kh, int kw, int Kp) {
    const int T = kh * kw;
    std::vector<float> pk((size_t)Co * Kp, 0.f);
    for (int o = 0; o < Co; ++o) for (int ci = 0; ci < Ci; ++ci) for (int t = 0; t < T; ++t)
        pk[(size_t)o * Kp + (size_t)t * Ci + ci] = w[((size_t)o * Ci + ci) * T + t];
    return pk;
}

// ConvTranspose2d(3, stride 2, padding 1, output_padding 1) by output parity: output (2g + py, 2g' + px) of phase ph = 2*py + px.  Even parity takes
// kernel index 1 at input offset 0; odd parity takes index 2 at offset 0 and index 0 at offset +1 (zero beyond the edge): 1, 2, 2 and 4 taps.
// Returns the tap count of the phase; tap i reads the input at offset (dy[i], dx[i]) and, where asked for, kernel element (ky[i], kx[i]).
inline int convT_phase_taps(int ph, signed char* dy, signed char* dx, int* ky = nullptr, int* kx = nullptr) {
    const int py = ph >> 1, px = ph & 1, ny = py ? 2 : 1, nx = px ? 2 : 1;
    for (int a = 0; a < ny; ++a) for (int b = 0; b < nx; ++b) {
        const int i = a * nx + b;
        dy[i] = (signed char)a; dx[i] = (signed char)b;
        if (ky) ky[i] = py ? (a == 0 ? 2 : 0) : 1;
        if (kx) kx[i] = px ? (b == 0 ? 2 : 0) : 1;
    }
    return ny * nx;
}
// its weight [Ci,Co,3,3] -> the four phase images [Co][ntaps*Ci] (k = tap*Ci + ci), concatenated in the order ph = 0..3: 9*Co*Ci elements
inline std::vector<float> pack_convT_phases(const float* w, int Ci, int Co) {
    std::vector<float> pk((size_t)9 * Ci * Co);
    size_t o = 0;
    for (int ph = 0; ph < 4; ++ph) {
        signed char dy[4], dx[4]; int ky[4], kx[4];
        const int nt = convT_phase_taps(ph, dy, dx, ky, kx);
        for (int co = 0; co < Co; ++co) for (int i = 0; i < nt; ++i) for (int ci = 0; ci < Ci; ++ci)
            pk[o++] = w[(((size_t)ci * Co + co) * 3 + ky[i]) * 3 + kx[i]];
    }
    return pk;
}

// ConvTranspose2d(k, stride k) weight [Ci,Co,k,k] -> GEMM image [(ky*k + kx)*Co + co][ci]: every tap is a 1x1 conv onto its own output pixel
inline std::vector<float> pack_convT_taps(const float* w, int Ci, int Co, int k) {
    const int T = k * k;
    std::vector<float> pk((size_t)T * Co * Ci);
    for (int ci = 0; ci < Ci; ++ci) for (int co = 0; co < Co; ++co) for (int t = 0; t < T; ++t)
        pk[((size_t)t * Co + co) * Ci + ci] = w[((size_t)ci * Co + co) * T + t];
    return pk;
}
// and its bias [Co] replicated per tap: [k*k][Co]
inline std::vector<float> pack_convT_taps_bias(const float* b, int Co, int k) {
    std::vector<float> rep((size_t)k * k * Co);
    for (int t = 0; t < k * k; ++t) memcpy(&rep[(size_t)t * Co], b, (size_t)Co * 4);
    return rep;
}

// two [rows, cols] matrices -> [2*rows, cols], rows alternating in blocks of 16 (a's rows 0..15, b's rows 0..15, a's 16..31, ...): the gated GEMM
// epilogues see (gate, value) pairs.  rows is a multiple of 16.
inline std::vector<float> interleave16(const float* a, const float* b, int rows, int cols) {
    std::vector<float> pk((size_t)2 * rows * cols);
    for (int r = 0; r < rows; ++r) {
        const size_t blk = (size_t)(r / 16) * 32 + (r % 16);
        memcpy(&pk[blk * cols], &a[(size_t)r * cols], (size_t)cols * 4);
        memcpy(&pk[(blk + 16) * cols], &b[(size_t)r * cols], (size_t)cols * 4);
    }
    return pk;
}

// [rows, K] -> [rows, Kp], every row zero padded (the ViT patch projection: K = 3*p*p to a multiple of 32)
inline std::vector<float> pad_rows(const float* w, int rows, int K, int Kp) {
    std::vector<float> pk((size_t)rows * Kp, 0.f);
    for (int r = 0; r < rows; ++r) memcpy(&pk[(size_t)r * Kp], &w[(size_t)r * K], (size_t)K * 4);
    return pk;
}
