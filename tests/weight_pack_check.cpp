// Stand-alone driver of controlar_amd/csrc/weight_pack.h (tests/test_weight_pack_cpu.py builds it with the host compiler and compares every line with numpy
// written from the PyTorch definition of the tensor).  Every input is w[i] = i; one line per case: its name, then the packed values.
#include "../controlar_amd/csrc/weight_pack.h"

#include <cstdio>
#include <string>

static std::vector<float> iota(size_t n, float first = 0.f) {
    std::vector<float> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = first + (float)i;
    return v;
}
static void put(const std::string& name, const std::vector<float>& v) {
    printf("%s", name.c_str());
    for (float x : v) printf(" %.0f", x);
    printf("\n");
}

int main() {
    const int conv[4][4] = {{2, 3, 7, 160}, {2, 3, 3, 32}, {3, 32, 3, 288}, {1, 4, 7, 224}};      // Co, Ci, k, Kp
    for (auto& s : conv)
        put("conv_" + std::to_string(s[0]) + "_" + std::to_string(s[1]) + "_" + std::to_string(s[2]) + "_" + std::to_string(s[3]),
            pack_conv(iota((size_t)s[0] * s[1] * s[2] * s[2]).data(), s[0], s[1], s[2], s[2], s[3]));
    {
        const int Ci = 4, Co = 2;
        put("convT_phases_4_2", pack_convT_phases(iota((size_t)Ci * Co * 9).data(), Ci, Co));
        for (int ph = 0; ph < 4; ++ph) {          // per phase: tap count, then (dy, dx, ky, kx) of every tap
            signed char dy[4], dx[4]; int ky[4], kx[4];
            const int nt = convT_phase_taps(ph, dy, dx, ky, kx);
            std::vector<float> v = {(float)nt};
            for (int i = 0; i < nt; ++i) for (int x : {(int)dy[i], (int)dx[i], ky[i], kx[i]}) v.push_back((float)x);
            put("convT_phase_taps_" + std::to_string(ph), v);
        }
    }
    for (int k : {2, 4}) {
        const int Ci = 3, Co = 2;
        put("convT_taps_" + std::to_string(k), pack_convT_taps(iota((size_t)Ci * Co * k * k).data(), Ci, Co, k));
        put("convT_taps_bias_" + std::to_string(k), pack_convT_taps_bias(iota(Co).data(), Co, k));
    }
    for (int rows : {16, 48}) {
        const int cols = 5;
        put("interleave16_" + std::to_string(rows), interleave16(iota((size_t)rows * cols).data(), iota((size_t)rows * cols, (float)rows * cols).data(), rows, cols));
    }
    put("pad_rows_3_27_32", pad_rows(iota(3 * 27).data(), 3, 27, 32));
    return 0;
}
