// gemm_split.hip — fp32 GEMM / 3x3 convolution at bf16 MFMA rate (car_config.vq_split_bf16, GemmP::split3).
// gfx950 has no TF32: every fp32 operand x is split into two bf16 numbers, hi = bf16(x) and lo = bf16(x - hi), and a product is taken as three
// v_mfma_f32_16x16x32_bf16 accumulating in fp32:  x·w ~ hi·lo + lo·hi + hi·hi  (lo·lo, about 2^-16 of the product, is left out).
// gemm_f32s_kernel keeps the contract of gemm_f32_mfma_kernel (gemm.hip): fp32 A gathered through make_arow / a_off, fp32 W[N][K], fp32 output through
// epi_value<float>, batch strides — on a 128 x 128 x 32 tile, four waves of 64 x 64 (4 x 4 accumulator fragments), two LDS stages, one barrier per chunk.
// The loader reads fp32 from global memory, splits in registers and writes four bf16 planes per stage (A-hi, A-lo, W-hi, W-lo; 128 rows of 32 k, 80-byte
// rows as ConvT<bf16_t>::LD): 40 KB per stage, 80 KB of dynamic LDS.  Per chunk a wave reads 16 fragments of 16 bytes and issues 48 MFMAs, in a fixed
// order; an output element sums its chunks in order of k whatever M is, so a row's result depends neither on the batch it is computed in nor on its
// place in that batch.  Weights are split on the fly: no second weight image.  No atomics.
#include "car_common.h"
#include "gemm_gather.h"
#include <type_traits>

// THE split (kernel and car_debug_split_bf16), on a pair of values, bf16 bits packed low | high << 16: hi = round-to-nearest-even bf16 of x, lo = RNE bf16 of
// x - float(hi) (that difference is exact in fp32).  Where hi is not finite — an inf, a NaN, a value that rounds to inf — the difference is +-inf or NaN and lo
// is zero, so an inf or a NaN stays what it is and does not become inf - inf.  The rounding is f2bf on the host and the hardware's v_cvt_pk_bf16_f32 on the
// device: the same RNE on every number (subnormals included: the kernels run with fp32 denormals on); only the payload of a NaN may differ, which no output shows.
__host__ __device__ __forceinline__ unsigned car_rne_bf16x2(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __bf16 bf2_t __attribute__((ext_vector_type(2)));
    typedef float f2_t __attribute__((ext_vector_type(2)));
    union { bf2_t v; unsigned u; } c; c.v = __builtin_convertvector((f2_t){a, b}, bf2_t);
    return c.u;
#else
    return (unsigned)f2bf(a) | ((unsigned)f2bf(b) << 16);
#endif
}
__host__ __device__ __forceinline__ void car_split_bf16x2(float x0, float x1, unsigned& hi, unsigned& lo) {
    hi = car_rne_bf16x2(x0, x1);
    float d0 = x0 - bf2f((bf16_t)(hi & 0xffffu)), d1 = x1 - bf2f((bf16_t)(hi >> 16));
    d0 = fabsf(d0) < INFINITY ? d0 : 0.f; d1 = fabsf(d1) < INFINITY ? d1 : 0.f;      // false for a NaN too
    lo = car_rne_bf16x2(d0, d1);
}

// Host-only: the split above on n values (tests).
extern "C" int car_debug_split_bf16(const float* x, int64_t n, uint16_t* hi, uint16_t* lo) {
    if (!x || !hi || !lo || n < 0) return -1;
    for (int64_t i = 0; i < n; i += 2) {
        unsigned h, l;
        car_split_bf16x2(x[i], i + 1 < n ? x[i + 1] : 0.f, h, l);
        hi[i] = (uint16_t)(h & 0xffffu); lo[i] = (uint16_t)(l & 0xffffu);
        if (i + 1 < n) { hi[i + 1] = (uint16_t)(h >> 16); lo[i + 1] = (uint16_t)(l >> 16); }
    }
    return 0;
}

#define GS_LD 40                        // row stride of a plane in elements (80 B: 16-byte aligned, off the 64-byte period) = ConvT<bf16_t>::LD
#define GS_PLANE (128 * GS_LD)          // one bf16 plane: 128 rows x 32 k
#define GS_STAGE (4 * GS_PLANE)         // A-hi | A-lo | W-hi | W-lo
#define GS_SMEM_BYTES (2 * GS_STAGE * 2)

// 8 consecutive fp32 -> 8 hi and 8 lo bf16, packed for one 16-byte LDS store each
__device__ __forceinline__ void gs_split8(const float4 a, const float4 b, uint4& hi, uint4& lo) {
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    unsigned h[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) car_split_bf16x2(v[2 * e], v[2 * e + 1], h[e], l[e]);
    hi = make_uint4(h[0], h[1], h[2], h[3]); lo = make_uint4(l[0], l[1], l[2], l[3]);
}

template <int AMODE, int UPS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void gemm_f32s_kernel(GemmP p) {       // two workgroups per CU (80 KB of LDS each): at most 256 registers
    extern __shared__ __attribute__((aligned(16))) unsigned char gs_smem[];
    bf16_t* const sm = (bf16_t*)gs_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q4 = lane >> 4, c16 = lane & 15;
    const int wm = wave >> 1, wn = wave & 1;
    const int z = blockIdx.z, z0 = z / p.nb1, z1 = z - z0 * p.nb1;
    const float* A = (const float*)p.A + z0 * p.sA0 + z1 * p.sA1;
    const float* W = (const float*)p.W + z0 * p.sW0 + z1 * p.sW1;
    const long zC = z0 * p.sC0 + z1 * p.sC1, zR = z0 * p.sR0 + z1 * p.sR1;
    const int m0 = blockIdx.y * 128, n0 = blockIdx.x * 128;
    // loader: two rows (lrow, lrow + 64) of each operand, 8 consecutive k (two 16-byte loads) of the 32-wide chunk
    const int lrow = tid >> 2, lk = (tid & 3) * 8;
    const Geo geo = { p.M, p.Cin, p.Ho, p.Wo, UPS, p.lda, 0 };
    ARow ar[2]; bool wok[2]; const float* wp[2];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        ar[v] = make_arow<AMODE>(geo, m0 + lrow + 64 * v);
        wok[v] = (n0 + lrow + 64 * v) < p.N;
        wp[v] = W + (wok[v] ? (long)(n0 + lrow + 64 * v) * p.ldw : 0L) + lk;      // a row past N reads row 0 and is zeroed
    }
    // register staging: the activations are prefetched TWO chunks ahead (two register sets; the 3x3 gather mostly misses the L2 of the XCD it runs on, and
    // one chunk of MFMAs does not cover that latency), the weights — one image that every workgroup reads — one chunk ahead
    // Every load is unconditional — a padded tap or a row past the end reads a valid address (the operand's first bytes) and is zeroed when it is split — so
    // the loads of a step issue back to back and the wait in front of the split leaves the far prefetch in flight.
    const int nk = p.K / 32;
    float4 ra[2][2][2], rb[2][2];
    bool oka[2][2];
    int tap = 0, c0 = 0;                                     // AMODE_CONV3: the chunk gload_a loads next is channels c0 .. c0 + 31 of tap `tap` (Cin % 32 == 0)
    // Both loaders clamp the chunk to the last one: the steps at the end of the loop prefetch it again (valid addresses, never stored) instead of branching.
    auto gload_a = [&](auto set, int kt) {                   // called for kt = 0, 1, 2, ... in order
        constexpr int S = decltype(set)::value;
        const int kc = kt < nk ? kt : nk - 1;
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const long o = AMODE == AMODE_PLAIN ? (ar[v].ok ? ar[v].base + kc * 32 + lk : -1L) : a_off_conv3(geo, ar[v], tap, c0 + lk);      // PLAIN: a_off's arithmetic
            oka[S][v] = o >= 0;
            const float* src = A + (o >= 0 ? o : 0);
            ra[S][v][0] = *(const float4*)src; ra[S][v][1] = *(const float4*)(src + 4);
        }
        if (AMODE != AMODE_PLAIN && kt + 1 < nk) { c0 += 32; if (c0 == p.Cin) { c0 = 0; ++tap; } }
    };
    auto gload_w = [&](int kt) {
        const int kc = kt < nk ? kt : nk - 1;
#pragma unroll
        for (int v = 0; v < 2; ++v) { rb[v][0] = *(const float4*)(wp[v] + (long)kc * 32); rb[v][1] = *(const float4*)(wp[v] + (long)kc * 32 + 4); }
    };
    auto keep = [](float4 x, bool ok) { return make_float4(ok ? x.x : 0.f, ok ? x.y : 0.f, ok ? x.z : 0.f, ok ? x.w : 0.f); };
    auto sstore = [&](auto set, int buf) {
        constexpr int S = decltype(set)::value;
        bf16_t* s = sm + buf * GS_STAGE + lk;
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            uint4 hi, lo;
            const int r = (lrow + 64 * v) * GS_LD;
            gs_split8(keep(ra[S][v][0], oka[S][v]), keep(ra[S][v][1], oka[S][v]), hi, lo);
            *(uint4*)(s + r) = hi; *(uint4*)(s + GS_PLANE + r) = lo;
            gs_split8(keep(rb[v][0], wok[v]), keep(rb[v][1], wok[v]), hi, lo);
            *(uint4*)(s + 2 * GS_PLANE + r) = hi; *(uint4*)(s + 3 * GS_PLANE + r) = lo;
        }
    };
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // chunk kt of A lives in register set kt & 1 and in LDS stage kt & 1
    auto step = [&](auto par, int kt) {
        constexpr int P = decltype(par)::value;              // = kt & 1
        gload_w(kt + 1);                                     // issued before the far prefetch: the wait in front of sstore leaves the loads of chunk kt + 2 in flight
        gload_a(std::integral_constant<int, P>{}, kt + 2);   // set P is free: chunk kt went to LDS during step kt - 1
        // fragments: lane (c16, q4) holds k = 8 q4 .. 8 q4 + 7 of row c16 of each 16-row block.  W is the MFMA's first operand: a lane's four accumulator
        // registers are four consecutive n of one m (16-byte stores), as in gemm_f32_mfma_kernel
        const bf16_t* s = sm + P * GS_STAGE + c16 * GS_LD + q4 * 8;
        bf16x8 ah[4], al[4], wh[4], wl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ah[j] = *(const bf16x8*)(s + (wm * 64 + j * 16) * GS_LD);
            al[j] = *(const bf16x8*)(s + GS_PLANE + (wm * 64 + j * 16) * GS_LD);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            wh[i] = *(const bf16x8*)(s + 2 * GS_PLANE + (wn * 64 + i * 16) * GS_LD);
            wl[i] = *(const bf16x8*)(s + 3 * GS_PLANE + (wn * 64 + i * 16) * GS_LD);
        }
        // the fixed order of a chunk: the two cross terms, then hi·hi
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[i], al[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[i], ah[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[i], ah[j], acc[i][j], 0, 0, 0);
        if (kt + 1 < nk) sstore(std::integral_constant<int, 1 - P>{}, 1 - P);     // the other stage: its last readers passed the barrier that ended the previous chunk
        __syncthreads();
    };
    gload_a(std::integral_constant<int, 0>{}, 0); gload_w(0);
    gload_a(std::integral_constant<int, 1>{}, 1);
    sstore(std::integral_constant<int, 0>{}, 0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt += 2) {
        step(std::integral_constant<int, 0>{}, kt);
        if (kt + 1 < nk) step(std::integral_constant<int, 1>{}, kt + 1);
    }
    // epilogue of gemm_f32_mfma_kernel: lane (c16, q4) owns m = .. + c16 and n = .. + 4 q4 .. + 3 of every fragment
    const float* bias = (const float*)p.bias; const float* scale = (const float*)p.scale; const float* R = (const float*)p.R;
    const bool vec = (p.ldc & 3) == 0 && ((zC & 3) == 0) && (((uintptr_t)p.C & 15) == 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + wm * 64 + j * 16 + c16;
        if (m >= p.M) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + wn * 64 + i * 16 + q4 * 4;
            if (n >= p.N) continue;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (n + r < p.N) ? epi_value<float>(p, bias, scale, R, zR, m, (long)m, n + r, acc[i][j][r]) : 0.f;
            float* dst = (float*)p.C + zC + (long)m * p.ldc + n;
            if (vec && n + 3 < p.N) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
            else { for (int r = 0; r < 4; ++r) if (n + r < p.N) dst[r] = v[r]; }
        }
    }
}

// host -----------------------------------------------------------------------------------
// ONE predicate decides whether an fp32 call with GemmP::split3 takes gemm_f32s_kernel: whole 32-wide chunks (for a convolution inside one tap), and the
// 16-byte alignment and stride rules of the fp32 MFMA path.  Everything else stays on the exact fp32 kernels of gemm.hip — never less accurate.
extern "C" int car_gemm_split_ok(int amode, const GemmP* pp) {
    const GemmP& p = *pp;
    if (!(amode == AMODE_PLAIN || (amode == AMODE_CONV3 && (p.ups == 0 || p.ups == 1)))) return 0;      // AMODE_CONV3S2 is the encoder's
    return p.M > 0 && p.N > 0 && p.K >= 32 && p.K % 32 == 0 && p.ldw % 4 == 0 && ((uintptr_t)p.A & 15) == 0 && ((uintptr_t)p.W & 15) == 0 &&
           p.sA0 % 4 == 0 && p.sA1 % 4 == 0 && p.sW0 % 4 == 0 && p.sW1 % 4 == 0 && !p.gn_part && !p.swiglu &&
           (amode == AMODE_PLAIN ? p.lda % 4 == 0 : (p.Cin > 0 && p.Cin % 32 == 0 && p.K == 9 * p.Cin));
}
// launches gemm_f32s_kernel for a call car_gemm_split_ok accepted (nb0, nb1 >= 1).  The 80 KB of dynamic LDS need the attribute, once per device.
extern "C" hipError_t car_launch_gemm_split(int amode, const GemmP* pp, hipStream_t st) {
    static bool attr[16] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 16) return hipErrorInvalidDevice;
    if (!attr[dev]) {
        const void* ks[3] = { (const void*)gemm_f32s_kernel<AMODE_PLAIN, 0>, (const void*)gemm_f32s_kernel<AMODE_CONV3, 0>, (const void*)gemm_f32s_kernel<AMODE_CONV3, 1> };
        for (const void* k : ks)
            if ((e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, GS_SMEM_BYTES)) != hipSuccess) return e;
        attr[dev] = true;
    }
    const GemmP& p = *pp;
    const dim3 g((p.N + 127) / 128, (p.M + 127) / 128, p.nb0 * p.nb1);
    if (amode == AMODE_PLAIN) hipLaunchKernelGGL((gemm_f32s_kernel<AMODE_PLAIN, 0>), g, dim3(256), GS_SMEM_BYTES, st, p);
    else if (p.ups == 0) hipLaunchKernelGGL((gemm_f32s_kernel<AMODE_CONV3, 0>), g, dim3(256), GS_SMEM_BYTES, st, p);
    else hipLaunchKernelGGL((gemm_f32s_kernel<AMODE_CONV3, 1>), g, dim3(256), GS_SMEM_BYTES, st, p);
    return hipSuccess;
}
