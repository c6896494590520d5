"""Kernel-level parity on the GPU: the standalone harnesses under experiments/ check individual HIP kernels against host fp64 references of the same op
(the end-to-end tests compare whole stages with the oracle).  Each harness is one hipcc line; it is built here if the binary is missing or older than
its sources, then run in its quick mode."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "controlar_amd", "csrc")


def _build(name, extra=()):
    src = os.path.join(ROOT, "experiments", name + ".hip")
    exe = os.path.join(ROOT, "experiments", name)
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, *extra, src, "-o", exe], check=True, capture_output=True, timeout=900)
    return exe


def test_exact_mode_kernels_against_fp64_references():
    """decode_f32.hip (experiments/f32_check.hip, quick mode): dec_gemm_f32 on v_mfma_f32_16x16x4_f32 — every tile configuration and epilogue (plain, residual, SwiGLU,
    RoPE + q scale + K/V rows) within 2e-5 of an fp64 GEMM, bit-identical across tile configurations and between a row computed alone and inside a batch; the
    fixed-split fp32 attention within 2e-5 of an fp64 softmax(QK^T)V over masked / ragged prefixes at four positions and four batch sizes, bit-identical alone vs in a batch.
    Round 5: the LDS-tiled kernel dec_gemm_f32t (ten configurations: 1 / 2 / 4 / 8 K-groups, both stage depths) BIT-equal to the register kernel on every epilogue, plain and
    with the on-the-fly RMSNorm (itself within 2e-4 of an fp64 norm + GEMM); the one-launch attention forms (4-, 12-, 16-wave workgroups) bit-equal to split + combine."""
    exe = _build("f32_check")
    out = subprocess.run([exe, "quick"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout[-3000:] + out.stderr[-1000:]
    assert "BITS DIFFER" not in out.stdout and "FAIL" not in out.stdout


def test_fp8_decode_linears_against_a_reference_on_identical_codes():
    """dec_gemm<F8> (experiments/f8_check.hip): the e4m3 weight image pack.hip builds must hold exactly the round-to-nearest-even codes of w / (amax / 448), and
    both fp8 linears — weight-only (codes widened to bf16 in registers) and W8A8 (activations quantised to e4m3 in registers, v_mfma_f32_16x16x32_fp8_fp8) — must
    reproduce an fp64 product of THOSE codes (W8A8: with the activations quantised on the host by the reference rounding, ties and values beyond 448 included) to
    the one bf16 ulp of the epilogue, for K = 1280 / 3584 and one / several m-blocks.  At whole-model level two W8A8 implementations decorrelate within three
    layers (tests/test_configs_gpu.py); on identical inputs nothing does, so this is the check that pins the kernel."""
    exe = _build("f8_check")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout[-3000:] + out.stderr[-1000:]
    assert "FAIL" not in out.stdout


def test_nhwc_conv_kernels_against_exact_integer_references():
    """hed.hip, dpt.hip, lineart.hip (experiments/nhwc_conv_check.hip, quick mode): car_launch_hed_conv, car_launch_dpt_conv and car_launch_la_conv called directly on
    small-integer operands, where every product and sum is exact in fp32, so the expected output has no tolerance — fp32 mode bit-equal to the host's integer
    convolution, bf16 mode to its bf16 rounding, side partials and the DPT map to the exact sums of the rounded channels.  Two images per case, both modes, two runs
    with equal bits; partial / tail / exact tiles, the pool over an odd map, the Cin = 3 element-wise gather, a half-masked channel tile, stride 2 on odd and even
    maps, residual addends, the folded projection, reflection, a transposed-conv phase; every refusal of the launchers returns hipErrorInvalidValue."""
    exe = _build("nhwc_conv_check")
    out = subprocess.run([exe, "quick"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout[-3000:] + out.stderr[-1000:]
    assert "BITS DIFFER" not in out.stdout and "FAIL" not in out.stdout


def test_generic_gemm_and_conv_kernels_against_exact_integer_references():
    """gemm.hip (experiments/gemm_check.hip, quick mode, built with -DCAR_DEV_KNOBS so that the CAR_* switches really select the alternate routes): every kernel
    family behind car_launch_gemm through the real launcher, each case asserting its car_gemm_route value first — gemm_bf16_kernel, gemm_bf16_glds_kernel (tiles == 512
    exactly, 8 and 9 ring stages, and one batch fewer on the register kernel), conv3_halo64_kernel, conv3_halo_kernel (CAR_CONV_HALO128), gemm_f32_mfma_kernel,
    gemm_f32_kernel.  Operands are small hashed integers whose products and sums are exact (the harness checks the condition per output element), so the whole output
    allocation — values, ldc gap columns, batch gaps, guards, all poisoned — is compared with memcmp: plain / batched / 3x3 / stride-2 / folded-upsample gathers over
    ragged tiles, patch and linear row order, EP_VEC and EP_SCALAR with bias_n / bias_m / scale / residual / alpha, bf16 and fp32 stores, one dense case per
    epilogue path (EP_VEC, EP_SCALAR, EP_SWIGLU) with sums far beyond 8 bits that replays the documented order of the rounding points, a bias pointer with BIAS_NONE, the GroupNorm partials of the halo epilogue bit-equal to integer sums of the stored
    values and to gn_partial_vec_kernel's totals, every refusal (gn_part, K % 32 / K % 16) returning its code and writing nothing.  Only the activations and SwiGLU
    have a bound, derived not measured: one bf16 ulp of the rounded fp64 function (SwiGLU: ulp(gate) |c| + ulp(out)) on at most 1 % of the elements, SiLU over |x| <= 30.5
    and the GELU forms over [-3.5, 30.5] (below -4.3 their fp32 form cancels).  Two runs, equal bits."""
    exe = _build("gemm_check", extra=("-DCAR_DEV_KNOBS",))
    out = subprocess.run([exe, "quick"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout[-3000:] + out.stderr[-1000:]
    assert "BITS DIFFER" not in out.stdout and "FAIL" not in out.stdout


def test_batched_attention_against_exact_and_fp64_references():
    """attn_run (engine_attn.hip) driven by experiments/attn_check.hip (quick mode, built with -DCAR_DEV_KNOBS so that CAR_NO_FLASH is live; that switch is read once
    per process, hence two invocations): flash64_kernel<QT, MODE> in the bf16 mode, transpose_pad -> car_launch_gemm -> softmax_wave / softmax_reg / softmax /
    t5_softmax kernel -> car_launch_gemm in the exact mode (first run) and in the bf16 mode (second run).  H = 2, nb = 3, T in {1, 15, 16, 17, 31, 32, 33, 63, 64, 65,
    120, 128, 129, 192, 193, 197, 257}, all three mask kinds at every T, both input layouts (ld = D, ld = 3D), 40 x 70 straight through car_launch_flash64; every case
    on a poisoned arena of which everything but out and the scratch planes is compared with memcmp, V^T and P pad columns zero, two runs with equal bits.  No
    tolerance: Q = 0 with integer V (every row one of the three candidate 1 / count: pins the attended set under left / right padding, holes, a fully masked
    sequence — T5: uniform over all keys in both forms — and a 0 / -128 bias per head and query), one-hot scores whose keys are >= 128 apart (the output is the bits
    of the winner's V row, winners at 0 / 15 / 16 / 31 / 32 / 33 / T - 1, losers +-3e38), softmax_reg_kernel == softmax_kernel, window invariance of the wave and
    register softmax for c in {16, 48}, every refusal of car_launch_flash64 and its way through attn_run.  Dense integer Q, K and bf16 V, bias against an fp64 softmax on
    every element under the bound derived in the harness header from the rounding points of each form (the exact mode's at fp32 level)."""
    exe = _build("attn_check", extra=("-DCAR_DEV_KNOBS",))
    for env in ({}, {"CAR_NO_FLASH": "1"}):
        out = subprocess.run([exe, "quick"], capture_output=True, text=True, timeout=600, env={**os.environ, **env})
        assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout[-3000:] + out.stderr[-1000:]
        assert "BITS DIFFER" not in out.stdout and "FAIL" not in out.stdout
        assert ("CAR_NO_FLASH" in out.stdout) == bool(env)


def test_bf16_decode_kernels_against_exact_integer_references():
    """decode2.hip (experiments/decode_check.hip, quick mode): dec_gemm_kernel, rmsnorm2_kernel and the two writers of the packed KV cache (the EPI_QKV epilogue,
    prefill_rope_kv2_kernel) through the real launchers, every dec_gemm case asserting its car_dec_gemm_route value (I, J, WAVES, F8, NORM) first.  Operands are
    small hashed integers (times a power of two), wscale rows powers of two, RoPE tables dyadic pairs: every partial sum is exact in fp32 (checked per output
    element, the sums of squares behind ssq_out included), so the reference — the documented bf16 / e4m3 rounding points replayed on exact sums — has one possible
    result, and the WHOLE poisoned arena of a case is compared with memcmp: outputs, inputs, guards, cache rows at positions other than *pos, rows >= M of the packed
    SwiGLU output, of ssq_out, h, outf and qout; rows >= M of a packed X hold NaNs.  Every tile shape (18 + the 16-wave one) x every epilogue x bf16 / e4m3 / W8A8
    weights (ties 17 -> 16, 19 -> 20 and values beyond 448 in the activations and in the e4m3 KV rows); M in {1, 2, 5, 16, 17, 50, 70}; K below the wave count,
    unevenly split, and deep enough for the refill branch to run more than once; grids with the XCD remap on and off; helper workgroups; both w_nt bits; EPI_RESID
    with and without ssq_out; EPI_QKV at positions 0 / 15 / 16 / 31 / 32 / 33 / SA - 1 with the prologue and the late read of *pos; every refusal returns non-zero and
    writes nothing.  Norm forms on sign rows +-2^a(m) (rnd(v rstd) = +-1 for every rstd within 2 ulp, so no tolerance): rmsnorm2 -> packed xn -> NORM 0 for
    D = 256 .. 4096, NORM 1 with gather / control add / nh_out, NORM 2 on every tile and NORM 3 for K = 256 / 768 / 1280, their partials written by a preceding
    EPI_RESID launch.  Integer rows in [-8, 8]: every rmsnorm2 row equals the row of ONE of the three candidate rstd values (the correctly rounded 1/sqrt and its
    neighbours: rsqrtf's documented 1 ulp), and NORM 1 / 2 / 3 are bit-equal to rmsnorm2 followed by NORM 0 of the same tile shape.  The prefill writer for Tn in
    {1, 33, 40} x t0 in {0, 7, 32}, and a decode-time row that must land behind it.  One-hot attention (H = 2, SA = 96, T = 40, b in {1, 8, 17}): q = 16 e_d and
    K_p[d] = 8 make one attended position win by >= 128, every other probability is exactly 0 and the output must be the bits of V_p — bf16 and e4m3 caches under
    every variant, dec_attn2s (162) with and without helpers, the persistent grid, packed output, nsplit 1 / 4, masks with holes through the in-kernel scan; masked
    and never-written rows hold +-3e38 / +-448.  The only bound is SwiGLU's, derived in gemm_check.hip: ulp(gate) |c| + ulp(out) from the rounded fp64 function on
    at most 1 % of the elements."""
    exe = _build("decode_check")
    out = subprocess.run([exe, "quick"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout[-3000:] + out.stderr[-1000:]
    assert "BITS DIFFER" not in out.stdout and "FAIL" not in out.stdout


def test_helper_kernels_against_exact_and_fp64_references():
    """ops.hip and t5.hip (experiments/ops_check.hip, quick mode, built with -DCAR_DEV_KNOBS so that CAR_GN_SCALAR is live; the harness sets it per case): the helper
    kernels in front of every stage through their real car_launch_* entry points — GroupNorm (gn_partial / gn_partial_vec / gn_finalize / gn_apply / gn_apply_vec),
    vq_argmin, vq_lookup, conv_out (scalar and MFMA form), conv_in3, rmsnorm_kernel, layernorm_kernel, swiglu, swiglu_parts, t5_gated_act, convert, build_text,
    gather_rows, label_index, t5_prep, patchify, vit_assemble, ctrl_scale_rows, row_mix_scale, set_pos_step, advance.  Every case on one arena poisoned with 0xff,
    256 guard bytes between the buffers, the WHOLE arena compared with the expected image (outputs, unchanged inputs, guards), two images / several rows with
    different data, both modes, two runs with equal bits, every pointer's byte extent asserted on the host before the launch.  No tolerance wherever the arithmetic
    is exact: stage-1 GroupNorm partials of hashed integers for HW in {1, 64, 255, 256, 257, 600} x C in {32 .. 512, 96, 320} (vector == scalar kernel), sign rows
    +-2^a(b, g) through stages 2 and 3 (mean 0, rstd 2^-a, y = +-gamma + beta; CAR_GN_SCALAR bit-equal to the vector route; have_part; y == nullptr; the stride
    loop twice); vq_argmin on a dyadic codebook (distances exactly 0 / 2 / 4) with the winner at 0 / 63 / 64 / 255 / 256 / 257 / ncode - 1 for ncode in {1, 5, 64,
    255, 256, 257, 1000, 16384}, exact ties (the lower index wins across lanes, waves and iterations), an all-zero row, and NaN / inf rows whose token must be 0
    — torch.argmin's answer; the kernel used to return 0x7fffffff there; conv_out on integer operands with asymmetric weights (MFMA form == scalar form == the
    integer convolution, H x W in {1x1, 5x7, 16x16, 17x33, 31x16}); conv_in3 with 257 -> 256 and 259 -> 260; rmsnorm_kernel for D in {64 .. 8192} (the second
    register group included) with gather, the three add modes, split-K parts of 1 / 3 / 4 / 5 / 8 / 9 slices, h_out and xn present or absent: every row bit-equal
    to the row of one of the three candidate rstd values, sign rows to the only one; layernorm on sign rows around an integer centre; the block-16 interleaved
    SwiGLU / GELU layout on saturated integer gates; all 65536 bf16 patterns (x 17 low halves) through convert against the harness's own rounding; clamps, flags,
    -0, NaN payloads, windows and dyadic bicubic weights in the copy and index kernels.  Bounds are derived in the harness header, never measured: swish (expf's
    ulp), dense GroupNorm statistics at mean/std 0 / 4 / 16 against a two-pass fp64 reference (profiles/ops_check_quick.txt holds the measured ratios), dense
    argmin (the token within (2 cd + 16) 2^-23 of the fp64 minimum, equal to the fp64 argmin wherever the runner-up is further away), vq_lookup, layernorm,
    SwiGLU (gemm_check.hip's rule)."""
    exe = _build("ops_check", extra=("-DCAR_DEV_KNOBS",))
    out = subprocess.run([exe, "quick"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout[-3000:] + out.stderr[-1000:]
    assert "BITS DIFFER" not in out.stdout and "FAIL" not in out.stdout
