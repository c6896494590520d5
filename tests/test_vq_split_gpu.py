"""GPU: the split-bf16 VQ decoder (car_config.vq_split_bf16, Engine(cfg, "fp32", vq_split=True)).  The kernel alone on operands whose
result is exact (experiments/split_gemm_check.hip), then the decoder end to end: against the reference's pixels within the EXACT decoder's bound
(max <= 2e-3, mean <= 1e-4: tests/test_parity_gpu.py, test_configs_gpu.py, test_bench_shapes_gpu.py hold the fp32 decoder to it on these goldens; the
reference arithmetic with every Conv2d operand split this way is 8.6e-5 / 1.1e-5 away on the CPU, a split that loses one cross term 0.028 / 4.0e-3),
that it is neither the fp32 nor the bf16 path in disguise, batch invariance, the fall-back of ineligible layers, and that nothing but car_vq_decode
sees the flag."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests.cases import GOLDEN, load_case, record_measured

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "controlar_amd", "csrc")
ATOL, MTOL = 2e-3, 1e-4


def _build(name, extra=()):
    src = os.path.join(ROOT, "experiments", name + ".hip")
    exe = os.path.join(ROOT, "experiments", name)
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, *extra, src, "-o", exe], check=True, capture_output=True, timeout=900)
    return exe


def test_split_kernels_against_exact_integer_references():
    """gemm_split.hip (experiments/split_gemm_check.hip): gemm_f32s_kernel through car_launch_gemm on integer-valued operands whose split products and sums
    are exact in fp32, compared with == against the host's integer reference — A with at most 8 significant bits against W with 9-16 (needs the A-hi·W-lo
    term), the mirror image, and both with 9 or more bits against the three-term sum hi·hi + hi·lo + lo·hi (which differs from the exact product by the
    lo·lo left out).  Plain with bias, residual and alpha over partial m- and n-tiles, the batched form, three convolutions (every pixel on a border; two
    m-tiles with the second nearly empty; the folded x2 upsample), nothing written past the end of the output, and an ineligible call (Cin = 16) whose
    bits do not depend on the flag."""
    exe = _build("split_gemm_check")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout[-3000:] + out.stderr[-1000:]
    assert "FAIL" not in out.stdout


def _vq_engine(vq, prec="fp32", seed=2, **kw):
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    cfg = C.tiny_t2i(64, "canny"); cfg.vq = vq
    eng = Engine(cfg, prec, **kw)
    eng.load_state_dict(synth.vq_state_dict(cfg.vq, seed=seed), finalize=True)
    return eng


@pytest.fixture(scope="module")
def split16():
    """one fp32 context with the option on and the real VQ-16 decoder (ch = 128, z = 256, 16384 x 8 codebook), shared by the tests that only decode"""
    from controlar_amd import config as C
    eng = _vq_engine(C.VQConfig(), vq_split=True)
    yield eng
    eng.close()


def test_vq16_real_8x8_within_the_exact_decoders_bound_and_on_its_own_path(split16):
    """vq16_real_8x8 (B = 2): within the fp32 bound of the reference's pixels — which the bf16 decoder (0.13-0.16 away) cannot reach — and not bit-equal
    to the exact fp32 decoder on the same tokens, so the split kernels did run."""
    from controlar_amd import config as C
    gold = np.load(os.path.join(GOLDEN, "vq16_real_8x8.npz"))
    toks = torch.from_numpy(gold["tokens"])
    px = split16.vq_decode(toks, 8, 8).cpu()
    d = np.abs(px.numpy() - gold["pixels"])
    print(f"vq16_8x8 split: max {d.max():.3e} mean {d.mean():.3e}")
    record_measured("vq16_8x8[fp32+vq_split]", max_abs_diff=d.max(), mean_abs_diff=d.mean())
    assert d.max() <= ATOL and d.mean() <= MTOL, (d.max(), d.mean())
    exact = _vq_engine(C.VQConfig())
    px32 = exact.vq_decode(toks, 8, 8).cpu()
    exact.close()
    dd = (px - px32).abs()
    print(f"vq16_8x8 split vs exact fp32 decoder: max {float(dd.max()):.3e}, {int((px != px32).sum())} of {px.numel()} elements differ")
    assert not torch.equal(px, px32)


def test_vq8_real_8x8_within_the_exact_decoders_bound():
    """The VQ-8 variant (vq_model.py:415-417), B = 2."""
    from controlar_amd import config as C
    gold = np.load(os.path.join(GOLDEN, "vq8_real_8x8.npz"))
    eng = _vq_engine(C.VQConfig(ch_mult=(1, 2, 2, 4)), seed=3, vq_split=True)
    px = eng.vq_decode(torch.from_numpy(gold["tokens"]), 8, 8).cpu().numpy()
    eng.close()
    d = np.abs(px - gold["pixels"])
    print(f"vq8_8x8 split: max {d.max():.3e} mean {d.mean():.3e}")
    record_measured("vq8_8x8[fp32+vq_split]", max_abs_diff=d.max(), mean_abs_diff=d.mean())
    assert d.max() <= ATOL and d.mean() <= MTOL, (d.max(), d.mean())


def test_vq16_real_512_in_batch_chunks(split16):
    """32 x 32 tokens -> 512 x 512 pixels, B = 17 = the fp32 activation chunk + 1, the golden tokens in the first and the last row (the second chunk holds
    one image), as tests/test_bench_shapes_gpu.py::test_vq16_real_512_in_batch_chunks has it for the exact decoder."""
    gold = np.load(os.path.join(GOLDEN, "vq16_real_32x32.npz"))
    B = 17
    g = torch.Generator().manual_seed(21)
    toks = torch.randint(0, split16.cfg.vq.codebook_size, (B, 1024), generator=g, dtype=torch.int32)
    toks[0] = torch.from_numpy(gold["tokens"][0]); toks[B - 1] = torch.from_numpy(gold["tokens"][1])
    px = split16.vq_decode(toks, 32, 32)
    assert bool(torch.isfinite(px).all())
    for row, gi in ((0, 0), (B - 1, 1)):
        p = px[row].cpu().numpy()
        for name, got in (("lattice", p[:, ::8, ::8]), ("corner", p[:, :24, :24]), ("centre", p[:, 244:268, 244:268])):
            d = np.abs(got - gold[name][gi])
            print(f"vq16_512 split row {row} {name}: max {d.max():.3e} mean {d.mean():.3e}")
            record_measured(f"vq16_512[fp32+vq_split,row{row},{name}]", max_abs_diff=d.max(), mean_abs_diff=d.mean())
            assert d.max() <= ATOL and d.mean() <= MTOL, (row, name, d.max(), d.mean())


def test_pixels_do_not_depend_on_the_batch_or_the_row(split16):
    """B = 3 at 8 x 8 tokens with rows 0 and 2 holding the same tokens: equal bits; a second call and a B = 1 call on that row give the same bits."""
    g = torch.Generator().manual_seed(33)
    toks = torch.randint(0, split16.cfg.vq.codebook_size, (3, 64), generator=g, dtype=torch.int32)
    toks[2] = toks[0]
    px = split16.vq_decode(toks, 8, 8).cpu()
    assert torch.equal(px[0], px[2]) and not torch.equal(px[0], px[1])
    assert torch.equal(split16.vq_decode(toks, 8, 8).cpu(), px)
    assert torch.equal(split16.vq_decode(toks[:1], 8, 8).cpu()[0], px[0])


def test_a_decoder_with_an_ineligible_layer_falls_back_to_exact_fp32_there():
    """z_channels = 16: conv_in (Cin = 16, no multiple of 32) is refused by the one predicate and runs on the exact fp32 kernel inside an otherwise split
    decode, which must stay within the bound of the exact decoder's pixels for the same tokens.  (A decoder in which NO layer is eligible does not exist:
    GroupNorm(32) needs every normalised channel count to be a multiple of 32 — with ch = 24 the reference raises and the GroupNorm kernels here would
    divide by zero channels per group — so every convolution behind a norm is eligible.  That a refused call is bit-equal with and without the flag is
    checked on the kernel itself, the Cin = 16 case of experiments/split_gemm_check.hip.)"""
    from controlar_amd import config as C
    vq = C.VQConfig(codebook_size=1024, z_channels=16, ch=32)
    g = torch.Generator().manual_seed(5)
    toks = torch.randint(0, vq.codebook_size, (2, 16), generator=g, dtype=torch.int32)
    out = []
    for split in (False, True):
        eng = _vq_engine(vq, seed=3, vq_split=split)
        out.append(eng.vq_decode(toks, 4, 4).cpu())
        eng.close()
    d = (out[0] - out[1]).abs()
    print(f"z_channels 16, split vs exact: max {float(d.max()):.3e} mean {float(d.mean()):.3e}")
    assert bool(torch.isfinite(out[1]).all()) and float(d.max()) <= ATOL and float(d.mean()) <= MTOL, (float(d.max()), float(d.mean()))
    assert not torch.equal(out[0], out[1])          # the eligible layers did take the split kernel


def test_the_flag_reaches_nothing_but_vq_decode():
    """A context that also holds the tiny GPT, option on: tiny_canny_cfg1's greedy tokens are the golden's bit for bit, and vq_encode returns the golden
    indices of vq_encode_tiny."""
    from controlar_amd import synth
    from controlar_amd.engine import Engine
    cs = load_case("tiny_canny_cfg1"); gold = cs["gold"]
    eng = Engine(cs["cfg"], "fp32", vq_split=True)
    eng.load_state_dict(cs["gsd"]); eng.load_state_dict(cs["vsd"]); eng.finalize()
    eng.encode_control(cs["img"].cuda())
    mask = cs["mask"].cuda() if cs["mask"] is not None else None
    toks = eng.generate(cs["emb"].cuda(), cs["n_new"], mask, cfg_scale=cs["cfg_scale"], cfg_interval=cs["cfg_interval"], control_strength=cs["control_strength"])
    assert np.array_equal(toks.cpu().numpy(), gold["tokens"])
    eng.close()
    egold = np.load(os.path.join(GOLDEN, "vq_encode_tiny.npz"))
    eng = Engine(cs["cfg"], "fp32", vq_split=True)
    eng.load_state_dict(synth.vq_state_dict(cs["cfg"].vq, seed=int(egold["meta"][3])), finalize=True)
    img = synth.smooth_control(2, 128, 128, seed=77) + 0.1 * synth.canny_like_control(2, 128, 128, seed=78)
    assert np.array_equal(eng.vq_encode(img.cuda()).cpu().numpy(), egold["tokens"])
    eng.close()


def test_dropin_vqmodel_honours_engine_options():
    """models.VQModel in fp32 with engine_options = {"vq_split": True} decodes vq16_real_8x8 within the same bound, on a context that has the option set;
    a bf16 engine refuses the option."""
    from controlar_amd import config as C, models as M, synth
    from controlar_amd.engine import Engine
    gold = np.load(os.path.join(GOLDEN, "vq16_real_8x8.npz"))
    vq = M.VQ_models["VQ-16"]()
    vq.load_state_dict(synth.vq_state_dict(vq.vq, seed=2))
    vq.engine_options = {"vq_split": True}
    toks = torch.from_numpy(gold["tokens"]).cuda()
    px = vq.decode_code(toks, [toks.shape[0], vq.vq.codebook_embed_dim, 8, 8]).cpu().numpy()
    assert vq.engine._cc.vq_split_bf16 == 1 and vq.engine.precision == "fp32"
    d = np.abs(px - gold["pixels"])
    assert d.max() <= ATOL and d.mean() <= MTOL, (d.max(), d.mean())
    with pytest.raises(ValueError, match="vq_split"):
        Engine(C.tiny_t2i(), "bf16", vq_split=True)
