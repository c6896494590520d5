#!/usr/bin/env python
"""Mint the DPT depth fixtures from the UNMODIFIED ``transformers.models.dpt.modeling_dpt.DPTForDepthEstimation`` (the class sample_t2i.py:33 imports).

Runs only where ``transformers`` imports.  The model is built from a ``DPTConfig`` made of ``controlar_amd.config.tiny_dpt()`` / ``tiny_dpt_wide()`` and
loaded with ``controlar_amd.synth.dpt_state_dict(cfg, seed)`` (regenerated from the seed, never committed).  Inputs are seeded uint8 images, stored as
uint8; ``pixel_values = (x/255 - 0.5)/0.5``, the image processor's rescale and normalise.

Each ``depth_<case>.npz`` holds
  x                      the input, uint8 [B,3,S,S]
  ref                    predicted_depth of the fp32 model, [B,S,S]
  ref_f32_vs_f64_max     max |ref - the same model in .double()|: the yardstick of the exact mode
  bf16_native_max/mean   max / mean |ref - the same model under .bfloat16() on the CPU|: the yardstick of the fast mode
  bf16_emul_max/mean     max / mean |ref - the fp32 model with every Conv2d / ConvTranspose2d / Linear input and weight rounded to bf16 (forward pre-hook)|:
                         an independent placement of the bf16 rounding points, the evidence that a second correct bf16 implementation fits the bound
  zero_share             share of ref == 0 (the final ReLU)

The conditions at the bottom of ``mint`` / ``check_all`` are asserted here and re-checked from the files by tests/test_depth_cpu.py.

usage: python tests/golden/make_depth_golden.py [--out DIR] [case ...]
"""
import argparse
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WEIGHT_SEED = 13
CASES = {            # name -> (config, B, S, input seed)
    "b2_32": ("tiny_dpt", 2, 32, 301),         # grid 2, the smallest legal size: the stride-2 stage is 1 x 1, pos-embed shrunk 4 -> 2; two images must not mix
    "b1_64": ("tiny_dpt", 1, 64, 302),         # grid 4, the native position grid: the resize is the identity
    "b1_96": ("tiny_dpt", 1, 96, 303),         # grid 6: pos-embed enlarged by 1.5, partial pixel tiles at every level
    "b1_128": ("tiny_dpt", 1, 128, 304),       # grid 8, 65 tokens: attention crosses a 64-key block boundary; 128 x 128 final map
    "wide_b1_64": ("tiny_dpt_wide", 1, 64, 305),   # neck widths 96 / 192 / 384: partial channel tiles, several k-chunks per tap
}


def transformers_present() -> bool:
    try:
        import transformers.models.dpt.modeling_dpt  # noqa: F401
        return True
    except Exception:
        return False


def case_input(name: str) -> torch.Tensor:
    _, B, S, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, 3, S, S), generator=g).to(torch.uint8)


def pixel_values(x: torch.Tensor) -> torch.Tensor:
    return (x.to(torch.float32) / 255 - 0.5) / 0.5


def hf_config(cfg):
    from transformers import DPTConfig
    return DPTConfig(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                     intermediate_size=cfg.intermediate_size, image_size=cfg.image_size, patch_size=cfg.patch_size,
                     backbone_out_indices=list(cfg.backbone_out_indices), neck_hidden_sizes=list(cfg.neck_hidden_sizes),
                     fusion_hidden_size=cfg.fusion_hidden_size, readout_type=cfg.readout_type, reassemble_factors=list(cfg.reassemble_factors),
                     layer_norm_eps=cfg.layer_norm_eps, hidden_act=cfg.hidden_act, qkv_bias=cfg.qkv_bias, is_hybrid=cfg.is_hybrid,
                     use_batch_norm_in_fusion_residual=cfg.use_batch_norm_in_fusion_residual, add_projection=cfg.add_projection,
                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def build_model(cfg_name: str):
    """DPTForDepthEstimation in fp32 around the synthetic weights (strict load: the name lists must agree)."""
    from transformers import DPTForDepthEstimation
    from controlar_amd import config as Cfg, synth
    cfg = getattr(Cfg, cfg_name)()
    model = DPTForDepthEstimation(hf_config(cfg)).float().eval()
    model.load_state_dict(synth.dpt_state_dict(cfg, WEIGHT_SEED), strict=True)
    return model


def _bf16_emulation(model):
    e = copy.deepcopy(model)
    for m in e.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d, torch.nn.Linear)):
            m.weight.data = m.weight.data.to(torch.bfloat16).float()
            m.register_forward_pre_hook(lambda mod, args: (args[0].to(torch.bfloat16).float(),) + tuple(args[1:]))
    return e


def mint(name: str, out_dir: str, model=None) -> str:
    torch.set_num_threads(1)
    if model is None:
        model = build_model(CASES[name][0])
    x = case_input(name)
    pv = pixel_values(x)
    with torch.no_grad():
        ref = model(pixel_values=pv).predicted_depth
        ref64 = copy.deepcopy(model).double()(pixel_values=pv.double()).predicted_depth
        nat = copy.deepcopy(model).bfloat16()(pixel_values=pv.bfloat16()).predicted_depth.float()
        emu = _bf16_emulation(model)(pixel_values=pv).predicted_depth
    assert ref.dtype == torch.float32 and ref64.dtype == torch.float64 and tuple(ref.shape) == (x.shape[0], x.shape[2], x.shape[3])
    d64 = (ref.double() - ref64).abs()
    dn, de = (ref - nat).abs(), (ref - emu).abs()
    zero_share = (ref == 0).float().mean().item()
    rec = dict(x=x.numpy(), ref=ref.numpy(), ref_f32_vs_f64_max=np.float64(d64.max().item()),
               bf16_native_max=np.float64(dn.max().item()), bf16_native_mean=np.float64(dn.mean().item()),
               bf16_emul_max=np.float64(de.max().item()), bf16_emul_mean=np.float64(de.mean().item()), zero_share=np.float64(zero_share))
    print(f"{name}: out {tuple(ref.shape)} max {ref.max().item():.3f} zero share {zero_share:.4f}  f32 vs f64 max {d64.max().item():.3g}  "
          f"bf16 native max {dn.max().item():.3g} mean {dn.mean().item():.3g}  emulation max {de.max().item():.3g} mean {de.mean().item():.3g}")
    check_case(name, rec)
    path = os.path.join(out_dir, f"depth_{name}.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < 150_000, (path, os.path.getsize(path))
    return path


def check_case(name, z):
    """The per-case conditions on a fixture (a dict or an open npz)."""
    ref = z["ref"]
    assert float(z["zero_share"]) <= 0.25, (name, "a map of zeros could pass", float(z["zero_share"]))
    assert float(ref.max()) >= 1.0, (name, "map maximum", float(ref.max()))
    assert float(z["bf16_emul_max"]) <= 1.5 * float(z["bf16_native_max"]), (name, float(z["bf16_emul_max"]), float(z["bf16_native_max"]))
    assert float(z["bf16_emul_mean"]) <= 1.5 * float(z["bf16_native_mean"]), (name, float(z["bf16_emul_mean"]), float(z["bf16_native_mean"]))


def check_all(files):
    """The condition over the whole set: the final ReLU is exercised somewhere."""
    assert max(float(z["zero_share"]) for z in files) >= 0.01, "no case clips at the final ReLU"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("cases", nargs="*", default=list(CASES))
    a = ap.parse_args()
    models = {}
    for c in a.cases:
        cn = CASES[c][0]
        if cn not in models:
            models[cn] = build_model(cn)
        mint(c, a.out, models[cn])
    check_all([np.load(os.path.join(a.out, f"depth_{c}.npz")) for c in CASES if os.path.exists(os.path.join(a.out, f"depth_{c}.npz"))])
