#!/usr/bin/env python
"""Mint the LineArt fixtures from the UNMODIFIED reference module ``condition.lineart`` (condition/lineart.py:26-86).

Runs only where the reference tree is present (CONTROLAR_REFERENCE, as tests/golden/make_golden.py).  That file imports ``controlnet_aux`` and
``cv2`` at module level and never uses them in ``LineArt``: when one of them cannot be imported, an empty stand-in module is registered for exactly
that name.  Weights are ``controlar_amd.synth.lineart_state_dict(seed)`` (17 MB: regenerated, never committed); inputs are seeded integer-valued
0..255 images, which is what the reference receives (sample_t2i.py:129-132) and which bf16 holds exactly.

Each ``lineart_<case>.npz`` holds
  x                    the input, fp32 [B,3,H,W]
  ref                  LineArt.forward in fp32, [B,1,Ho,Wo]
  ref_f32_vs_f64_max   max |ref - the same module in .double()|: the yardstick of the exact mode
  bf16_emul_max/mean   max / mean |ref - the same module with every conv's input and weight rounded to bf16 (forward pre-hook)|: the yardstick of the
                       fast mode

usage: python tests/golden/make_lineart_golden.py [--out DIR] [case ...]
"""
import argparse
import copy
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CONTROLAR_REFERENCE", "/root/reference")

WEIGHT_SEED = 11
CASES = {            # name -> (B, H, W, input seed)
    "b2_16x24": (2, 16, 24, 101),       # two different images: statistics must not mix
    "b1_30x44": (1, 30, 44, 102),       # output 32 x 44: stride-2 floor on odd sizes, every reflection edge
    "b1_8x8": (1, 8, 8, 103),           # 2 x 2 at the residual level: reflection hits both sides, InstanceNorm over 4 elements
    "b1_72x104": (1, 72, 104, 104),     # 468 pixels at the residual level, 7488 at full resolution: partial tiles in both
}


def reference_tree_present() -> bool:
    return os.path.isfile(os.path.join(REF, "condition", "lineart.py"))


def import_reference_lineart():
    """condition.lineart of the reference, unmodified; empty stand-ins for the two unused third-party imports that are absent."""
    for name in ("controlnet_aux", "cv2"):
        try:
            importlib.import_module(name)
        except ImportError:
            m = types.ModuleType(name)
            if name == "controlnet_aux":
                m.LineartDetector = None          # `from controlnet_aux import LineartDetector`: the name must exist, it is never used
            sys.modules[name] = m
    if REF not in sys.path:
        sys.path.insert(0, REF)
    return importlib.import_module("condition.lineart")


def case_input(name: str) -> torch.Tensor:
    B, H, W, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, 3, H, W), generator=g).float()


def build_model(mod):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from controlar_amd import synth
    net = mod.LineArt()
    net.load_state_dict(synth.lineart_state_dict(WEIGHT_SEED))
    return net.eval()


def _bf16_emulation(net):
    e = copy.deepcopy(net)
    for m in e.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
            m.weight.data = m.weight.data.to(torch.bfloat16).float()
            m.register_forward_pre_hook(lambda mod, args: (args[0].to(torch.bfloat16).float(),))
    return e


def mint(name: str, out_dir: str, net=None) -> str:
    torch.set_num_threads(1)
    if net is None:
        net = build_model(import_reference_lineart())
    x = case_input(name)
    with torch.no_grad():
        ref = net(x)
        ref64 = copy.deepcopy(net).double()(x.double())
        emu = _bf16_emulation(net)(x)
    d64 = (ref.double() - ref64).abs()
    de = (ref - emu).abs()
    path = os.path.join(out_dir, f"lineart_{name}.npz")
    np.savez_compressed(path, x=x.numpy(), ref=ref.numpy(), ref_f32_vs_f64_max=np.float64(d64.max().item()),
                        bf16_emul_max=np.float64(de.max().item()), bf16_emul_mean=np.float64(de.mean().item()))
    print(f"{name}: out {tuple(ref.shape)} range {ref.min().item():.4f}..{ref.max().item():.4f} std {ref.std().item():.3f}  "
          f"f32 vs f64 max {d64.max().item():.3g}  bf16 emulation max {de.max().item():.3g} mean {de.mean().item():.3g}")
    return path


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("cases", nargs="*", default=list(CASES))
    a = ap.parse_args()
    model = build_model(import_reference_lineart())
    for c in a.cases:
        mint(c, a.out, model)
