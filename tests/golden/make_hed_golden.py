#!/usr/bin/env python
"""Mint the HED fixtures from the UNMODIFIED reference classes of ``condition.hed`` (condition/hed.py:17-81).

Runs only where the reference tree is present (CONTROLAR_REFERENCE, as tests/golden/make_golden.py).  That file imports ``cv2`` at module level and
uses it only in ``nms``: when it cannot be imported, an empty stand-in module is registered for that name.  ``HEDdetector.__init__`` fetches its
checkpoint when the file is missing, so the constructor is never called: ``ControlNetHED_Apache2()`` takes the synthetic weights
(``controlar_amd.synth.hed_state_dict(seed)``, 59 MB: regenerated, never committed), a detector is made with ``HEDdetector.__new__`` +
``torch.nn.Module.__init__`` and gets the network as ``netNetwork``; the unmodified ``HEDdetector.__call__`` then runs on it.  Inputs are seeded
integer-valued 0..255 images stored as uint8, which is what the scripts pass (sample_t2i.py:126-128).

Each ``hed_<case>.npz`` holds
  x                    the input, uint8 [B,3,H,W]
  ref                  HEDdetector.__call__ in fp32, [B,H,W], 0..255
  ref_f32_vs_f64_max   max |ref - the same module in .double()|: the yardstick of the exact mode
  bf16_emul_max/mean   max / mean |ref - the same module with every conv2d's input and weight rounded to bf16 (forward pre-hook)|: the yardstick of
                       the fast mode

usage: python tests/golden/make_hed_golden.py [--out DIR] [case ...]
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
    "b2_16x24": (2, 16, 24, 201),       # the smallest legal size (block 5 is 1 x 1); two different images must not mix
    "b1_17x31": (1, 17, 31, 202),       # odd sizes: the first pool drops the last row and column
    "b1_35x50": (1, 35, 50, 203),       # 35 -> 17 -> 8 -> 4 -> 2, 50 -> 25 -> 12 -> 6 -> 3: up-sampling scales that are no powers of two
    "b1_72x104": (1, 72, 104, 204),     # partial pixel tiles at every level; 512-channel layers with several k-chunks per tap
}


def reference_tree_present() -> bool:
    return os.path.isfile(os.path.join(REF, "condition", "hed.py"))


def import_reference_hed():
    """condition.hed of the reference, unmodified; an empty stand-in for cv2 (used by `nms` only) when it is absent."""
    try:
        importlib.import_module("cv2")
    except ImportError:
        sys.modules["cv2"] = types.ModuleType("cv2")
    if REF not in sys.path:
        sys.path.insert(0, REF)
    return importlib.import_module("condition.hed")


def case_input(name: str) -> torch.Tensor:
    B, H, W, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, 3, H, W), generator=g).to(torch.uint8)


def build_model(mod):
    """A HEDdetector around synthetic weights, without its downloading constructor."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from controlar_amd import synth
    net = mod.ControlNetHED_Apache2().float()
    net.load_state_dict(synth.hed_state_dict(WEIGHT_SEED))
    det = mod.HEDdetector.__new__(mod.HEDdetector)
    torch.nn.Module.__init__(det)
    det.netNetwork = net
    return det.eval()


def _bf16_emulation(det):
    e = copy.deepcopy(det)
    for m in e.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.weight.data = m.weight.data.to(torch.bfloat16).float()
            m.register_forward_pre_hook(lambda mod, args: (args[0].to(torch.bfloat16).float(),))
    return e


def mint(name: str, out_dir: str, det=None) -> str:
    torch.set_num_threads(1)
    if det is None:
        det = build_model(import_reference_hed())
    x = case_input(name)
    with torch.no_grad():
        ref = det(x)                                    # uint8 in: promoted by `x - self.norm`, as in the scripts
        ref64 = copy.deepcopy(det).double()(x)
        emu = _bf16_emulation(det)(x)
    assert ref.dtype == torch.float32 and ref64.dtype == torch.float64
    d64 = (ref.double() - ref64).abs()
    de = (ref - emu).abs()
    path = os.path.join(out_dir, f"hed_{name}.npz")
    np.savez_compressed(path, x=x.numpy(), ref=ref.numpy(), ref_f32_vs_f64_max=np.float64(d64.max().item()),
                        bf16_emul_max=np.float64(de.max().item()), bf16_emul_mean=np.float64(de.mean().item()))
    inside = ((ref >= 5) & (ref <= 250)).float().mean().item()
    print(f"{name}: out {tuple(ref.shape)} range {ref.min().item():.2f}..{ref.max().item():.2f} inside 5..250 {inside:.3f}  "
          f"f32 vs f64 max {d64.max().item():.3g}  bf16 emulation max {de.max().item():.3g} mean {de.mean().item():.3g}")
    return path


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("cases", nargs="*", default=list(CASES))
    a = ap.parse_args()
    model = build_model(import_reference_hed())
    for c in a.cases:
        mint(c, a.out, model)
