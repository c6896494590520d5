#!/usr/bin/env python
"""Mint the LPIPS / PSNR fixtures on the CPU from the restatement in tests/recon_ref.py (the reference's own ``LPIPS`` class cannot be constructed:
it needs torchvision and fetches a checkpoint; tests/test_lpips_cpu.py holds the restated trunk to the unmodified ``ControlNetHED_Apache2``).

Inputs and weights are regenerated from seeds (``case_inputs``, ``controlar_amd.synth.lpips_state_dict(WEIGHT_SEED)``) and never stored.  Every case
holds three pairs: two unrelated images, an image and a copy perturbed by 1e-3 noise, an identical pair.  ``lpips_<case>.npz`` holds
  val64, layers64      the restatement in fp64: [3], [3,5]
  val32, layers32      the same in fp32
  val_bf, layers_bf    the same with every conv's input and weight, and every tap, rounded to bf16 (fp32 otherwise)
  psnr64, psnr32       PSNR of quantised(b) / 255 against (a + 1) / 2 in fp64 and in fp32: [3]
``lpips_measured.json`` holds per case the restatement's own deviations, the yardsticks of the GPU tests: max |fp32 - fp64| and max |bf16 emulation - fp32|
over the fixture's values and over its per-layer terms, and max |psnr32 - psnr64| over the finite entries.

usage: python tests/golden/make_lpips_golden.py [--out DIR] [case ...]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

WEIGHT_SEED = 17
NOISE = 1e-3
CASES = {            # name -> (H, W, input seed)
    "16x24": (16, 24, 301),       # the smallest legal size (slice 5 is 1 x 1)
    "17x31": (17, 31, 302),       # odd sides: every pool drops a row and a column
    "35x50": (35, 50, 303),
    "72x104": (72, 104, 304),     # more than one 128-pixel tile per row block, channel tiles of all five widths
}


def case_inputs(name: str):
    """a, b fp32 [3,3,H,W] in [-1,1]: pair 0 unrelated, pair 1 a copy perturbed by 1e-3 noise, pair 2 identical."""
    H, W, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    # smooth-ish images: a coarse random field up-sampled, plus fine noise, clamped to [-1, 1]
    def image():
        coarse = torch.rand(1, 3, (H + 7) // 8 + 1, (W + 7) // 8 + 1, generator=g) * 2 - 1
        up = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
        return (up + 0.25 * torch.randn(1, 3, H, W, generator=g)).clamp(-1, 1)
    a = torch.cat([image(), image(), image()])
    b = torch.cat([image(), (a[1:2] + NOISE * torch.randn(1, 3, H, W, generator=g)).clamp(-1, 1), a[2:3].clone()])
    return a.contiguous(), b.contiguous()


def weights():
    from controlar_amd import synth
    return synth.lpips_state_dict(WEIGHT_SEED)


def mint(name: str, out_dir: str, sd=None):
    import recon_ref as R
    torch.set_num_threads(1)
    if sd is None:
        sd = weights()
    a, b = case_inputs(name)
    with torch.no_grad():
        v32, l32 = R.lpips(a, b, sd)
        v64, l64 = R.lpips(a.double(), b.double(), {k: v.double() for k, v in sd.items()})
        vbf, lbf = R.lpips(a, b, sd, bf16=True)
        rest, gt = R.restored_and_gt(R.recon_quantise_torch(b), a)
        p64, p32 = R.psnr(rest, gt, 1.0, torch.float64), R.psnr(rest, gt, 1.0, torch.float32)
    assert v32.dtype == torch.float32 and v64.dtype == torch.float64 and vbf.dtype == torch.float32
    path = os.path.join(out_dir, f"lpips_{name}.npz")
    np.savez_compressed(path, val64=v64.numpy(), layers64=l64.numpy(), val32=v32.numpy(), layers32=l32.numpy(), val_bf=vbf.numpy(), layers_bf=lbf.numpy(),
                        psnr64=p64.numpy(), psnr32=p32.numpy())
    fin = torch.isfinite(p64)
    dev = lambda x, y: float((x.double() - y.double()).abs().max())
    rec = dict(f32_vs_f64_val=dev(v32, v64), f32_vs_f64_layers=dev(l32, l64), bf16_vs_f32_val=dev(vbf, v32), bf16_vs_f32_layers=dev(lbf, l32),
               psnr_f32_vs_f64=dev(p32[fin], p64[fin]))
    print(f"{name}: lpips {[f'{x:.6g}' for x in v64.tolist()]} psnr {[f'{x:.4g}' for x in p64.tolist()]} {rec}")
    return path, rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("cases", nargs="*", default=list(CASES))
    args = ap.parse_args()
    sd = weights()
    mpath = os.path.join(args.out, "lpips_measured.json")
    measured = json.load(open(mpath)) if os.path.exists(mpath) else {}
    for c in args.cases:
        measured[c] = mint(c, args.out, sd)[1]
    json.dump(measured, open(mpath, "w"), indent=1, sort_keys=True)
