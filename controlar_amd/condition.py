"""Condition extractors of the path's front end.  ``CannyDetector`` keeps the call shape of the reference's
``condition/canny.py:6-14`` (array or tensor (H, W, 3) in, array (H, W) out) and runs ``car_canny`` on the GPU.  ``LineArt`` keeps the call shape of
``condition/lineart.py:26-86`` (tensor (B, 3, H, W) in, tensor (B, 1, Ho, Wo) in 0..1 out) and runs ``car_lineart``.  ``HEDdetector`` keeps the call shape of
``condition/hed.py:56-81`` (tensor (B, 3, H, W) in, raw 0..255; tensor (B, H, W) in 0..255 out) and runs ``car_hed``."""
from __future__ import annotations

import numpy as np
import torch

from .config import tiny_t2i
from .engine import Engine


class CannyDetector:
    def __init__(self, device=None):
        self._eng = Engine(tiny_t2i(), "bf16", device=device)        # the kernel needs no weights: any context serves

    def __call__(self, img, low_threshold=100, high_threshold=200):
        """input: array or tensor (H,W,3)   output: array (H,W)   (condition/canny.py:7-14)"""
        if torch.is_tensor(img):
            img = img.cpu().detach().numpy().astype(np.uint8)
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(img, dtype=np.uint8)))
        return self._eng.canny(x, low_threshold, high_threshold).cpu().numpy()


class LineArt:
    """Drop-in for the reference's ``LineArt()`` module (default constructor: 3 residual blocks, sigmoid) as the sampling scripts use it
    (sample_t2i.py:110-113: construct, load_state_dict, .to(device); :129-132: call).  The weights live in a context of their own."""

    def __init__(self, input_nc=3, output_nc=1, n_residual_blocks=3, sigmoid=True, precision="bf16", device=None):
        if (input_nc, output_nc, n_residual_blocks, sigmoid) != (3, 1, 3, True):
            raise NotImplementedError("car_lineart implements the reference's default LineArt(3, 1, 3, sigmoid=True)")
        self.precision = precision
        self._eng = Engine(tiny_t2i(), precision, device=device)     # the config only shapes the GPT / VQ side, which this context does not hold

    def load_state_dict(self, sd, strict=True):
        self._eng.load_lineart(sd, finalize=True)
        return self

    def to(self, device=None, *args, **kwargs):
        return self

    def eval(self):
        return self

    def forward(self, x, cond=None):
        """input: tensor (B,C,H,W)   output: tensor (B,1,H,W) 0~1   (condition/lineart.py:74-86)"""
        return self._eng.lineart(x).to(x.device)

    def __call__(self, x, cond=None):
        return self.forward(x, cond)


class HEDdetector:
    """Drop-in for the reference's ``HEDdetector()`` as the sampling scripts use it (sample_t2i.py:108-109: construct, .to(device), .eval();
    :126-128: call on a uint8 (B,3,H,W) tensor).  The reference's constructor fetches ``ControlNetHED.pth``; this one never downloads: pass the
    local file as ``model_path``, or hand the weights to ``load_state_dict``.  The weights live in a context of their own."""

    def __init__(self, model_path=None, precision="bf16", device=None):
        self.precision = precision
        self._eng = Engine(tiny_t2i(), precision, device=device)     # the config only shapes the GPT / VQ side, which this context does not hold
        if model_path is not None:
            self.load_state_dict(torch.load(model_path, map_location="cpu"))

    def load_state_dict(self, sd, strict=True):
        """ControlNetHED_Apache2().state_dict() keys, with or without the detector's ``netNetwork.`` prefix."""
        self._eng.load_hed(sd, finalize=True)
        return self

    def to(self, device=None, *args, **kwargs):
        return self

    def eval(self):
        return self

    def __call__(self, input_image):
        """input: tensor (B,C,H,W)   output: tensor (B,H,W)   (condition/hed.py:67-81)"""
        return self._eng.hed(input_image).to(input_image.device)


class _DepthOutput:
    def __init__(self, predicted_depth):
        self.predicted_depth = predicted_depth


class DepthEstimator:
    """Stands where the sampling scripts hold ``DPTForDepthEstimation.from_pretrained("dpt_large")`` and its image processor (sample_t2i.py:33,114-116,
    133-139): ``from_pretrained(local_dir)``, ``.to(device)``, ``.eval()``, ``model(pixel_values=...).predicted_depth``.  ``from_pretrained`` reads
    ``config.json`` and ``model.safetensors`` (or ``pytorch_model.bin``) from a LOCAL directory and never downloads.  ``preprocess`` is the processor's
    rescale and normalise ((x/255 - 0.5)/0.5); the processor's PIL resize to the model's square input size stays with the caller: this class takes
    square images whose side is a multiple of 32.  The weights live in a context of their own."""

    def __init__(self, cfg, state_dict=None, precision="bf16", device=None):
        self.config = cfg
        self.precision = precision
        self._eng = Engine(tiny_t2i(), precision, device=device)     # the config only shapes the GPT / VQ side, which this context does not hold
        if state_dict is not None:
            self._eng.load_depth(state_dict, cfg, finalize=True)

    @classmethod
    def from_pretrained(cls, local_dir, precision="bf16", device=None):
        import json
        import os
        from .checkpoint import load_checkpoint, _torch_load
        from .config import DPTConfig
        with open(os.path.join(local_dir, "config.json")) as f:
            cfg = DPTConfig.from_hf_dict(json.load(f))
        st = os.path.join(local_dir, "model.safetensors")
        if os.path.exists(st):
            sd = load_checkpoint(st)
        else:
            sd = _torch_load(os.path.join(local_dir, "pytorch_model.bin"))
            for k in ("state_dict", "model"):
                if k in sd and isinstance(sd[k], dict):
                    sd = sd[k]
        return cls(cfg, sd, precision=precision, device=device)

    @staticmethod
    def preprocess(images):
        """uint8 [B,3,S,S] -> fp32 pixel_values: rescale by 1/255, normalise with mean = std = 0.5 (DPTImageProcessor's defaults for dpt-large)."""
        return (images.to(torch.float32) / 255 - 0.5) / 0.5

    def to(self, device=None, *args, **kwargs):
        return self

    def eval(self):
        return self

    def __call__(self, pixel_values=None, **kwargs):
        return _DepthOutput(self._eng.depth(pixel_values).to(pixel_values.device))
