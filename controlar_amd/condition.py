"""Condition extractors of the path's front end.  ``CannyDetector`` keeps the call shape of the reference's
``condition/canny.py:6-14`` (array or tensor (H, W, 3) in, array (H, W) out) and runs ``car_canny`` on the GPU.  ``LineArt`` keeps the call shape of
``condition/lineart.py:26-86`` (tensor (B, 3, H, W) in, tensor (B, 1, Ho, Wo) in 0..1 out) and runs ``car_lineart``.  ``HEDdetector`` keeps the call shape of
``condition/hed.py:56-81`` (tensor (B, 3, H, W) in, raw 0..255; tensor (B, H, W) in 0..255 out) and runs ``car_hed``.  ``Resizer`` is PIL's 8-bit
``Image.resize`` on the GPU (``car_resize``, bit-identical to Pillow); beside it stand the reference's own resize helpers with their call shapes:
``center_crop_arr`` (dataset/augmentation.py:8-26), ``resize_image_to_16_multiple`` (sample_t2i_MR.py:37-49), ``resize_image`` and ``HWC3``
(condition/utils.py:9-38)."""
from __future__ import annotations

import numpy as np
import torch

from .config import tiny_t2i
from .engine import Engine


# Pillow's filter codes (Image.Resampling), which are car_resize's
LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 1, 2, 3, 4, 5


def _is_pil(img) -> bool:
    return hasattr(img, "resize") and hasattr(img, "mode") and hasattr(img, "size") and not torch.is_tensor(img) and not isinstance(img, np.ndarray)


def _to_u8(img):
    """PIL image (mode L or RGB), uint8 array or uint8 tensor -> (uint8 tensor, kind) with kind in 'pil' | 'np' | 'torch'."""
    if _is_pil(img):
        if img.mode not in ("L", "RGB", "RGBA"):
            raise ValueError(f"the GPU resizer takes 8-bit images of mode L or RGB, got mode {img.mode!r}: convert() it first")
        return torch.from_numpy(np.array(img)), "pil"                 # RGBA reaches car_resize, whose refusal points at HWC3
    if torch.is_tensor(img):
        if img.dtype != torch.uint8:
            raise TypeError(f"the GPU resizer takes 8-bit images (torch.uint8), got {img.dtype}")
        return img, "torch"
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise TypeError(f"the GPU resizer takes 8-bit images (uint8), got {a.dtype}")
    return torch.from_numpy(np.ascontiguousarray(a)), "np"


def _back(t: torch.Tensor, kind: str, like=None):
    """The result in the kind the caller gave: a PIL image, an array, or a tensor on the device of the input."""
    if kind == "torch":
        return t.to(like.device)
    a = t.cpu().numpy()
    if kind == "np":
        return a
    from PIL import Image
    return Image.fromarray(a)


class Resizer:
    """``Image.resize(size, resample, box)`` of 8-bit images on the GPU, bit for bit (``car_resize``).  It owns a context as ``CannyDetector`` does.
    A PIL image (mode L or RGB) returns a PIL image; an array or tensor (H,W), (H,W,C) or (B,H,W,C) with C in {1, 3} comes back in kind."""

    def __init__(self, device=None):
        self._eng = Engine(tiny_t2i(), "bf16", device=device)        # the kernel needs no weights: any context serves

    def __call__(self, img, size, resample=BICUBIC, box=None):
        x, kind = _to_u8(img)
        return _back(self._eng.resize(x, size, resample, box), kind, x)

    def on_device(self, x: torch.Tensor, size, resample=BICUBIC, box=None, **kw):
        """The same on a uint8 tensor, result left on the GPU (``want_control`` / ``want_float`` as ``Engine.resize`` takes them)."""
        return self._eng.resize(x, size, resample, box, **kw)


_shared = {}


def shared_resizer(device=None) -> Resizer:
    """One Resizer per device for the helpers below (created on first use)."""
    key = str(torch.device(device)) if device is not None else "default"
    if key not in _shared:
        _shared[key] = Resizer(device)
    return _shared[key]


def HWC3(x):
    """condition/utils.py:9-25 in plain torch: (H,W) / (H,W,1) -> three equal channels, (H,W,3) as it is, (H,W,4) blended over white.
    Array in, array out; tensor in, tensor out."""
    t = torch.from_numpy(x) if isinstance(x, np.ndarray) else x
    assert t.dtype == torch.uint8
    if t.dim() == 2:
        t = t[:, :, None]
    assert t.dim() == 3
    C = t.shape[2]
    assert C == 1 or C == 3 or C == 4
    if C == 1:
        t = torch.cat([t, t, t], dim=2)
    elif C == 4:
        color = t[:, :, 0:3].to(torch.float32)
        alpha = t[:, :, 3:4].to(torch.float32) / 255.0
        t = (color * alpha + 255.0 * (1.0 - alpha)).clip(0, 255).to(torch.uint8)
    return t.numpy() if isinstance(x, np.ndarray) else t


def center_crop_arr(pil_image, image_size, resizer=None):
    """dataset/augmentation.py:8-26 (ADM's centre crop): BOX halvings while the shorter side is at least 2*image_size, BICUBIC to
    round(side * image_size / shorter side), then the central image_size x image_size window.  Every resize runs on the GPU."""
    r = resizer or shared_resizer()
    x, kind = _to_u8(pil_image)
    t = x
    H, W = t.shape[0], t.shape[1]
    while min(W, H) >= 2 * image_size:
        W, H = W // 2, H // 2
        t = r.on_device(t, (W, H), BOX)
    scale = image_size / min(W, H)
    W, H = round(W * scale), round(H * scale)
    t = r.on_device(t, (W, H), BICUBIC)
    crop_y, crop_x = (H - image_size) // 2, (W - image_size) // 2
    return _back(t[crop_y: crop_y + image_size, crop_x: crop_x + image_size].contiguous(), kind, x)


def resize_image_to_16_multiple(image_path, condition_type="seg", resizer=None):
    """sample_t2i_MR.py:37-49: both sides up to the next multiple of 16 (32 for 'depth'), Image.resize's default filter (BICUBIC).  Takes the path
    the reference takes (opened with PIL, a PIL image comes back) or an image that is already loaded (PIL image, array or tensor, back in kind)."""
    import os
    if isinstance(image_path, (str, bytes, os.PathLike)):
        from PIL import Image
        image_path = Image.open(image_path)
    x, kind = _to_u8(image_path)
    height, width = x.shape[0], x.shape[1]
    m = 32 if condition_type == "depth" else 16
    new_width, new_height = (width + m - 1) // m * m, (height + m - 1) // m * m
    return _back((resizer or shared_resizer()).on_device(x, (new_width, new_height), BICUBIC), kind, x)


def resize_image(input_image, resolution, resizer=None):
    """condition/utils.py:28-38: the shorter side to `resolution`, both sides rounded to multiples of 64.  The reference resizes with cv2
    (INTER_LANCZOS4 when enlarging, INTER_AREA when shrinking); cv2 is not available, so PIL's counterparts LANCZOS / BOX stand in: not bit-equal
    to cv2.resize, bit-equal to PIL."""
    x, kind = _to_u8(input_image)
    H, W = float(x.shape[0]), float(x.shape[1])
    k = float(resolution) / min(H, W)
    H, W = int(np.round(H * k / 64.0)) * 64, int(np.round(W * k / 64.0)) * 64
    return _back((resizer or shared_resizer()).on_device(x, (W, H), LANCZOS if k > 1 else BOX), kind, x)


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
    rescale and normalise ((x/255 - 0.5)/0.5) and, given ``size``, also its PIL bicubic resize in front, on the GPU.  The model itself takes square
    images whose side is a multiple of 32.  The weights live in a context of their own."""

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
    def preprocess(images, size=None):
        """uint8 [B,3,S,S] -> fp32 pixel_values: rescale by 1/255, normalise with mean = std = 0.5 (DPTImageProcessor's defaults for dpt-large).
        With ``size`` = (height, width) the uint8 batch [B,3,H,W] (or one PIL image / (H,W,3) array, as ``processor(images=...)`` gets it) is first
        resized to exactly that size on the GPU with PIL's BICUBIC, which is what the processor does at sample_t2i.py:135 (size=(512,512),
        keep_aspect_ratio off); pixel_values then come from the same launch and stay on the GPU."""
        if size is None:
            return (images.to(torch.float32) / 255 - 0.5) / 0.5
        if torch.is_tensor(images) and images.dim() == 4:
            x = images.permute(0, 2, 3, 1)
        else:
            x = _to_u8(images)[0]
            x = HWC3(x)[None]
        r = shared_resizer(x.device if x.is_cuda else None)
        return r.on_device(x, (int(size[1]), int(size[0])), BICUBIC, want_float="norm")[1]

    def to(self, device=None, *args, **kwargs):
        return self

    def eval(self):
        return self

    def __call__(self, pixel_values=None, **kwargs):
        return _DepthOutput(self._eng.depth(pixel_values).to(pixel_values.device))
