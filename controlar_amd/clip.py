"""The CLIP score of the text-to-image evaluation (evaluations/t2i/evaluation.py:129-176, compute_clip_score) on the device, without saved PNGs and
without OpenAI's ``clip`` package: both towers, CLIP's preprocessor and the cosine run in libcontrolar_hip.so (car_clip_encode_image /
car_clip_encode_text / car_clip_score).

What stays outside the boundary: the BPE tokenizer (host-side string work, as sentencepiece for T5).  The device path takes the int64 ids it
produces, ``[B, 77]``; ``photo_depicts_ids`` is what the script does to them afterwards."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from .config import CLIPConfig, clip_vit_b32, tiny_t2i
from .engine import Engine

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def requant_table() -> torch.Tensor:
    """What an 8-bit value becomes on its way through the evaluation script: EvalDataset turns the PNG into a float tensor (ToTensor, Normalize(0.5, 0.5))
    and tensor2pil turns that back into bytes with a clamp and a TRUNCATING cast, all in fp32.  uint8 [256]; not the identity."""
    u = torch.arange(256, dtype=torch.float32)
    x = (u / 255.0 - 0.5) / 0.5
    return ((x + 1.0) * 127.5).clamp(0.0, 255.0).to(torch.uint8)


def photo_depicts_ids(ids: torch.Tensor, prepend_ids: Sequence[int], eot_id: int) -> torch.Tensor:
    """The caption ids as the script feeds them to the text tower (evaluation.py:151-163, the prefix of arXiv 2104.08718): the ids of "A photo depicts "
    go in behind the start token, the row is cut back to its original width, and a row whose last column is now occupied ends in the end-of-text id.
    ids integer [B, T] from the caller's tokenizer; ``prepend_ids`` (three ids there) and ``eot_id`` come from that tokenizer too."""
    if ids.dim() != 2 or ids.dtype.is_floating_point:
        raise ValueError(f"photo_depicts_ids: expected integer ids [B,T], got {ids.dtype} {tuple(ids.shape)}")
    B, T = ids.shape
    pre = torch.as_tensor(list(prepend_ids), dtype=ids.dtype, device=ids.device)[None].expand(B, -1)
    out = torch.cat([ids[:, :1], pre, ids[:, 1:]], dim=1)[:, :T].clone()
    last = out[:, T - 1]
    out[:, T - 1] = torch.where(last > 0, torch.full_like(last, int(eot_id)), last)
    return out


def clip_resized_size(H: int, W: int, n_px: int):
    """torchvision's Resize(n_px) on an H x W image: the short side becomes n_px, the long side int(n_px * long / short).  -> (Hr, Wr)"""
    return (n_px, int(n_px * W / H)) if H <= W else (int(n_px * H / W), n_px)


def center_crop_offset(side: int, crop: int) -> int:
    """torchvision's CenterCrop offset along one axis: int(round((side - crop) / 2.0)), Python's round (half to even)."""
    return int(round((side - crop) / 2.0))


def preprocess_reference(img_hwc_u8, n_px: int) -> torch.Tensor:
    """CLIP's preprocessor restated with PIL and torch on the CPU (the check of the device path, not part of it): BICUBIC resize of the short side, centre
    crop, u / 255, (x - mean) / std.  img uint8 [H,W,3] -> fp32 [3,n_px,n_px]."""
    import numpy as np
    from PIL import Image
    a = img_hwc_u8.cpu().numpy() if torch.is_tensor(img_hwc_u8) else np.asarray(img_hwc_u8)
    H, W, _ = a.shape
    Hr, Wr = clip_resized_size(H, W, n_px)
    im = Image.fromarray(a, "RGB").resize((Wr, Hr), Image.BICUBIC)
    top, left = center_crop_offset(Hr, n_px), center_crop_offset(Wr, n_px)
    crop = np.asarray(im)[top:top + n_px, left:left + n_px]
    x = torch.from_numpy(np.array(crop)).permute(2, 0, 1).to(torch.float32).div(255)
    mean = torch.tensor(CLIP_MEAN, dtype=torch.float32)[:, None, None]
    std = torch.tensor(CLIP_STD, dtype=torch.float32)[:, None, None]
    return (x - mean) / std


def from_openai_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """OpenAI's ``clip.load(...).state_dict()`` names -> HF CLIPModel names (released checkpoints come in either form).  The fused attention
    in_proj splits into q / k / v, ``visual.proj`` and ``text_projection`` ([width, proj] there) are transposed, the class embedding and the positional
    tables are renamed; ``input_resolution``, ``context_length`` and ``vocab_size`` carry no weights and are dropped."""
    out: Dict[str, torch.Tensor] = {}

    def block(src: str, dst: str):
        names = {"ln_1": "layer_norm1", "ln_2": "layer_norm2", "mlp.c_fc": "mlp.fc1", "mlp.c_proj": "mlp.fc2", "attn.out_proj": "self_attn.out_proj"}
        for k, v in sd.items():
            if not k.startswith(src):
                continue
            rest = k[len(src):]                          # "N.attn.in_proj_weight"
            n, tail = rest.split(".", 1)
            p = f"{dst}encoder.layers.{n}."
            if tail in ("attn.in_proj_weight", "attn.in_proj_bias"):
                kind = "weight" if tail.endswith("weight") else "bias"
                q, kk, vv = v.chunk(3, dim=0)
                out[p + f"self_attn.q_proj.{kind}"], out[p + f"self_attn.k_proj.{kind}"], out[p + f"self_attn.v_proj.{kind}"] = q, kk, vv
                continue
            for a, b in names.items():
                if tail.startswith(a + "."):
                    out[p + b + tail[len(a):]] = v
                    break
            else:
                raise KeyError(f"from_openai_state_dict: unexpected tensor {k}")

    block("visual.transformer.resblocks.", "vision_model.")
    block("transformer.resblocks.", "text_model.")
    simple = {"visual.conv1.weight": "vision_model.embeddings.patch_embedding.weight",
              "visual.class_embedding": "vision_model.embeddings.class_embedding",
              "visual.positional_embedding": "vision_model.embeddings.position_embedding.weight",
              "visual.ln_pre.weight": "vision_model.pre_layrnorm.weight", "visual.ln_pre.bias": "vision_model.pre_layrnorm.bias",
              "visual.ln_post.weight": "vision_model.post_layernorm.weight", "visual.ln_post.bias": "vision_model.post_layernorm.bias",
              "token_embedding.weight": "text_model.embeddings.token_embedding.weight",
              "positional_embedding": "text_model.embeddings.position_embedding.weight",
              "ln_final.weight": "text_model.final_layer_norm.weight", "ln_final.bias": "text_model.final_layer_norm.bias",
              "logit_scale": "logit_scale"}
    for k, v in sd.items():
        if k in simple:
            out[simple[k]] = v
        elif k == "visual.proj":
            out["visual_projection.weight"] = v.t().contiguous()
        elif k == "text_projection":
            out["text_projection.weight"] = v.t().contiguous()
        elif k in ("input_resolution", "context_length", "vocab_size") or ".resblocks." in k:
            continue
        else:
            raise KeyError(f"from_openai_state_dict: unexpected tensor {k}")
    return out


def is_openai_state_dict(sd: Dict[str, torch.Tensor]) -> bool:
    return "visual.conv1.weight" in sd


class CLIPScorer:
    """CLIP with both towers in libcontrolar_hip.so.  ``state_dict``: HF CLIPModel names or OpenAI's (recognised and mapped)."""

    def __init__(self, config: Optional[CLIPConfig] = None, state_dict: Optional[Dict[str, torch.Tensor]] = None, precision: str = "bf16",
                 device=None, engine: Optional[Engine] = None):
        if state_dict is None:
            raise ValueError("CLIPScorer needs a state_dict (nothing is downloaded)")
        self.config = config or clip_vit_b32()
        # the model lives in its own context unless one is shared (car_clip_configure works on any context)
        self.engine = engine or Engine(tiny_t2i(), precision=precision, device=device)
        self.device = self.engine.device
        if is_openai_state_dict(state_dict):
            state_dict = from_openai_state_dict(state_dict)
        self.engine.clip_configure(self.config)
        self.engine.load_clip_state_dict(state_dict, finalize=True)

    @torch.no_grad()
    def encode_image(self, img_u8: torch.Tensor, requant: bool = False) -> torch.Tensor:
        """uint8 [B,H,W,3] -> fp32 [B,proj_dim]: CLIP's preprocessor and image tower (``requant``: the script's float round trip first)."""
        return self.engine.clip_encode_image(img_u8, requant=requant)

    @torch.no_grad()
    def encode_text(self, ids: torch.Tensor) -> torch.Tensor:
        """integer ids [B,T] -> fp32 [B,proj_dim]"""
        return self.engine.clip_encode_text(ids)

    @torch.no_grad()
    def eval_image(self, pixels: torch.Tensor, eval_res: int = 256) -> torch.Tensor:
        """The image as compute_clip_score's loader hands it over, still 8-bit: ``pixels`` [B,3,H,W] in [-1,1] quantised as save_image writes the PNG,
        the long edge cropped at the centre (CenterCropLongEdge), LANCZOS to ``eval_res``.  uint8 [B,eval_res,eval_res,3]."""
        e = self.engine
        u8 = e.pixels_to_u8(pixels)
        _, H, W, _ = u8.shape
        s = min(H, W)
        top, left = center_crop_offset(H, s), center_crop_offset(W, s)
        return e.resize(u8, (eval_res, eval_res), "lanczos", box=(left, top, left + s, top + s))

    @torch.no_grad()
    def score(self, pixels: torch.Tensor, ids: torch.Tensor, eval_res: int = 256) -> torch.Tensor:
        """The script's whole path for one batch: ``pixels`` [B,3,H,W] in [-1,1] straight from vq_decode, ``ids`` [B,T] as photo_depicts_ids leaves
        them.  fp32 [B] cosines on the device; nothing is copied to the host."""
        img = self.encode_image(self.eval_image(pixels, eval_res), requant=True)
        return self.engine.clip_score(img, self.encode_text(ids))
