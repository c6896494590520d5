"""Deterministic synthetic weights and inputs (no checkpoints or datasets exist offline).

The recipe is SURVEY.md §8(d): reference-shaped state dicts keyed by the reference's own
parameter names (gpt_t2i.Transformer, HF Dinov2Model under ``adapter.model.``, VQModel),
drawn from a seeded torch CPU generator so the imported reference (golden script), the CPU
oracle and the HIP path all consume bit-identical fp32 tensors.

Why not the reference's own init: ``output.weight`` and every ``MLP`` are zero-initialised
(gpt_t2i.py:377,174-175) so logits and control tokens would be identically 0.
"""
from __future__ import annotations

import math
from typing import Dict

import torch

from .config import PathConfig, GPTConfig, ViTConfig, VQConfig, T5Config, DPTConfig, CLIPConfig


class _Rng:
    def __init__(self, seed: int):
        self.g = torch.Generator(device="cpu")
        self.g.manual_seed(seed)

    def normal(self, *shape, std=1.0, mean=0.0):
        return torch.randn(*shape, generator=self.g, dtype=torch.float32) * std + mean

    def uniform(self, *shape, lo=-1.0, hi=1.0):
        return torch.rand(*shape, generator=self.g, dtype=torch.float32) * (hi - lo) + lo


def gpt_state_dict(cfg: GPTConfig, vit: ViTConfig, seed: int = 0, ctrl_gain: float = 1.1) -> Dict[str, torch.Tensor]:
    """Names follow gpt_t2i.Transformer.state_dict() (reference gpt_t2i.py:310-349).
    SURVEY §8(d) recipe: embeddings N(0,1), transformer linears N(0,0.03^2), output.weight
    N(0,0.2^2); the text/control MLPs are fan-in scaled so control tokens are O(0.3) at every size."""
    r = _Rng(seed)
    D, H = cfg.dim, cfg.ffn_hidden
    lin = 0.03
    ctrl = ctrl_gain * D ** -0.5
    sd: Dict[str, torch.Tensor] = {}
    sd["tok_embeddings.weight"] = r.normal(cfg.vocab_size, D, std=1.0)
    if cfg.model_type == "c2i":      # LabelEmbedder (gpt.py:66-96): num_classes + 1 rows, last = CFG null class
        sd["cls_embedding.embedding_table.weight"] = r.normal(cfg.num_classes + 1, D, std=1.0)
    else:
        sd["cls_embedding.cap_proj.fc1.weight"] = r.normal(D, cfg.caption_dim, std=3.0 * cfg.caption_dim ** -0.5)
        sd["cls_embedding.cap_proj.fc2.weight"] = r.normal(D, D, std=3.0 * D ** -0.5)
        sd["cls_embedding.uncond_embedding"] = r.normal(cfg.cls_token_num, cfg.caption_dim, std=cfg.caption_dim ** -0.5)
    sd["adapter_mlp.fc1.weight"] = r.normal(D, vit.hidden, std=ctrl_gain * vit.hidden ** -0.5)
    sd["adapter_mlp.fc2.weight"] = r.normal(D, D, std=ctrl)
    sd["condition_mlp.cap_proj.fc1.weight"] = r.normal(D, D, std=ctrl)
    sd["condition_mlp.cap_proj.fc2.weight"] = r.normal(D, D, std=ctrl)
    for k in range(3):
        sd[f"condition_layers.{k}.fc1.weight"] = r.normal(D, D, std=ctrl)
        sd[f"condition_layers.{k}.fc2.weight"] = r.normal(D, D, std=ctrl)
    for i in range(cfg.n_layer):
        p = f"layers.{i}."
        sd[p + "attention.wqkv.weight"] = r.normal(3 * D, D, std=lin)
        sd[p + "attention.wo.weight"] = r.normal(D, D, std=lin)
        sd[p + "feed_forward.w1.weight"] = r.normal(H, D, std=lin)
        sd[p + "feed_forward.w3.weight"] = r.normal(H, D, std=lin)
        sd[p + "feed_forward.w2.weight"] = r.normal(D, H, std=lin)
        sd[p + "attention_norm.weight"] = r.normal(D, std=0.1, mean=1.0)
        sd[p + "ffn_norm.weight"] = r.normal(D, std=0.1, mean=1.0)
    sd["norm.weight"] = r.normal(D, std=0.1, mean=1.0)
    sd["output.weight"] = r.normal(cfg.vocab_size, D, std=0.2)
    return sd


def vit16_state_dict(cfg: ViTConfig, seed: int = 1, prefix: str = "adapter.model.") -> Dict[str, torch.Tensor]:
    """Names follow HF ViTModel.state_dict() (transformers 5.15.0 modeling_vit.py: layers.{i}.attention.{q,k,v,o}_proj ...)."""
    r = _Rng(seed)
    D, M = cfg.hidden, cfg.mlp
    n_pos = cfg.pos_grid * cfg.pos_grid + 1
    sd: Dict[str, torch.Tensor] = {}
    e = prefix + "embeddings."
    sd[e + "cls_token"] = r.normal(1, 1, D, std=0.02)
    sd[e + "position_embeddings"] = r.normal(1, n_pos, D, std=0.2)
    fan_in = 3 * cfg.patch * cfg.patch
    sd[e + "patch_embeddings.projection.weight"] = r.normal(D, 3, cfg.patch, cfg.patch, std=fan_in ** -0.5)
    sd[e + "patch_embeddings.projection.bias"] = r.normal(D, std=0.02)
    for i in range(cfg.layers):
        p = f"{prefix}layers.{i}."
        sd[p + "layernorm_before.weight"] = r.normal(D, std=0.1, mean=1.0)
        sd[p + "layernorm_before.bias"] = r.normal(D, std=0.05)
        for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
            sd[p + f"attention.{n}.weight"] = r.normal(D, D, std=(0.7 if n == "o_proj" else 1.0) * D ** -0.5)
            sd[p + f"attention.{n}.bias"] = r.normal(D, std=0.02)
        sd[p + "layernorm_after.weight"] = r.normal(D, std=0.1, mean=1.0)
        sd[p + "layernorm_after.bias"] = r.normal(D, std=0.05)
        sd[p + "mlp.fc1.weight"] = r.normal(M, D, std=D ** -0.5)
        sd[p + "mlp.fc1.bias"] = r.normal(M, std=0.02)
        sd[p + "mlp.fc2.weight"] = r.normal(D, M, std=0.7 * M ** -0.5)
        sd[p + "mlp.fc2.bias"] = r.normal(D, std=0.02)
    sd[prefix + "layernorm.weight"] = r.normal(D, std=0.1, mean=1.0)
    sd[prefix + "layernorm.bias"] = r.normal(D, std=0.05)
    sd[prefix + "pooler.dense.weight"] = r.normal(D, D, std=D ** -0.5)      # present in the checkpoint, unused on the path
    sd[prefix + "pooler.dense.bias"] = torch.zeros(D)
    return sd


def vit_state_dict(cfg: ViTConfig, seed: int = 1, prefix: str = "adapter.model.") -> Dict[str, torch.Tensor]:
    """Names follow HF Dinov2Model.state_dict() (transformers 5.15.0 modeling_dinov2.py)."""
    if cfg.variant == "vit":
        return vit16_state_dict(cfg, seed, prefix)
    r = _Rng(seed)
    D, M = cfg.hidden, cfg.mlp
    n_pos = cfg.pos_grid * cfg.pos_grid + 1
    sd: Dict[str, torch.Tensor] = {}
    e = prefix + "embeddings."
    sd[e + "cls_token"] = r.normal(1, 1, D, std=0.02)
    sd[e + "mask_token"] = torch.zeros(1, D)
    sd[e + "position_embeddings"] = r.normal(1, n_pos, D, std=0.2)
    fan_in = 3 * cfg.patch * cfg.patch
    sd[e + "patch_embeddings.projection.weight"] = r.normal(D, 3, cfg.patch, cfg.patch, std=fan_in ** -0.5)
    sd[e + "patch_embeddings.projection.bias"] = r.normal(D, std=0.02)
    for i in range(cfg.layers):
        p = f"{prefix}encoder.layer.{i}."
        sd[p + "norm1.weight"] = r.normal(D, std=0.1, mean=1.0)
        sd[p + "norm1.bias"] = r.normal(D, std=0.05)
        for n in ("query", "key", "value"):
            sd[p + f"attention.attention.{n}.weight"] = r.normal(D, D, std=D ** -0.5)
            sd[p + f"attention.attention.{n}.bias"] = r.normal(D, std=0.02)
        sd[p + "attention.output.dense.weight"] = r.normal(D, D, std=D ** -0.5)
        sd[p + "attention.output.dense.bias"] = r.normal(D, std=0.02)
        sd[p + "layer_scale1.lambda1"] = r.normal(D, std=0.05, mean=0.5)
        sd[p + "norm2.weight"] = r.normal(D, std=0.1, mean=1.0)
        sd[p + "norm2.bias"] = r.normal(D, std=0.05)
        sd[p + "mlp.fc1.weight"] = r.normal(M, D, std=D ** -0.5)
        sd[p + "mlp.fc1.bias"] = r.normal(M, std=0.02)
        sd[p + "mlp.fc2.weight"] = r.normal(D, M, std=M ** -0.5)
        sd[p + "mlp.fc2.bias"] = r.normal(D, std=0.02)
        sd[p + "layer_scale2.lambda1"] = r.normal(D, std=0.05, mean=0.5)
    sd[prefix + "layernorm.weight"] = r.normal(D, std=0.1, mean=1.0)
    sd[prefix + "layernorm.bias"] = r.normal(D, std=0.05)
    return sd


def _conv(r: _Rng, sd, name, cout, cin, k):
    bound = 1.0 / math.sqrt(cin * k * k)
    # gain ~sqrt(3): keeps activations O(1) through 30 conv layers with swish
    sd[name + ".weight"] = r.uniform(cout, cin, k, k, lo=-bound, hi=bound) * 1.7
    sd[name + ".bias"] = r.uniform(cout, lo=-bound, hi=bound)


def _gn(r: _Rng, sd, name, c):
    sd[name + ".weight"] = r.normal(c, std=0.1, mean=1.0)
    sd[name + ".bias"] = r.normal(c, std=0.1)


def vq_decoder_layout(cfg: VQConfig):
    """Yields the decode-side module list in execution order (reference vq_model.py:129-195).
    Items: ("res", name, cin, cout) | ("attn", name, c) | ("up", name, c)."""
    nres = len(cfg.ch_mult)
    block_in = cfg.ch * cfg.ch_mult[nres - 1]
    out = [("res", "decoder.mid.0", block_in, block_in), ("attn", "decoder.mid.1", block_in),
           ("res", "decoder.mid.2", block_in, block_in)]
    for idx, i_level in enumerate(reversed(range(nres))):
        block_out = cfg.ch * cfg.ch_mult[i_level]
        for j in range(cfg.num_res_blocks + 1):
            out.append(("res", f"decoder.conv_blocks.{idx}.res.{j}", block_in, block_out))
            block_in = block_out
            if i_level == nres - 1:
                out.append(("attn", f"decoder.conv_blocks.{idx}.attn.{j}", block_in))
        if i_level != 0:
            out.append(("up", f"decoder.conv_blocks.{idx}.upsample", block_in))
    return out, block_in


def vq_encoder_layout(cfg: VQConfig):
    """Encoder module list in execution order (reference vq_model.py:62-126).
    Items: ("res", name, cin, cout) | ("attn", name, c) | ("down", name, c)."""
    nres = len(cfg.ch_mult)
    in_mult = (1,) + tuple(cfg.ch_mult)
    out = []
    block_in = cfg.ch
    for i_level in range(nres):
        block_in = cfg.ch * in_mult[i_level]
        block_out = cfg.ch * cfg.ch_mult[i_level]
        for j in range(cfg.num_res_blocks):
            out.append(("res", f"encoder.conv_blocks.{i_level}.res.{j}", block_in, block_out))
            block_in = block_out
            if i_level == nres - 1:
                out.append(("attn", f"encoder.conv_blocks.{i_level}.attn.{j}", block_in))
        if i_level != nres - 1:
            out.append(("down", f"encoder.conv_blocks.{i_level}.downsample", block_in))
    out += [("res", "encoder.mid.0", block_in, block_in), ("attn", "encoder.mid.1", block_in), ("res", "encoder.mid.2", block_in, block_in)]
    return out, block_in


def vq_state_dict(cfg: VQConfig, seed: int = 2) -> Dict[str, torch.Tensor]:
    """Decode-side names of VQModel.state_dict() (reference vq_model.py:28-39,129-169)."""
    r = _Rng(seed)
    sd: Dict[str, torch.Tensor] = {}
    cb = r.uniform(cfg.codebook_size, cfg.codebook_embed_dim, lo=-1.0, hi=1.0)
    sd["quantize.embedding.weight"] = torch.nn.functional.normalize(cb, p=2, dim=-1) * r.uniform(cfg.codebook_size, 1, lo=0.5, hi=1.5)
    _conv(r, sd, "post_quant_conv", cfg.z_channels, cfg.codebook_embed_dim, 1)
    layout, last = vq_decoder_layout(cfg)
    block_in = cfg.ch * cfg.ch_mult[-1]
    _conv(r, sd, "decoder.conv_in", block_in, cfg.z_channels, 3)
    for item in layout:
        if item[0] == "res":
            _, name, cin, cout = item
            _gn(r, sd, name + ".norm1", cin)
            _conv(r, sd, name + ".conv1", cout, cin, 3)
            _gn(r, sd, name + ".norm2", cout)
            _conv(r, sd, name + ".conv2", cout, cout, 3)
            if cin != cout:
                _conv(r, sd, name + ".nin_shortcut", cout, cin, 1)
        elif item[0] == "attn":
            _, name, c = item
            _gn(r, sd, name + ".norm", c)
            for n in ("q", "k", "v", "proj_out"):
                _conv(r, sd, f"{name}.{n}", c, c, 1)
        else:
            _, name, c = item
            _conv(r, sd, name + ".conv", c, c, 3)
    _gn(r, sd, "decoder.norm_out", last)
    _conv(r, sd, "decoder.conv_out", 3, last, 3)
    # ---- encode side (vq_model.py:62-126 Encoder, :39 quant_conv).  Appended AFTER the decode side so the decoder tensors
    # (and every golden minted from them) keep their values.
    enc, elast = vq_encoder_layout(cfg)
    _conv(r, sd, "encoder.conv_in", cfg.ch, 3, 3)
    for item in enc:
        if item[0] == "res":
            _, name, cin, cout = item
            _gn(r, sd, name + ".norm1", cin)
            _conv(r, sd, name + ".conv1", cout, cin, 3)
            _gn(r, sd, name + ".norm2", cout)
            _conv(r, sd, name + ".conv2", cout, cout, 3)
            if cin != cout:
                _conv(r, sd, name + ".nin_shortcut", cout, cin, 1)
        elif item[0] == "attn":
            _, name, c = item
            _gn(r, sd, name + ".norm", c)
            for n in ("q", "k", "v", "proj_out"):
                _conv(r, sd, f"{name}.{n}", c, c, 1)
        else:
            _, name, c = item
            _conv(r, sd, name + ".conv", c, c, 3)
    _gn(r, sd, "encoder.norm_out", elast)
    _conv(r, sd, "encoder.conv_out", cfg.z_channels, elast, 3)
    _conv(r, sd, "quant_conv", cfg.codebook_embed_dim, cfg.z_channels, 1)
    return sd


def path_state_dicts(cfg: PathConfig, seed: int = 0):
    gpt = gpt_state_dict(cfg.gpt, cfg.vit, seed=seed)
    gpt.update(vit_state_dict(cfg.vit, seed=seed + 1))
    vq = vq_state_dict(cfg.vq, seed=seed + 2)
    return gpt, vq


# ----------------------------------------------------------------------------- inputs
def canny_like_control(batch: int, H: int, W: int, seed: int = 1234, density: float = 0.08, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Binary edge-like map in {-1,+1}, 3 identical channels, as sample_t2i.py:123-125,141
    produces from cv2.Canny (uint8 {0,255} -> 2*(x/255-0.5)).  One seeded generator per image (image i of any batch is the
    same map); written straight into the output in `dtype` (both values are exact in bf16)."""
    out = torch.empty(batch, 3, H, W, dtype=dtype)
    one, neg = torch.tensor(1.0, dtype=dtype), torch.tensor(-1.0, dtype=dtype)
    for i in range(batch):
        g = torch.Generator().manual_seed(seed + i)
        m = torch.rand(H, W, generator=g) > (1.0 - density)
        out[i] = torch.where(m, one, neg)            # broadcast over the 3 channels
    return out


def smooth_control(batch: int, H: int, W: int, seed: int = 1234) -> torch.Tensor:
    """Smooth map in [-1,1] (depth / soft-edge stand-in): low-pass filtered noise, 3 channels."""
    out = []
    for i in range(batch):
        g = torch.Generator().manual_seed(seed + i)
        lo = torch.rand(1, 1, max(H // 32, 2), max(W // 32, 2), generator=g)
        m = torch.nn.functional.interpolate(lo, size=(H, W), mode="bilinear", align_corners=True)[0, 0]
        out.append((2.0 * m - 1.0)[None].repeat(3, 1, 1))
    return torch.stack(out)


def class_labels(batch: int, num_classes: int, seed: int = 1234) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, num_classes, (batch,), generator=g, dtype=torch.int64)


def text_embeddings_with_lengths(lengths, T: int = 120, caption_dim: int = 2048, seed: int = 1234):
    """As text_embeddings but with explicit valid lengths (edge cases: 1 = a single real token, T = no padding at all)."""
    embs, masks = [], []
    for i, L in enumerate(lengths):
        g = torch.Generator().manual_seed(seed + i)
        e = 0.2 * torch.randn(T, caption_dim, generator=g)
        m = torch.zeros(T, dtype=torch.int64)
        m[T - int(L):] = 1
        embs.append(e * m[:, None])
        masks.append(m)
    return torch.stack(embs), torch.stack(masks)


def text_embeddings(batch: int, T: int = 120, caption_dim: int = 2048, seed: int = 1234):
    """0.2*randn caption features, valid length L~U{8..40}, LEFT-padded exactly as
    sample_t2i.py:146-160: valid tokens occupy the last L slots, features multiplied by mask."""
    embs, masks = [], []
    for i in range(batch):
        g = torch.Generator().manual_seed(seed + i)
        e = 0.2 * torch.randn(T, caption_dim, generator=g)
        L = int(torch.randint(8, min(41, T + 1), (1,), generator=g).item())
        m = torch.zeros(T, dtype=torch.int64)
        m[T - L:] = 1
        embs.append(e * m[:, None])
        masks.append(m)
    return torch.stack(embs), torch.stack(masks)


def t5_state_dict(cfg: T5Config, seed: int = 7) -> Dict[str, torch.Tensor]:
    """HF T5EncoderModel.state_dict() names (shared.weight, encoder.block.N.layer.{0,1}.*, encoder.final_layer_norm.weight).
    Scales follow T5PreTrainedModel._init_weights (q: (d_model*d_kv)^-0.5 because attention is unscaled; k, v, wi: d_model^-0.5;
    o: (heads*d_kv)^-0.5; wo: d_ff^-0.5) except that norms are 1 + 0.1 N and the relative bias is N(0, 0.5^2) so both matter."""
    r = _Rng(seed)
    D, kv, H, F = cfg.d_model, cfg.d_kv, cfg.num_heads, cfg.d_ff
    inner = H * kv
    sd = {"shared.weight": r.normal(cfg.vocab_size, D)}
    for i in range(cfg.num_layers):
        a = f"encoder.block.{i}.layer.0."
        sd[a + "SelfAttention.q.weight"] = r.normal(inner, D, std=(D * kv) ** -0.5 * 2.0)
        sd[a + "SelfAttention.k.weight"] = r.normal(inner, D, std=D ** -0.5)
        sd[a + "SelfAttention.v.weight"] = r.normal(inner, D, std=D ** -0.5)
        sd[a + "SelfAttention.o.weight"] = r.normal(D, inner, std=inner ** -0.5)
        if i == 0:
            sd[a + "SelfAttention.relative_attention_bias.weight"] = r.normal(cfg.relative_attention_num_buckets, H, std=0.5)
        sd[a + "layer_norm.weight"] = 1.0 + 0.1 * r.normal(D)
        f = f"encoder.block.{i}.layer.1."
        sd[f + "DenseReluDense.wi_0.weight"] = r.normal(F, D, std=D ** -0.5)
        sd[f + "DenseReluDense.wi_1.weight"] = r.normal(F, D, std=D ** -0.5)
        sd[f + "DenseReluDense.wo.weight"] = r.normal(D, F, std=F ** -0.5)
        sd[f + "layer_norm.weight"] = 1.0 + 0.1 * r.normal(D)
    sd["encoder.final_layer_norm.weight"] = 1.0 + 0.1 * r.normal(D)
    return sd


def t5_tokens(batch: int, cfg: T5Config, seed: int = 4321, lengths=None):
    """Tokenizer-shaped inputs: ids RIGHT-padded with 0 to model_max_length (HF T5 tokenizer pads right; the reference left-pads
    the EMBEDDINGS afterwards, sample_t2i.py:146-160), last valid id = 1 (</s>), attention_mask 1 on valid positions."""
    T = cfg.model_max_length
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(batch, T, dtype=torch.int64)
    mask = torch.zeros(batch, T, dtype=torch.int64)
    for b in range(batch):
        L = int(lengths[b]) if lengths is not None else int(torch.randint(4, min(41, T + 1), (1,), generator=g).item())
        ids[b, :L - 1] = torch.randint(2, cfg.vocab_size, (L - 1,), generator=g)
        ids[b, L - 1] = 1
        mask[b, :L] = 1
    return ids, mask


def clip_state_dict(cfg: CLIPConfig, seed: int = 17) -> Dict[str, torch.Tensor]:
    """HF CLIPModel.state_dict() names and shapes (text_model.*, vision_model.*, visual_projection.weight, text_projection.weight, logit_scale).
    Linears are fan-in scaled so activations stay O(1) through the layers; biases, the class token, positions and the norm offsets are large enough
    that dropping any of them shows."""
    r = _Rng(seed)
    sd: Dict[str, torch.Tensor] = {}

    def tower(p, D, F, layers):
        for i in range(layers):
            q = f"{p}encoder.layers.{i}."
            for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
                sd[q + f"self_attn.{n}.weight"] = r.normal(D, D, std=(1.5 if n in ("q_proj", "k_proj") else 1.0) * D ** -0.5)
                sd[q + f"self_attn.{n}.bias"] = r.normal(D, std=0.05)
            sd[q + "layer_norm1.weight"] = 1.0 + 0.1 * r.normal(D)
            sd[q + "layer_norm1.bias"] = r.normal(D, std=0.05)
            sd[q + "mlp.fc1.weight"] = r.normal(F, D, std=D ** -0.5)
            sd[q + "mlp.fc1.bias"] = r.normal(F, std=0.05)
            sd[q + "mlp.fc2.weight"] = r.normal(D, F, std=F ** -0.5)
            sd[q + "mlp.fc2.bias"] = r.normal(D, std=0.05)
            sd[q + "layer_norm2.weight"] = 1.0 + 0.1 * r.normal(D)
            sd[q + "layer_norm2.bias"] = r.normal(D, std=0.05)

    Dt, Dv, g = cfg.text_width, cfg.vision_width, cfg.grid
    sd["logit_scale"] = torch.tensor(math.log(1 / 0.07), dtype=torch.float32)
    sd["text_model.embeddings.token_embedding.weight"] = r.normal(cfg.vocab_size, Dt, std=0.5)
    sd["text_model.embeddings.position_embedding.weight"] = r.normal(cfg.context_length, Dt, std=0.3)
    tower("text_model.", Dt, cfg.text_mlp, cfg.text_layers)
    sd["text_model.final_layer_norm.weight"] = 1.0 + 0.1 * r.normal(Dt)
    sd["text_model.final_layer_norm.bias"] = r.normal(Dt, std=0.05)
    sd["vision_model.embeddings.class_embedding"] = r.normal(Dv, std=0.5)
    sd["vision_model.embeddings.patch_embedding.weight"] = r.normal(Dv, 3, cfg.patch, cfg.patch, std=(3 * cfg.patch * cfg.patch) ** -0.5)
    sd["vision_model.embeddings.position_embedding.weight"] = r.normal(g * g + 1, Dv, std=0.3)
    sd["vision_model.pre_layrnorm.weight"] = 1.0 + 0.1 * r.normal(Dv)
    sd["vision_model.pre_layrnorm.bias"] = r.normal(Dv, std=0.05)
    tower("vision_model.", Dv, cfg.vision_mlp, cfg.vision_layers)
    sd["vision_model.post_layernorm.weight"] = 1.0 + 0.1 * r.normal(Dv)
    sd["vision_model.post_layernorm.bias"] = r.normal(Dv, std=0.05)
    sd["visual_projection.weight"] = r.normal(cfg.proj_dim, Dv, std=Dv ** -0.5)
    sd["text_projection.weight"] = r.normal(cfg.proj_dim, Dt, std=Dt ** -0.5)
    return sd


def clip_tokens(batch: int, cfg: CLIPConfig, lengths=None, seed: int = 977) -> torch.Tensor:
    """Tokenizer-shaped ids int64 [batch, context_length] as OpenAI's ``clip.tokenize`` lays them out: the start token (eot - 1), caption ids below it,
    ONE end-of-text id (``cfg.eot_id``, the largest) at ``lengths[i] - 1``, zeros after it.  ``lengths[i]`` >= 2 (start + end)."""
    T, eot = cfg.context_length, cfg.eot_id
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(batch, T, dtype=torch.int64)
    for b in range(batch):
        L = int(lengths[b]) if lengths is not None else int(torch.randint(2, T + 1, (1,), generator=g).item())
        assert 2 <= L <= T, L
        ids[b, 0] = eot - 1
        if L > 2:
            ids[b, 1:L - 1] = torch.randint(1, eot - 1, (L - 2,), generator=g)
        ids[b, L - 1] = eot
    return ids


def clip_images(sizes, seed: int = 4242):
    """8-bit RGB test images [H, W, 3] (a list, one per (H, W) of ``sizes``): smooth gradients plus noise, so that resampling and rounding both matter."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for (H, W) in sizes:
        yy = torch.linspace(0, 1, H)[:, None, None]
        xx = torch.linspace(0, 1, W)[None, :, None]
        ph = torch.rand(3, generator=g)[None, None, :] * 6.28
        base = 0.5 + 0.35 * torch.sin(6.0 * yy + ph) * torch.cos(5.0 * xx - ph)
        img = (base + 0.15 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
        out.append((img * 255.0).round().to(torch.uint8))
    return out


def lineart_state_dict(seed: int = 11) -> Dict[str, torch.Tensor]:
    """LineArt().state_dict() names and shapes (reference condition/lineart.py:26-72, n_residual_blocks = 3): 24 tensors.  The stock initialisation gives
    an output of about 0.5 everywhere, which pins nothing; here every weight is N(0, 1/fan_in) (a transposed conv sees 9/4 taps per output on average),
    biases are N(0, 0.1^2), and the last conv is scaled x3 so that the sigmoid output spreads over (0, 1)."""
    r = _Rng(seed)
    sd: Dict[str, torch.Tensor] = {}

    def conv(name, co, ci, k, gain=1.0):
        sd[name + ".weight"] = r.normal(co, ci, k, k, std=gain * (ci * k * k) ** -0.5)
        sd[name + ".bias"] = r.normal(co, std=0.1)

    def convt(name, ci, co):
        sd[name + ".weight"] = r.normal(ci, co, 3, 3, std=(ci * 9 / 4) ** -0.5)
        sd[name + ".bias"] = r.normal(co, std=0.1)

    conv("model0.1", 64, 3, 7)
    conv("model1.0", 128, 64, 3)
    conv("model1.3", 256, 128, 3)
    for i in range(3):
        conv(f"model2.{i}.conv_block.1", 256, 256, 3)
        conv(f"model2.{i}.conv_block.5", 256, 256, 3)
    convt("model3.0", 256, 128)
    convt("model3.3", 128, 64)
    conv("model4.1", 1, 64, 7, gain=3.0)
    return sd


HED_BLOCKS = ((3, 64, 2), (64, 128, 2), (128, 256, 3), (256, 512, 3), (512, 512, 3))     # (Cin, Cout, convs) of block1..5 (condition/hed.py:40-44)


def hed_state_dict(seed: int = 11, proj_gain: float = 0.05) -> Dict[str, torch.Tensor]:
    """ControlNetHED_Apache2().state_dict() names and shapes (reference condition/hed.py:17-53): 37 tensors, 14.7 M parameters.  The stock initialisation
    has norm = 0 and tiny side outputs (a flat 127.5 everywhere); here conv weights are N(0, 2/fan_in) (He: the ReLU chain keeps its scale), biases
    N(0, 0.1^2), norm close to the channel means of natural images, and the 1x1 side projections N(0, proj_gain^2 / Cout), which spreads the fused
    sigmoid over most of 0..255 without saturating it."""
    r = _Rng(seed)
    sd: Dict[str, torch.Tensor] = {}
    sd["norm"] = torch.tensor([123.7, 116.3, 103.5]).view(1, 3, 1, 1) + r.normal(1, 3, 1, 1, std=0.5)
    for b, (ci, co, n) in enumerate(HED_BLOCKS, 1):
        for i in range(n):
            cin = ci if i == 0 else co
            sd[f"block{b}.convs.{i}.weight"] = r.normal(co, cin, 3, 3, std=(2.0 / (cin * 9)) ** 0.5)
            sd[f"block{b}.convs.{i}.bias"] = r.normal(co, std=0.1)
        sd[f"block{b}.projection.weight"] = r.normal(1, co, 1, 1, std=proj_gain * co ** -0.5)
        sd[f"block{b}.projection.bias"] = r.normal(1, std=0.1)
    return sd


LPIPS_FEATURES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))     # the convs of slice1..5 in torchvision's vgg16().features (lpips.py:128-137)


def lpips_state_dict(seed: int = 17, spelling: str = "lpips", scaling: bool = True) -> Dict[str, torch.Tensor]:
    """LPIPS().state_dict() names and shapes (reference tokenizer/tokenizer_image/lpips.py:53-65,99-141): 26 trunk tensors, five 1x1 ``lin`` weights and
    the two ScalingLayer buffers, 14.7 M parameters.  Trunk: conv weights N(0, 2/fan_in) (He: ``relu5_3`` is neither dead nor saturated after thirteen
    ReLUs), biases N(0, 0.1^2).  ``lin`` weights are U(0, 0.6): non-negative, as the trained ones are, and a pair of unrelated images lands near the
    0.1 .. 1 a real LPIPS reports.  ``spelling='torchvision'`` names the trunk ``features.N.*`` as torchvision's vgg16 does (the real LPIPS checkpoint
    holds only the lin layers); ``scaling=False`` leaves the ScalingLayer buffers out (the loader then takes the constants)."""
    if spelling not in ("lpips", "torchvision"):
        raise ValueError(f"spelling {spelling!r}: 'lpips' or 'torchvision'")
    r = _Rng(seed)
    sd: Dict[str, torch.Tensor] = {}
    if scaling:
        sd["scaling_layer.shift"] = torch.tensor([-.030, -.088, -.188]).view(1, 3, 1, 1)
        sd["scaling_layer.scale"] = torch.tensor([.458, .448, .450]).view(1, 3, 1, 1)
    for s, ((ci, co, _), idx) in enumerate(zip(HED_BLOCKS, LPIPS_FEATURES), 1):
        for i, n in enumerate(idx):
            cin = ci if i == 0 else co
            key = f"net.slice{s}.{n}" if spelling == "lpips" else f"features.{n}"
            sd[key + ".weight"] = r.normal(co, cin, 3, 3, std=(2.0 / (cin * 9)) ** 0.5)
            sd[key + ".bias"] = r.normal(co, std=0.1)
    for l, (_, co, _) in enumerate(HED_BLOCKS):
        sd[f"lin{l}.model.1.weight"] = r.uniform(1, co, 1, 1, lo=0.0, hi=0.6)
    return sd


def dpt_state_dict(cfg: DPTConfig, seed: int = 13) -> Dict[str, torch.Tensor]:
    """DPTForDepthEstimation(cfg).state_dict() names and shapes (transformers modeling_dpt.py, non-hybrid, readout 'project').  The stock initialisation
    (std 0.02, zero biases, zero position embeddings) gives a nearly constant map; here weights are N(0, 1/fan_in) (a ConvTranspose2d whose kernel equals
    its stride sees Cin inputs per output), biases 0.1 N(0,1), LayerNorm weights 1 + 0.1 N(0,1), cls and position embeddings 0.5 N(0,1), and the last
    bias is 1 so that the final ReLU clips only part of the map."""
    r = _Rng(seed)
    D, I, F = cfg.hidden_size, cfg.intermediate_size, cfg.fusion_hidden_size
    sd: Dict[str, torch.Tensor] = {}

    def lin(name, co, ci):
        sd[name + ".weight"] = r.normal(co, ci, std=ci ** -0.5)
        sd[name + ".bias"] = r.normal(co, std=0.1)

    def conv(name, co, ci, k, bias=True):
        sd[name + ".weight"] = r.normal(co, ci, k, k, std=(ci * k * k) ** -0.5)
        if bias:
            sd[name + ".bias"] = r.normal(co, std=0.1)

    def ln(name):
        sd[name + ".weight"] = 1.0 + r.normal(D, std=0.1)
        sd[name + ".bias"] = r.normal(D, std=0.1)

    sd["dpt.embeddings.cls_token"] = r.normal(1, 1, D, std=0.5)
    sd["dpt.embeddings.position_embeddings"] = r.normal(1, cfg.pos_grid ** 2 + 1, D, std=0.5)
    conv("dpt.embeddings.patch_embeddings.projection", D, 3, cfg.patch_size)
    for l in range(cfg.num_hidden_layers):
        p = f"dpt.encoder.layer.{l}."
        for m in ("query", "key", "value"):
            lin(p + "attention.attention." + m, D, D)
        lin(p + "attention.output.dense", D, D)
        lin(p + "intermediate.dense", I, D)
        lin(p + "output.dense", D, I)
        ln(p + "layernorm_before")
        ln(p + "layernorm_after")
    ln("dpt.layernorm")                                     # part of the state dict; never reaches the depth map
    for i, (c, f) in enumerate(zip(cfg.neck_hidden_sizes, cfg.reassemble_factors)):
        p = f"neck.reassemble_stage.layers.{i}."
        conv(p + "projection", c, D, 1)
        if f > 1:
            k = int(f)
            sd[p + "resize.weight"] = r.normal(c, c, k, k, std=c ** -0.5)       # [Cin, Cout, k, k]
            sd[p + "resize.bias"] = r.normal(c, std=0.1)
        elif f < 1:
            conv(p + "resize", c, c, 3)
    for i in range(4):
        lin(f"neck.reassemble_stage.readout_projects.{i}.0", D, 2 * D)
    for i, c in enumerate(cfg.neck_hidden_sizes):
        conv(f"neck.convs.{i}", F, c, 3, bias=False)
    for i in range(4):
        p = f"neck.fusion_stage.layers.{i}."
        conv(p + "projection", F, F, 1)
        for u in ("residual_layer1", "residual_layer2"):
            conv(p + u + ".convolution1", F, F, 3)
            conv(p + u + ".convolution2", F, F, 3)
    conv("head.head.0", F // 2, F, 3)
    conv("head.head.2", 32, F // 2, 3)
    conv("head.head.4", 1, 32, 1)
    sd["head.head.4.bias"] = torch.ones(1)
    return sd
