"""generate() with the reference signature (autoregressive/models/generate.py:134-204), running the whole
loop in libcontrolar_hip.so.  Callers that keep working unchanged: sample_t2i.py:163, sample_t2i_MR.py:184,
test_t2i.py:220, demo/model.py:156,250."""
from __future__ import annotations

import torch

from .models import Transformer, _PendingControl


def _call_seed(kw) -> int:
    """Seed of the library's counter-based RNG for this call.  The reference draws from torch's global generator
    (torch.multinomial, generate.py:72), so consecutive calls differ and torch.manual_seed() reproduces a run; the same holds
    here: without an explicit `seed` kwarg (an extension) one 62-bit value is drawn from torch's CPU generator per call."""
    if "seed" in kw and kw["seed"] is not None:
        return _arg(kw["seed"], int)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def _arg(v, cast):
    """One value for the call -> cast(v); one value per image (list, tuple, 1-D tensor) -> passed through for Engine's row table."""
    if isinstance(v, (list, tuple)) or (torch.is_tensor(v) and v.dim() == 1):
        return v
    return cast(v)


@torch.no_grad()
def generate(model: Transformer, cond, max_new_tokens, emb_masks=None, cfg_scale=1.0, cfg_interval=-1, condition=None,
             condition_null=None, condition_token_nums=0, control_strength=1, **sampling_kwargs):
    """Returns int32 [B, max_new_tokens] on cond.device.  sampling_kwargs: temperature, top_k (default 2000 as sample(),
    generate.py:59), top_p, sample_logits (default True), and the extensions seed and rng_stream.  `condition` is the control image [B,3,H,W] in
    [-1,1] (or None).  cfg_scale, cfg_interval, control_strength and every sampling kwarg may be one value or one per image (list, tuple or 1-D tensor
    of length B): Engine.generate then takes the row-table entry (car_generate_rows)."""
    if model.model_type not in ("t2i", "c2i"):
        raise Exception("please check model type")
    eng = model.engine
    if condition is not None:
        if isinstance(condition, _PendingControl):
            condition = condition.img
        eng.encode_control(condition)                       # model.adapter + model.adapter_mlp (generate.py:136-138)
    if emb_masks is not None:
        assert emb_masks.shape[0] == cond.shape[0]          # generate.py:185-186
        assert emb_masks.shape[-1] == (1 + condition_token_nums if model.model_type == "c2i" else cond.shape[1])
    if model.model_type == "c2i" and condition_token_nums != 0:
        raise RuntimeError("c2i: condition_token_nums must be 0 (the only value the reference samplers pass, sample_c2i.py:55)")
    out = eng.generate(cond, int(max_new_tokens), emb_masks, cfg_scale=_arg(cfg_scale, float), cfg_interval=_arg(cfg_interval, int),
                       use_control=condition is not None, control_strength=_arg(control_strength, float),
                       temperature=_arg(sampling_kwargs.get("temperature", 1.0), float), top_k=_arg(sampling_kwargs.get("top_k", 2000), lambda k: int(k or 0)),
                       top_p=_arg(sampling_kwargs.get("top_p", 1.0), float), sample_logits=_arg(sampling_kwargs.get("sample_logits", True), bool),
                       seed=_call_seed(sampling_kwargs), rng_stream=sampling_kwargs.get("rng_stream"))
    return out.to(cond.device)


def score_loss(nll: torch.Tensor, valid=None) -> torch.Tensor:
    """The loss Transformer.forward returns next to its logits (gpt_t2i.py:472-481), from per-token nll [B,N]: the mean, or with valid [B] the
    valid-weighted sum over max(valid.sum() * N, 1) — the reference's (valid_all * loss_all).sum() / max(valid_all.sum(), 1) with valid repeated over
    the N positions.  Reduced in fp64 on nll's device; a 0-d fp64 tensor."""
    x = nll.to(torch.float64)
    if valid is None:
        return x.mean()
    v = torch.as_tensor(valid).to(device=x.device, dtype=torch.float64).reshape(-1)
    assert v.shape[0] == x.shape[0]
    return (x * v[:, None]).sum() / torch.clamp(v.sum() * x.shape[1], min=1.0)


@torch.no_grad()
def score(model: Transformer, cond, tokens, emb_masks=None, cfg_scale=1.0, cfg_interval=-1, condition=None, control_strength=1, valid=None):
    """Teacher-forced scoring with generate()'s argument conventions: Transformer.forward(idx, cond_idx, targets=tokens, valid=valid, condition=...)
    evaluated in one parallel pass (car_score).  Returns (nll [B,N] fp32 on cond.device, loss): nll[b,i] = -log p(tokens[b,i] | prompt, control,
    tokens[b,:i]) under the logits generate() samples from (after the CFG mix, before temperature / top-k / top-p); loss = score_loss(nll, valid)."""
    if model.model_type != "t2i":
        raise Exception("please check model type")          # scoring covers the t2i model
    eng = model.engine
    if condition is not None:
        if isinstance(condition, _PendingControl):
            condition = condition.img
        eng.encode_control(condition)                       # model.adapter + model.adapter_mlp (generate.py:136-138)
    if emb_masks is not None:
        assert emb_masks.shape[0] == cond.shape[0] and emb_masks.shape[-1] == cond.shape[1]          # generate.py:185-186
    nll = eng.score(cond, tokens, emb_masks, cfg_scale=_arg(cfg_scale, float), cfg_interval=_arg(cfg_interval, int), use_control=condition is not None,
                    control_strength=_arg(control_strength, float))
    loss = score_loss(nll, valid)
    return nll.to(cond.device), loss.to(cond.device)
