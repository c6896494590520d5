"""Thin host-side wrapper over the C ABI: owns one car_ctx, feeds it reference-named weights,
hands it data_ptr()s of PyTorch-ROCm tensors on the current stream.  PyTorch here is plumbing
(device memory + streams); all arithmetic of the path runs in libcontrolar_hip.so."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _lib as L
from .config import PathConfig


# Image.resize filters by name -> Pillow's integer codes, which are car_resize's (NEAREST = 0 is refused by the library)
RESAMPLE_CODES = {"nearest": 0, "lanczos": L.CAR_FILTER_LANCZOS, "bilinear": L.CAR_FILTER_BILINEAR, "bicubic": L.CAR_FILTER_BICUBIC,
                  "box": L.CAR_FILTER_BOX, "hamming": L.CAR_FILTER_HAMMING}


def _stream_ptr() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return L.CAR_DT_F32
    if t.dtype == torch.bfloat16:
        return L.CAR_DT_BF16
    raise TypeError(f"unsupported tensor dtype {t.dtype} (float32 or bfloat16)")


def first_valid_position(emb_masks: torch.Tensor) -> int:
    """First attendable prompt position over a batch of LEFT-padded caption masks [B, T] (sample_t2i.py:146-160): min over the rows of the index of the first
    non-zero entry; a row without any valid token counts as T.  This is what `car_sampling.first_valid_hint - 1` carries: the prefill window of car_generate
    starts at the multiple of 16 at or below it.  One reduction — free on a host mask, one sync on a device mask (do it once, outside a timed loop)."""
    B, T = emb_masks.shape
    nz = emb_masks != 0
    first = torch.where(nz.any(dim=1), nz.to(torch.int64).argmax(dim=1), torch.full((B,), T, device=emb_masks.device))
    return int(first.min())


def _per_image(v):
    """A per-image argument: a list / tuple or a 1-D tensor -> a Python list; one value for the whole call (a 0-d tensor included) -> None."""
    if torch.is_tensor(v):
        return v.tolist() if v.dim() == 1 else None
    return list(v) if isinstance(v, (list, tuple)) else None


def sampling_rows(B: int, rng_stream=None, **params):
    """The row table of a car_*_rows call, or None for the plain call.  `params`: cfg_scale, cfg_interval, temperature, top_k, top_p, sample_logits, seed,
    control_strength, each one value for the whole call or one per image (list, tuple or 1-D tensor of length B); rng_stream: None, one value or one
    per image — the first word of an image's Philox counter, 0 per image unless given, so that a request draws the same numbers wherever it sits in a
    batch.  All scalars and no rng_stream -> None (the existing entry points, unchanged).  Anything else -> a (CarSamplingRow * B) array with the
    scalars broadcast.  Raises ValueError, before the library is entered, on a length other than B and on rows that disagree about cfg_scale > 1:
    the CFG batch doubling is call-wide."""
    cols = {k: _per_image(v) for k, v in params.items()}
    streams = _per_image(rng_stream)
    if rng_stream is None and all(c is None for c in cols.values()):
        return None
    for name, c in list(cols.items()) + [("rng_stream", streams)]:
        if c is not None and len(c) != B:
            raise ValueError(f"{name} has {len(c)} entries for a batch of {B} images")
    at = lambda name, i: cols[name][i] if cols[name] is not None else params[name]
    rows = (L.CarSamplingRow * B)()
    for i, r in enumerate(rows):
        r.cfg_scale, r.cfg_interval, r.temperature, r.top_k = float(at("cfg_scale", i)), int(at("cfg_interval", i)), float(at("temperature", i)), int(at("top_k", i) or 0)
        r.top_p, r.sample_logits, r.seed = float(at("top_p", i)), int(bool(at("sample_logits", i))), int(at("seed", i)) & (2 ** 64 - 1)
        r.control_strength = float(at("control_strength", i))
        r.rng_stream = int(streams[i] if streams is not None else (rng_stream or 0)) & (2 ** 32 - 1)
    over = [r.cfg_scale > 1.0 for r in rows]
    if any(over) != all(over):
        raise ValueError("cfg_scale: the rows of one call must either all be > 1 or all be <= 1 (the CFG batch doubling is call-wide; a row at scale 1 "
                         "inside a CFG batch would compute u + (c - u) * 1, which is not c in fp32)")
    return rows


class Engine:
    """One context = one set of weights in one arithmetic mode ('fp32' exact | 'bf16' fast)."""

    sampling_rows = staticmethod(sampling_rows)

    def __init__(self, cfg: PathConfig, precision: str = "bf16", device: Optional[torch.device] = None, stream_priority: int = 0,
                 weights_fp8: bool = False, kv_fp8: bool = False, dev: Optional[bool] = None, vq_split: bool = False):
        # dev=True: the development build of the library (the CAR_* A/B switches exist only there; default: CONTROLAR_DEV_LIB=1 in the environment)
        self.lib = L.load(dev)
        if not torch.cuda.is_available():
            raise RuntimeError("controlar_amd needs a HIP device (no CPU fallback)")
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise RuntimeError(f"controlar_amd runs on a HIP device only, got {dev}")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        torch.cuda.set_device(self.device)
        self.cfg = cfg
        self.precision = precision
        self.mode = {"fp32": L.CAR_F32, "none": L.CAR_F32, "bf16": L.CAR_BF16}[precision]
        if vq_split and self.mode != L.CAR_F32:
            raise ValueError("vq_split=True (car_config.vq_split_bf16) is an option of the fp32 mode: the bf16 mode decodes on bf16 operands already")
        self.dtype = torch.float32 if self.mode == L.CAR_F32 else torch.bfloat16
        g, v, q = cfg.gpt, cfg.vit, cfg.vq
        cc = L.CarConfig()
        cc.abi_version, cc.mode = L.CAR_ABI_VERSION, self.mode
        cc.dim, cc.n_layer, cc.n_head, cc.ffn_hidden, cc.vocab_size = g.dim, g.n_layer, g.n_head, g.ffn_hidden, g.vocab_size
        cc.cls_token_num, cc.block_size, cc.caption_dim = g.cls_token_num, g.block_size, g.caption_dim
        cc.norm_eps, cc.rope_base = g.norm_eps, g.rope_base
        cc.vit_hidden, cc.vit_layers, cc.vit_heads, cc.vit_mlp = v.hidden, v.layers, v.heads, v.mlp
        cc.vit_patch, cc.vit_pos_grid, cc.vit_ln_eps = v.patch, v.pos_grid, v.ln_eps
        # dinov2_adapter.py:19-23: nearest for canny/seg, bicubic(align_corners=True) otherwise; the c2i ViT adapter
        # (vit_adapter.py:13-15) does not resize: nearest onto the same grid is the identity
        vit16 = getattr(v, "variant", "dinov2") == "vit"
        cc.resize_mode = L.CAR_RESIZE_NEAREST if (vit16 or g.condition_type in ("canny", "seg")) else L.CAR_RESIZE_BICUBIC_AC
        cc.vit_variant = 1 if vit16 else 0
        cc.model_type = 1 if g.model_type == "c2i" else 0
        cc.num_classes = g.num_classes
        cc.stream_priority = int(stream_priority)
        # BASELINE config 5; bf16 mode only.  True / 1 = weight-only e4m3 (bf16 MFMA); 'mfma' / 2 = W8A8 on the fp8 MFMA
        cc.decode_weight_fp8 = 2 if weights_fp8 in ("mfma", 2) else int(bool(weights_fp8))
        # opt-in e4m3 KV cache (bf16 mode only; bf16 KV is the default and the parity path): halves the KV stream, doubles the sequences that fit
        cc.kv_cache_fp8 = int(bool(kv_fp8))
        # opt-in split-bf16 VQ decoder (fp32 mode only): each fp32 conv / GEMM operand as two bf16 numbers, three bf16 MFMAs per product — fp32-grade pixels
        # (the exact decoder's tolerance against the reference) at a multiple of the fp32 MFMA's rate; vq_encode, generate and encode_control are untouched
        cc.vq_split_bf16 = int(bool(vq_split))
        cc.codebook_size, cc.codebook_dim, cc.z_channels, cc.vq_ch = q.codebook_size, q.codebook_embed_dim, q.z_channels, q.ch
        cc.vq_num_res_blocks, cc.vq_n_mult, cc.gn_eps = q.num_res_blocks, len(q.ch_mult), q.gn_eps
        for i, m in enumerate(q.ch_mult):
            cc.vq_ch_mult[i] = m
        self._cc = cc
        h = C.c_void_p()
        rc = self.lib.car_create(C.byref(h), C.byref(cc))
        if rc != 0:
            raise RuntimeError("car_create: " + self.lib.car_last_error(None).decode())
        self._h = h

    # ------------------------------------------------------------------ errors / lifecycle
    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what}: {self.lib.car_last_error(self._h).decode()}")

    def _prompt_mask(self, who: str, emb_masks, B: int, T: int, first_valid):
        """The pad mask of generate / score (`who`) as a device int64 tensor, and car_sampling.first_valid_hint: the caller's `first_valid` clamped to [0, T], plus
        one; 0 without a mask or a value.  A mask that is still on the host supplies the value for free, and a caller's value is checked against it."""
        if emb_masks is None:
            return None, 0
        assert emb_masks.shape[0] == B and emb_masks.shape[-1] == T          # generate.py:185-186
        if emb_masks.device.type == "cpu" and emb_masks.numel():
            true_first = first_valid_position(emb_masks.reshape(B, T))
            if first_valid is not None and int(first_valid) > true_first:
                raise RuntimeError(f"{who}: first_valid={int(first_valid)} is beyond the first valid prompt position of the batch ({true_first}): valid rows would be dropped")
            if first_valid is None:
                first_valid = true_first
        mask_t = emb_masks.to(device=self.device, dtype=torch.int64).contiguous()
        return mask_t, (0 if first_valid is None else max(0, min(int(first_valid), T)) + 1)

    def close(self):
        """Destroys the context.  A device-side error that no entry could report synchronously (wrong first_valid hint, out-of-range device label) is raised here
        at the latest — after the context is gone, so that close() always releases the memory."""
        if getattr(self, "_h", None):
            h, self._h = self._h, None
            rc, msg = 0, ""
            try:
                rc = self.lib.car_check_errors(h)
                if rc:
                    msg = (self.lib.car_last_error(h) or b"").decode(errors="replace")
            finally:
                self.lib.car_destroy(h)
            if rc:
                raise RuntimeError(f"car_check_errors at close(): {msg}")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd: Dict[str, torch.Tensor], finalize: bool = False):
        """Accepts the reference's state_dict names (gpt_t2i.Transformer incl. adapter.model.*, VQModel)."""
        for name, t in sd.items():
            if not torch.is_floating_point(t):
                continue
            t = t.detach()
            if t.dtype not in (torch.float32, torch.bfloat16):
                t = t.float()
            t = t.contiguous()
            shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
            self._check(self.lib.car_load_tensor(self._h, name.encode(), C.c_void_p(t.data_ptr()), shape, t.dim(), _dt(t)),
                        f"car_load_tensor({name})")
        if finalize:
            self.finalize()

    def finalize(self):
        self._check(self.lib.car_finalize_weights(self._h), "car_finalize_weights")

    # ------------------------------------------------------------------ path stages
    def encode_control(self, img: torch.Tensor, want_output: bool = False) -> Optional[torch.Tensor]:
        """model.adapter_mlp(model.adapter(img))  (generate.py:136-138).  img [B,3,H,W] in [-1,1]."""
        assert img.dim() == 4 and img.shape[1] == 3
        img = img.to(self.device)
        if img.dtype not in (torch.float32, torch.bfloat16):
            img = img.float()
        img = img.contiguous()
        B, _, H, W = img.shape
        out = None
        if want_output:
            out = torch.empty(B, (H // 16) * (W // 16), self.cfg.gpt.dim, dtype=self.dtype, device=self.device)
        self._check(self.lib.car_encode_control(self._h, C.c_void_p(img.data_ptr()), _dt(img), B, H, W,
                                                C.c_void_p(out.data_ptr() if out is not None else 0), C.c_void_p(_stream_ptr())),
                    "car_encode_control")
        return out

    def generate(self, cond: torch.Tensor, max_new_tokens: int, emb_masks: Optional[torch.Tensor] = None,
                 cfg_scale: float = 1.0, cfg_interval: int = -1, use_control: bool = True, control_strength: float = 1.0,
                 temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, sample_logits: bool = False, seed: int = 0,
                 forced_tokens: Optional[torch.Tensor] = None, return_logits: bool = False, first_valid: Optional[int] = None, rng_stream=None):
        """cfg_scale, cfg_interval, control_strength, temperature, top_k, top_p, sample_logits and seed each take one value for the call or one per
        image (a length-B list, tuple or 1-D tensor); with any of them per image, or with `rng_stream` given (one value or one per image; 0 per image
        otherwise), the call goes through car_generate_rows / car_generate_c2i_rows with the scalars broadcast (sampling_rows above): an image's
        result is then a function of its own row alone — in the fp32 mode bit for bit, whatever the batch around it.
        `first_valid`: a lower bound of the first valid (unpadded) prompt position over the batch, if the caller knows it — car_generate then sizes its prefill
        window without reading the device mask back (no host wait).  A mask that is still on the host supplies it for free, and a caller-supplied value is
        checked against such a mask here.  With a DEVICE mask a value that is too large cannot be seen without the host wait the hint exists to avoid: the
        device raises a sticky error flag, and it surfaces at the NEXT entry into the context, at stats(), check_errors() or close() — the tokens of the
        offending call are invalid."""
        c2i = self.cfg.gpt.model_type == "c2i"
        if c2i and cond.device.type == "cpu" and cond.numel():
            # labels that are still on the host are checked for free; device-resident labels are checked on the device (sticky flag, stats())
            lo, hi = int(cond.min()), int(cond.max())
            if lo < 0 or hi > self.cfg.gpt.num_classes:
                raise RuntimeError(f"car_generate_c2i: class label out of range [0,{self.cfg.gpt.num_classes}] (got {lo}..{hi})")
        cond = cond.to(self.device)
        if c2i:
            cond = cond.to(torch.int64).contiguous().view(-1)          # class labels [B]
            B, T = cond.shape[0], 1
        else:
            if cond.dtype not in (torch.float32, torch.bfloat16):
                cond = cond.float()
            cond = cond.contiguous()
            B, T, cap = cond.shape
            assert T == self.cfg.gpt.cls_token_num and cap == self.cfg.gpt.caption_dim
        mask_t, hint = self._prompt_mask("generate", emb_masks, B, T, first_valid)
        rows = sampling_rows(B, rng_stream, cfg_scale=cfg_scale, cfg_interval=cfg_interval, temperature=temperature, top_k=top_k, top_p=top_p,
                             sample_logits=sample_logits, seed=seed, control_strength=control_strength)
        sp = L.CarSampling()
        sp.first_valid_hint = hint
        if rows is None:
            sp.cfg_scale, sp.cfg_interval, sp.temperature, sp.top_k = float(cfg_scale), int(cfg_interval), float(temperature), int(top_k or 0)
            sp.top_p, sp.sample_logits, sp.seed, sp.control_strength = float(top_p), int(bool(sample_logits)), int(seed), float(control_strength)
        out = torch.empty(B, max_new_tokens, dtype=torch.int32, device=self.device)
        forced = None
        if forced_tokens is not None:
            forced = forced_tokens.to(device=self.device, dtype=torch.int32).contiguous()
        logits = torch.empty(B, max_new_tokens, self.cfg.gpt.vocab_size, dtype=torch.float32, device=self.device) if return_logits else None
        # the *_rows entries with rows = NULL are the plain calls (include/controlar_hip.h); errors keep the plain entry's name then
        tail = (C.byref(sp), rows, C.c_void_p(out.data_ptr()), C.c_void_p(forced.data_ptr() if forced is not None else 0),
                C.c_void_p(logits.data_ptr() if logits is not None else 0), C.c_void_p(_stream_ptr()))
        sfx = "_rows" if rows is not None else ""
        if c2i:
            self._check(self.lib.car_generate_c2i_rows(self._h, C.c_void_p(cond.data_ptr()), B, int(max_new_tokens), int(bool(use_control)), *tail),
                        "car_generate_c2i" + sfx)
        else:
            self._check(self.lib.car_generate_rows(self._h, C.c_void_p(cond.data_ptr()), _dt(cond), C.c_void_p(mask_t.data_ptr() if mask_t is not None else 0),
                                                   B, int(max_new_tokens), int(bool(use_control)), *tail), "car_generate" + sfx)
        return (out, logits) if return_logits else out

    def score(self, cond: torch.Tensor, tokens: torch.Tensor, emb_masks: Optional[torch.Tensor] = None, cfg_scale: float = 1.0,
              cfg_interval: int = -1, use_control: bool = True, control_strength: float = 1.0, return_logits: bool = False,
              first_valid: Optional[int] = None):
        """Per-token negative log-likelihood of `tokens` [B,N] under the prompt `cond` (and the control of the preceding encode_control) in one parallel
        pass (car_score): nll[b,i] = logsumexp(l_i) - l_i[tokens[b,i]] with l_i the logits row generate() would sample step i from after feeding back
        tokens[b,:i] (after the CFG mix, before temperature / top-k / top-p).  Returns fp32 [B,N], or (nll, logits [B,N,V]) with return_logits.  The other
        arguments mean what they mean to generate(); cfg_scale, cfg_interval and control_strength may be given per image (car_score_rows).  A token id outside [0, vocab) on a host tensor raises here; on a device tensor it raises the sticky
        flag (check_errors)."""
        if self.cfg.gpt.model_type == "c2i":
            raise RuntimeError("car_score: context was created for the c2i model; scoring covers the t2i model only")
        if not torch.is_tensor(cond) or cond.dim() != 3:
            raise ValueError(f"score: cond must be [B,T,caption_dim], got {tuple(getattr(cond, 'shape', ()))}")
        B, T, cap = cond.shape
        if T != self.cfg.gpt.cls_token_num or cap != self.cfg.gpt.caption_dim:
            raise ValueError(f"score: cond must be [B,{self.cfg.gpt.cls_token_num},{self.cfg.gpt.caption_dim}], got {tuple(cond.shape)}")
        if not torch.is_tensor(tokens) or tokens.dim() != 2 or tokens.shape[0] != B or tokens.shape[1] < 1 or tokens.dtype.is_floating_point:
            raise ValueError(f"score: tokens must be an integer tensor [B={B},N], got {tuple(getattr(tokens, 'shape', ()))}")
        N = int(tokens.shape[1])
        if tokens.device.type == "cpu":
            lo, hi = int(tokens.min()), int(tokens.max())
            if lo < 0 or hi >= self.cfg.gpt.vocab_size:
                raise RuntimeError(f"car_score: token id out of range [0,{self.cfg.gpt.vocab_size}) (got {lo}..{hi})")
        cond = cond.to(self.device)
        if cond.dtype not in (torch.float32, torch.bfloat16):
            cond = cond.float()
        cond = cond.contiguous()
        mask_t, hint = self._prompt_mask("score", emb_masks, B, T, first_valid)
        rows = sampling_rows(B, None, cfg_scale=cfg_scale, cfg_interval=cfg_interval, temperature=1.0, top_k=0, top_p=1.0, sample_logits=False, seed=0,
                             control_strength=control_strength)
        sp = L.CarSampling()
        sp.first_valid_hint = hint
        if rows is None:
            sp.cfg_scale, sp.cfg_interval, sp.temperature, sp.top_k = float(cfg_scale), int(cfg_interval), 1.0, 0
            sp.top_p, sp.sample_logits, sp.seed, sp.control_strength = 1.0, 0, 0, float(control_strength)
        tok = tokens.to(device=self.device, dtype=torch.int32).contiguous()
        nll = torch.empty(B, N, dtype=torch.float32, device=self.device)
        logits = torch.empty(B, N, self.cfg.gpt.vocab_size, dtype=torch.float32, device=self.device) if return_logits else None
        self._check(self.lib.car_score_rows(self._h, C.c_void_p(cond.data_ptr()), _dt(cond), C.c_void_p(mask_t.data_ptr() if mask_t is not None else 0),
                                            B, N, int(bool(use_control)), C.byref(sp), rows, C.c_void_p(tok.data_ptr()), C.c_void_p(nll.data_ptr()),
                                            C.c_void_p(logits.data_ptr() if logits is not None else 0), C.c_void_p(_stream_ptr())),
                    "car_score_rows" if rows is not None else "car_score")
        return (nll, logits) if return_logits else nll

    def score_rows(self, x: torch.Tensor, w: torch.Tensor, targets: torch.Tensor, pair_scale: Optional[torch.Tensor] = None,
                   round_bf16: bool = False, return_logits: bool = False):
        """The fused vocabulary projection + cross-entropy kernel alone (car_debug_score_rows; tests).  x [R,D], w [V,D] are converted to the context's
        element type.  Without pair_scale: targets [R] -> nll [R].  With pair_scale [R/2]: rows [0,R/2) conditional, [R/2,R) unconditional, targets and
        nll have R/2 rows."""
        x = x.to(device=self.device, dtype=self.dtype).contiguous()
        w = w.to(device=self.device, dtype=self.dtype).contiguous()
        R, D = x.shape
        V = w.shape[0]
        assert w.shape[1] == D
        Ro = R // 2 if pair_scale is not None else R
        t = targets.to(device=self.device, dtype=torch.int32).contiguous()
        assert t.numel() == Ro
        ps = None
        if pair_scale is not None:
            ps = pair_scale.to(device=self.device, dtype=torch.float32).contiguous()
            assert ps.numel() == Ro
        nll = torch.empty(Ro, dtype=torch.float32, device=self.device)
        logits = torch.empty(Ro, V, dtype=torch.float32, device=self.device) if return_logits else None
        self._check(self.lib.car_debug_score_rows(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()), C.c_void_p(t.data_ptr()),
                                                  C.c_void_p(ps.data_ptr() if ps is not None else 0), R, V, D, int(bool(round_bf16)),
                                                  C.c_void_p(nll.data_ptr()), C.c_void_p(logits.data_ptr() if logits is not None else 0),
                                                  C.c_void_p(_stream_ptr())), "car_debug_score_rows")
        return (nll, logits) if return_logits else nll

    def sample(self, logits: torch.Tensor, cfg_scale: float = 1.0, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
               sample_logits: bool = True, seed: int = 0, step: int = 0, cfg_interval: int = -1, rng_stream=None) -> torch.Tensor:
        """generate.py:59-74 sample() on caller-provided fp32 logits [rows, V] (rows = 2B under CFG) -> int32 [B].  Every sampling argument takes one
        value or one per image, and `rng_stream` one value or one per image, as in generate(): car_sample_logits_rows.  `step` stands for the loop
        index + 1 of the token loop: the CFG mix is dropped where cfg_interval > -1 and step - 1 > cfg_interval."""
        logits = logits.to(device=self.device, dtype=torch.float32).contiguous()
        rows, V = logits.shape
        scales = _per_image(cfg_scale)
        B = rows // 2 if (scales[0] if scales else cfg_scale) > 1.0 else rows
        tab = sampling_rows(B, rng_stream, cfg_scale=cfg_scale, cfg_interval=cfg_interval, temperature=temperature, top_k=top_k, top_p=top_p,
                            sample_logits=sample_logits, seed=seed, control_strength=1.0)
        sp = L.CarSampling()
        out = torch.empty(B, dtype=torch.int32, device=self.device)
        if tab is not None:
            self._check(self.lib.car_sample_logits_rows(self._h, C.c_void_p(logits.data_ptr()), B, V, C.byref(sp), tab, int(step),
                                                        C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr())), "car_sample_logits_rows")
            return out
        sp.cfg_scale, sp.cfg_interval, sp.temperature, sp.top_k = float(cfg_scale), int(cfg_interval), float(temperature), int(top_k or 0)
        sp.top_p, sp.sample_logits, sp.seed, sp.control_strength = float(top_p), int(bool(sample_logits)), int(seed), 1.0
        self._check(self.lib.car_sample_logits(self._h, C.c_void_p(logits.data_ptr()), B, V, C.byref(sp), int(step),
                                               C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr())), "car_sample_logits")
        return out

    def vq_decode(self, tokens: torch.Tensor, h: int, w: int) -> torch.Tensor:
        """VQModel.decode_code(tokens, [B,C,h,w]) -> fp32 [B,3,16h,16w]  (vq_model.py:53-56)."""
        tokens = tokens.to(device=self.device, dtype=torch.int32).contiguous().view(-1, h * w)
        B = tokens.shape[0]
        up = 2 ** (len(self.cfg.vq.ch_mult) - 1)
        out = torch.empty(B, 3, h * up, w * up, dtype=torch.float32, device=self.device)
        self._check(self.lib.car_vq_decode(self._h, C.c_void_p(tokens.data_ptr()), B, h, w, C.c_void_p(out.data_ptr()),
                                           C.c_void_p(_stream_ptr())), "car_vq_decode")
        return out

    def vq_encode(self, img: torch.Tensor) -> torch.Tensor:
        """VQModel.encode(img) -> min_encoding_indices int32 [B, (H/16)(W/16)]  (vq_model.py:41-46)."""
        img = img.to(device=self.device, dtype=torch.float32).contiguous()
        B, _, H, W = img.shape
        down = 2 ** (len(self.cfg.vq.ch_mult) - 1)
        out = torch.empty(B, (H // down) * (W // down), dtype=torch.int32, device=self.device)
        self._check(self.lib.car_vq_encode(self._h, C.c_void_p(img.data_ptr()), B, H, W, C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr())),
                    "car_vq_encode")
        return out

    def canny(self, img: torch.Tensor, low_threshold: float = 100, high_threshold: float = 200, want_control: bool = False):
        """cv2.Canny(img, low, high) of condition/canny.py:6-14 on the GPU.  img uint8 [B,H,W,3] (or [H,W,3]) -> uint8 [B,H,W] in
        {0,255}; with want_control also the control tensor [B,3,H,W] = 2*(edges/255-0.5) (sample_t2i.py:125,141)."""
        single = img.dim() == 3
        x = (img[None] if single else img).to(device=self.device, dtype=torch.uint8).contiguous()
        B, H, W, ch = x.shape
        assert ch == 3, "expected an RGB image [.., H, W, 3]"
        edges = torch.empty(B, H, W, dtype=torch.uint8, device=self.device)
        ctrl = torch.empty(B, 3, H, W, dtype=self.dtype, device=self.device) if want_control else None
        self._check(self.lib.car_canny(self._h, C.c_void_p(x.data_ptr()), B, H, W, float(low_threshold), float(high_threshold),
                                       C.c_void_p(edges.data_ptr()), C.c_void_p(ctrl.data_ptr() if ctrl is not None else 0), C.c_void_p(_stream_ptr())),
                    "car_canny")
        edges = edges[0] if single else edges
        return (edges, ctrl) if want_control else edges

    def resize(self, img: torch.Tensor, size, resample="bicubic", box=None, want_control: bool = False, want_float=None):
        """PIL's Image.resize(size, resample, box) on 8-bit images, bit for bit, on the GPU (car_resize).  img uint8 [B,H,W,C], [H,W,C] or [H,W], C in
        {1, 3}; size = (W, H) as PIL orders it; resample: a name ('lanczos', 'bilinear', 'bicubic', 'box', 'hamming') or Pillow's integer code; box =
        (x0, y0, x1, y1) in source pixels.  Returns the uint8 result in the input's layout; with want_control also the control tensor [B,3,Ho,Wo] =
        2*(x/255-0.5) in the context's element type; with want_float ('raw' | 0: (float)x, 'norm' | 1: (x/255-0.5)/0.5) also fp32 [B,C,Ho,Wo]."""
        filt = RESAMPLE_CODES.get(resample.lower()) if isinstance(resample, str) else int(resample)
        if filt is None:
            raise ValueError(f"unknown resample filter {resample!r} (one of {sorted(RESAMPLE_CODES)})")
        if img.dim() not in (2, 3, 4):
            raise ValueError(f"expected a uint8 image [B,H,W,C], [H,W,C] or [H,W], got {tuple(img.shape)}")
        if img.dtype != torch.uint8:
            raise TypeError(f"resize takes 8-bit images (torch.uint8), got {img.dtype}")
        x = img.to(self.device)
        x = (x[None, :, :, None] if img.dim() == 2 else x[None] if img.dim() == 3 else x).contiguous()
        B, H, W, ch = x.shape
        Wo, Ho = int(size[0]), int(size[1])
        norm = None if want_float is None else {"raw": 0, "norm": 1, 0: 0, 1: 1}[want_float]
        ok = Ho > 0 and Wo > 0                                    # a refused call allocates nothing: the library reports the reason
        out = torch.empty(B, Ho, Wo, ch, dtype=torch.uint8, device=self.device) if ok else None
        ctrl = torch.empty(B, 3, Ho, Wo, dtype=self.dtype, device=self.device) if (want_control and ok) else None
        fl = torch.empty(B, ch, Ho, Wo, dtype=torch.float32, device=self.device) if (norm is not None and ok) else None
        cbox = None if box is None else (C.c_float * 4)(*[float(v) for v in box])
        self._check(self.lib.car_resize(self._h, C.c_void_p(x.data_ptr()), B, H, W, ch, Ho, Wo, filt, cbox,
                                        C.c_void_p(out.data_ptr() if out is not None else 0), C.c_void_p(ctrl.data_ptr() if ctrl is not None else 0),
                                        C.c_void_p(fl.data_ptr() if fl is not None else 0), norm or 0, C.c_void_p(_stream_ptr())), "car_resize")
        out = out[0, :, :, 0] if img.dim() == 2 else out[0] if img.dim() == 3 else out
        extra = tuple(t for t in (ctrl, fl) if t is not None)
        return (out,) + extra if extra else out

    # ------------------------------------------------------------------ control-consistency metrics (evaluations/*.py, autoregressive/test/metric.py)
    def _metric_input(self, t: torch.Tensor, what: str) -> torch.Tensor:
        """uint8 stays uint8, everything else becomes fp32; on the device, contiguous."""
        if not torch.is_tensor(t):
            raise TypeError(f"{what}: expected a tensor, got {type(t).__name__}")
        return t.to(device=self.device, dtype=torch.uint8 if t.dtype == torch.uint8 else torch.float32).contiguous()

    @staticmethod
    def _metric_dt(t: torch.Tensor) -> int:
        return L.CAR_DT_U8 if t.dtype == torch.uint8 else L.CAR_DT_F32

    def ms_ssim(self, pred: torch.Tensor, target: torch.Tensor, scale=None, want_scales: bool = False):
        """torchmetrics' MultiScaleStructuralSimilarityIndexMeasure(data_range=1.0) per image on the GPU (car_ms_ssim).  pred, target [B,C,H,W] (or
        [B,H,W] = one channel), each uint8 or float; an element's value is clip(v * scale, 0, 1).  scale: one number for both inputs, a pair
        (pred, target), or None = 1/255 for a uint8 input and 1 for a float one.  Returns fp64 [B]; with want_scales also fp64 [B,5,2], per scale the
        (ssim, cs) means after relu.  Sides below 176 raise ValueError, as torchmetrics does (side // 16 <= 10)."""
        if pred.shape != target.shape:
            raise ValueError(f"ms_ssim: pred and target differ in shape: {tuple(pred.shape)} and {tuple(target.shape)}")
        if pred.dim() == 3:
            pred, target = pred[:, None], target[:, None]
        if pred.dim() != 4:
            raise ValueError(f"ms_ssim: expected [B,C,H,W] or [B,H,W], got {tuple(pred.shape)}")
        B, ch, H, W = pred.shape
        if H < 32 or W < 32:
            raise ValueError(f"ms_ssim: with 5 scales both sides must be at least 32, got {H} x {W}")
        if H // 16 <= 10 or W // 16 <= 10:
            raise ValueError(f"ms_ssim: with 5 scales and an 11 x 11 window both sides must be at least 176 (side // 16 > 10), got {H} x {W}")
        if B == 0 or ch == 0:
            raise ValueError(f"ms_ssim: empty batch {tuple(pred.shape)}")
        p, t = self._metric_input(pred, "ms_ssim"), self._metric_input(target, "ms_ssim")
        sp, st = scale if isinstance(scale, (tuple, list)) else (scale, scale)
        sp = (1.0 / 255.0 if p.dtype == torch.uint8 else 1.0) if sp is None else float(sp)
        st = (1.0 / 255.0 if t.dtype == torch.uint8 else 1.0) if st is None else float(st)
        out = torch.empty(B, dtype=torch.float64, device=self.device)
        tab = torch.empty(B, 5, 2, dtype=torch.float64, device=self.device) if want_scales else None
        self._check(self.lib.car_ms_ssim(self._h, C.c_void_p(p.data_ptr()), self._metric_dt(p), C.c_void_p(t.data_ptr()), self._metric_dt(t), B, ch, H, W,
                                         sp, st, C.c_void_p(out.data_ptr()), C.c_void_p(tab.data_ptr() if tab is not None else 0),
                                         C.c_void_p(_stream_ptr())), "car_ms_ssim")
        return (out, tab) if want_scales else out

    @staticmethod
    def _f1_rule(value, threshold, what):
        if (value is None) == (threshold is None):
            raise ValueError(f"f1: give {what} exactly one rule, value= (positive where v == value) or threshold= (positive where v > threshold)")
        return (0, float(value)) if value is not None else (1, float(threshold))

    def f1(self, pred: torch.Tensor, target: torch.Tensor, value=None, threshold=None, target_value=None, target_threshold=None, want_counts: bool = False):
        """Binary F1 per image on the GPU (car_f1).  pred, target [B,H,W] (or [H,W]), each uint8 or float.  An element is positive where v == value
        (evaluations/canny_f1score.py: value=255) or where v > threshold (metric.py's F1score: threshold=128); target_value / target_threshold give the
        target a rule of its own, otherwise it shares pred's.  Returns fp64 [B] = 2TP / (2TP + FP + FN), 0 where that denominator is 0; with want_counts
        also int64 [B,3] = TP, FP, FN."""
        if pred.shape != target.shape:
            raise ValueError(f"f1: pred and target differ in shape: {tuple(pred.shape)} and {tuple(target.shape)}")
        single = pred.dim() == 2
        if single:
            pred, target = pred[None], target[None]
        if pred.dim() != 3 or pred.numel() == 0:
            raise ValueError(f"f1: expected non-empty [B,H,W] or [H,W], got {tuple(pred.shape)}")
        rp, vp = self._f1_rule(value, threshold, "pred")
        rt, vt = (rp, vp) if target_value is None and target_threshold is None else self._f1_rule(target_value, target_threshold, "target")
        p, t = self._metric_input(pred, "f1"), self._metric_input(target, "f1")
        B, H, W = p.shape
        out = torch.empty(B, dtype=torch.float64, device=self.device)
        cnt = torch.empty(B, 3, dtype=torch.int64, device=self.device) if want_counts else None
        self._check(self.lib.car_f1(self._h, C.c_void_p(p.data_ptr()), self._metric_dt(p), rp, vp, C.c_void_p(t.data_ptr()), self._metric_dt(t), rt, vt,
                                    B, H, W, C.c_void_p(cnt.data_ptr() if cnt is not None else 0), C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr())),
                    "car_f1")
        if single:
            out, cnt = out[0], (cnt[0] if cnt is not None else None)
        return (out, cnt) if want_counts else out

    def rmse(self, pred: torch.Tensor, label: torch.Tensor, scale_to_max: bool = False) -> torch.Tensor:
        """sqrt(mean((pred * s - label)^2)) per image on the GPU (car_rmse).  pred float [B,H,W] (or [H,W]), label uint8 or float of the same shape.
        s = 1, or with scale_to_max 255 / max(pred) of that image (evaluations/depth_rmse.py:59).  Returns fp64 [B]."""
        if pred.shape != label.shape:
            raise ValueError(f"rmse: pred and label differ in shape: {tuple(pred.shape)} and {tuple(label.shape)}")
        single = pred.dim() == 2
        if single:
            pred, label = pred[None], label[None]
        if pred.dim() != 3 or pred.numel() == 0:
            raise ValueError(f"rmse: expected non-empty [B,H,W] or [H,W], got {tuple(pred.shape)}")
        p, t = pred.to(device=self.device, dtype=torch.float32).contiguous(), self._metric_input(label, "rmse")
        B, H, W = p.shape
        out = torch.empty(B, dtype=torch.float64, device=self.device)
        self._check(self.lib.car_rmse(self._h, C.c_void_p(p.data_ptr()), C.c_void_p(t.data_ptr()), self._metric_dt(t), B, H, W, int(bool(scale_to_max)),
                                      C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr())), "car_rmse")
        return out[0] if single else out

    def pixels_to_u8(self, x: torch.Tensor, want_float: bool = False):
        """torchvision's save_image(normalize=True, value_range=(-1, 1)) quantiser on the GPU (car_pixels_to_u8; autoregressive/test/test_t2i.py:233-234).
        x float [B,3,H,W] in [-1,1] (values outside are clamped) -> uint8 [B,H,W,3], what canny and resize take; with want_float also fp32 [B,3,H,W]
        holding the same 0..255 values, what hed and lineart take."""
        if x.dim() != 4 or x.shape[1] != 3 or x.numel() == 0:
            raise ValueError(f"pixels_to_u8: expected a non-empty image batch [B,3,H,W], got {tuple(x.shape)}")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        B, _, H, W = x.shape
        out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=self.device)
        fl = torch.empty(B, 3, H, W, dtype=torch.float32, device=self.device) if want_float else None
        self._check(self.lib.car_pixels_to_u8(self._h, C.c_void_p(x.data_ptr()), B, H, W, C.c_void_p(out.data_ptr()),
                                              C.c_void_p(fl.data_ptr() if fl is not None else 0), C.c_void_p(_stream_ptr())), "car_pixels_to_u8")
        return (out, fl) if want_float else out

    # ------------------------------------------------------------------ reconstruction quality (tokenizer/tokenizer_image/lpips.py, reconstruction_vq_ddp.py)
    def load_lpips(self, sd: Dict[str, torch.Tensor], finalize: bool = True):
        """LPIPS().state_dict() names (tokenizer/tokenizer_image/lpips.py:53-65: net.slice1.0.weight ... lin4.model.1.weight, scaling_layer.shift / .scale
        optional), with the trunk alternatively under torchvision's features.N.weight / .bias (the LPIPS checkpoint holds the lin layers only); the C ABI
        namespaces them under 'lpips.'.  May be called once per file: finalize=False for all but the last."""
        self.load_state_dict({"lpips." + k: v for k, v in sd.items()}, finalize=finalize)

    def lpips(self, a: torch.Tensor, b: torch.Tensor, want_layers: bool = False):
        """LPIPS.forward(a, b) in inference on the GPU (car_lpips).  a, b [B,3,H,W] in [-1,1] -> fp64 [B]; with want_layers also fp64 [B,5], the per-layer
        terms whose sum in the order 0..4 it is.  Identical inputs give exactly 0; lpips(a, b) and lpips(b, a) are bit-equal."""
        if a.shape != b.shape:
            raise ValueError(f"lpips: the images differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
        if a.dim() != 4 or a.shape[1] != 3 or a.numel() == 0:
            raise ValueError(f"lpips: expected two non-empty image batches [B,3,H,W], got {tuple(a.shape)}")
        x, y = (t.to(device=self.device, dtype=torch.float32).contiguous() for t in (a, b))
        B, _, H, W = x.shape
        out = torch.empty(B, dtype=torch.float64, device=self.device)
        lay = torch.empty(B, 5, dtype=torch.float64, device=self.device) if want_layers else None
        self._check(self.lib.car_lpips(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), B, H, W, C.c_void_p(out.data_ptr()),
                                       C.c_void_p(lay.data_ptr() if lay is not None else 0), C.c_void_p(_stream_ptr())), "car_lpips")
        return (out, lay) if want_layers else out

    def psnr(self, a: torch.Tensor, b: torch.Tensor, data_range: float = 1.0, a_map=None, b_map=None) -> torch.Tensor:
        """skimage's peak_signal_noise_ratio(a, b, data_range=data_range) per image on the GPU (car_psnr): 10 log10(data_range^2 / mse), mse the fp64 mean
        over everything behind the first axis; +inf for equal images.  a, b [B,...] of one shape, each uint8 or float.  A map reads an element first, in
        fp32: 'raw' v, 'div255' v / 255, 'half' (v + 1) / 2; default 'div255' for a uint8 input (reconstruction_vq_ddp.py:149) and 'raw' for a float one.
        Returns fp64 [B]."""
        if a.shape != b.shape:
            raise ValueError(f"psnr: the inputs differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
        if a.dim() < 2 or a.numel() == 0:
            raise ValueError(f"psnr: expected non-empty [B,...], got {tuple(a.shape)}")
        codes = {"raw": L.CAR_PSNR_RAW, "div255": L.CAR_PSNR_DIV255, "half": L.CAR_PSNR_HALF}
        x, y = self._metric_input(a, "psnr"), self._metric_input(b, "psnr")
        mx = codes["div255" if x.dtype == torch.uint8 else "raw"] if a_map is None else codes[a_map]
        my = codes["div255" if y.dtype == torch.uint8 else "raw"] if b_map is None else codes[b_map]
        B = x.shape[0]
        out = torch.empty(B, dtype=torch.float64, device=self.device)
        self._check(self.lib.car_psnr(self._h, C.c_void_p(x.data_ptr()), self._metric_dt(x), mx, C.c_void_p(y.data_ptr()), self._metric_dt(y), my, B,
                                      x.numel() // B, float(data_range), C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr())), "car_psnr")
        return out

    def recon_to_u8(self, x: torch.Tensor) -> torch.Tensor:
        """torch.clamp(127.5 * x + 128.0, 0, 255).to(torch.uint8), the quantiser of reconstruction_vq_ddp.py:144 and val_ddp.py:138, bit for bit on the GPU
        (car_recon_to_u8).  x float, any shape -> uint8 of that shape.  Not save_image's rule: that one is pixels_to_u8."""
        if x.numel() == 0:
            raise ValueError(f"recon_to_u8: empty input {tuple(x.shape)}")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty(x.shape, dtype=torch.uint8, device=self.device)
        self._check(self.lib.car_recon_to_u8(self._h, C.c_void_p(x.data_ptr()), x.numel(), C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr())),
                    "car_recon_to_u8")
        return out

    # ------------------------------------------------------------------ sample quality (evaluations/c2i/evaluator.py from compute_statistics down)
    def _acts(self, x: torch.Tensor, what: str) -> torch.Tensor:
        if x.dim() != 2 or x.shape[0] == 0:
            raise ValueError(f"{what}: expected non-empty activations [N, D], got {tuple(x.shape)}")
        return x.to(device=self.device, dtype=torch.float32).contiguous()

    def fid_state(self, D: int) -> torch.Tensor:
        """An empty moment state for D features (car_fid_state_bytes): fp64 [1 + 2D + D*D] = n | c | sum(x - c) | sum (x - c)(x - c)^T."""
        nbytes = self.lib.car_fid_state_bytes(int(D))
        if nbytes <= 0:
            raise ValueError(f"fid_state: D must be in 1 .. 16384, got {D}")
        return torch.zeros(nbytes // 8, dtype=torch.float64, device=self.device)

    def fid_accumulate(self, state: torch.Tensor, acts: torch.Tensor) -> torch.Tensor:
        """Adds acts [n, D] to a moment state in place (car_fid_accumulate): fp64 on the matrix cores, fixed order, the same updates give the same bits."""
        x = self._acts(acts, "fid_accumulate")
        n, D = x.shape
        if state.dtype != torch.float64 or state.numel() != 1 + 2 * D + D * D or not state.is_contiguous() or state.device != x.device:
            raise ValueError(f"fid_accumulate: the state is not Engine.fid_state({D})")
        self._check(self.lib.car_fid_accumulate(self._h, C.c_void_p(x.data_ptr()), n, D, C.c_void_p(state.data_ptr()), C.c_void_p(_stream_ptr())),
                    "car_fid_accumulate")
        return state

    def fid_finalize(self, state: torch.Tensor, D: int):
        """(mu fp64 [D], sigma fp64 [D, D]) = np.mean(axis=0), np.cov(rowvar=False) of everything accumulated (car_fid_finalize); at least 2 rows."""
        if state.dtype != torch.float64 or state.numel() != 1 + 2 * D + D * D:
            raise ValueError(f"fid_finalize: the state is not Engine.fid_state({D})")
        mu = torch.empty(D, dtype=torch.float64, device=self.device)
        sigma = torch.empty(D, D, dtype=torch.float64, device=self.device)
        self._check(self.lib.car_fid_finalize(self._h, C.c_void_p(state.data_ptr()), D, C.c_void_p(mu.data_ptr()), C.c_void_p(sigma.data_ptr()),
                                              C.c_void_p(_stream_ptr())), "car_fid_finalize")
        return mu, sigma

    def manifold_radii(self, feats: torch.Tensor, k: int = 3, row_batch: int = 10000, col_batch: int = 10000) -> torch.Tensor:
        """ManifoldEstimator.manifold_radii with nhood_sizes = (k,) (car_manifold_radii): fp32 [N], per row the (k+1)-th smallest squared distance to the
        set, its own included.  fp16 distances with the script's per-block fp32 fallback; the N x N matrix is never written."""
        x = self._acts(feats, "manifold_radii")
        N, D = x.shape
        out = torch.empty(N, dtype=torch.float32, device=self.device)
        self._check(self.lib.car_manifold_radii(self._h, C.c_void_p(x.data_ptr()), N, D, int(k), int(row_batch), int(col_batch), C.c_void_p(out.data_ptr()),
                                                C.c_void_p(_stream_ptr())), "car_manifold_radii")
        return out

    def manifold_pr(self, f1: torch.Tensor, r1: torch.Tensor, f2: torch.Tensor, r2: torch.Tensor, row_batch: int = 10000, col_batch: int = 10000):
        """ManifoldEstimator.evaluate_pr (car_manifold_pr): (status1 uint8 [N1], status2 uint8 [N2], pr fp64 [2]); status1[i] = any_j d_ij <= r2[j],
        status2[j] = any_i d_ij <= r1[i], pr = (mean status2, mean status1) = (precision, recall) with set 1 the reference batch."""
        a, b = self._acts(f1, "manifold_pr"), self._acts(f2, "manifold_pr")
        if a.shape[1] != b.shape[1]:
            raise ValueError(f"manifold_pr: the sets differ in D: {tuple(a.shape)} and {tuple(b.shape)}")
        ra, rb = (r.to(device=self.device, dtype=torch.float32).contiguous().reshape(-1) for r in (r1, r2))
        if ra.numel() != a.shape[0] or rb.numel() != b.shape[0]:
            raise ValueError(f"manifold_pr: one radius per row, got {ra.numel()} for {a.shape[0]} rows and {rb.numel()} for {b.shape[0]}")
        s1 = torch.empty(a.shape[0], dtype=torch.uint8, device=self.device)
        s2 = torch.empty(b.shape[0], dtype=torch.uint8, device=self.device)
        pr = torch.empty(2, dtype=torch.float64, device=self.device)
        self._check(self.lib.car_manifold_pr(self._h, C.c_void_p(a.data_ptr()), C.c_void_p(ra.data_ptr()), a.shape[0], C.c_void_p(b.data_ptr()),
                                             C.c_void_p(rb.data_ptr()), b.shape[0], a.shape[1], int(row_batch), int(col_batch), C.c_void_p(s1.data_ptr()),
                                             C.c_void_p(s2.data_ptr()), C.c_void_p(pr.data_ptr()), C.c_void_p(_stream_ptr())), "car_manifold_pr")
        return s1, s2, pr

    def debug_pairwise_distances(self, U: torch.Tensor, V: torch.Tensor):
        """One block of DistanceBlock.pairwise_distances (car_debug_pairwise_distances, tests): (fp32 [n, m], used_fp32 int32 [1])."""
        a, b = self._acts(U, "debug_pairwise_distances"), self._acts(V, "debug_pairwise_distances")
        if a.shape[1] != b.shape[1]:
            raise ValueError(f"debug_pairwise_distances: the sets differ in D: {tuple(a.shape)} and {tuple(b.shape)}")
        out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=self.device)
        used = torch.empty(1, dtype=torch.int32, device=self.device)
        self._check(self.lib.car_debug_pairwise_distances(self._h, C.c_void_p(a.data_ptr()), a.shape[0], C.c_void_p(b.data_ptr()), b.shape[0], a.shape[1],
                                                          C.c_void_p(out.data_ptr()), C.c_void_p(used.data_ptr()), C.c_void_p(_stream_ptr())),
                    "car_debug_pairwise_distances")
        return out, used

    def inception_score(self, acts: torch.Tensor, w: torch.Tensor, split_size: int = 5000) -> torch.Tensor:
        """compute_inception_score (car_inception_score): p = softmax(acts @ w) in fp32, the rest fp64.  acts [N, D], w [D, C] ->
        fp64 [1 + ceil(N / split_size)]: the score, then every split's value."""
        x = self._acts(acts, "inception_score")
        N, D = x.shape
        if w.dim() != 2 or w.shape[0] != D or w.shape[1] == 0:
            raise ValueError(f"inception_score: expected a softmax weight [{D}, C], got {tuple(w.shape)}")
        wm = w.to(device=self.device, dtype=torch.float32).contiguous()
        if int(split_size) < 1:
            raise ValueError(f"inception_score: split_size must be positive, got {split_size}")
        out = torch.empty(1 + -(-N // min(int(split_size), N)), dtype=torch.float64, device=self.device)
        self._check(self.lib.car_inception_score(self._h, C.c_void_p(x.data_ptr()), N, D, C.c_void_p(wm.data_ptr()), wm.shape[1], int(split_size),
                                                 C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr())), "car_inception_score")
        return out

    def load_lineart(self, sd: Dict[str, torch.Tensor], finalize: bool = True):
        """LineArt().state_dict() names (condition/lineart.py:26-72: model0.1.weight ... model4.1.bias); the C ABI namespaces them under 'lineart.'."""
        self.load_state_dict({"lineart." + k: v for k, v in sd.items()}, finalize=finalize)

    @staticmethod
    def lineart_output_size(H: int, W: int):
        """The network's own output size: two stride-2 convs (floor((n-1)/2)+1 each) followed by two 2x transposed convs."""
        down = lambda n: ((n - 1) // 2 + 1 - 1) // 2 + 1
        return 4 * down(H), 4 * down(W)

    def lineart(self, img: torch.Tensor, want_control: bool = False):
        """LineArt.forward (condition/lineart.py:74-86) on the GPU.  img [B,3,H,W], raw 0..255 values -> fp32 [B,1,Ho,Wo] in (0,1); with want_control
        also the control tensor [B,3,Ho,Wo] = 1 - 2*out in the context's element type (sample_t2i.py:131-132,141)."""
        assert img.dim() == 4 and img.shape[1] == 3, "expected an image batch [B, 3, H, W]"
        x = img.to(device=self.device, dtype=torch.float32).contiguous()
        B, _, H, W = x.shape
        Ho, Wo = self.lineart_output_size(H, W)
        out = torch.empty(B, 1, max(Ho, 0), max(Wo, 0), dtype=torch.float32, device=self.device)
        ctrl = torch.empty(B, 3, max(Ho, 0), max(Wo, 0), dtype=self.dtype, device=self.device) if want_control else None
        self._check(self.lib.car_lineart(self._h, C.c_void_p(x.data_ptr()), B, H, W, C.c_void_p(out.data_ptr()),
                                         C.c_void_p(ctrl.data_ptr() if ctrl is not None else 0), C.c_void_p(_stream_ptr())), "car_lineart")
        return (out, ctrl) if want_control else out

    def load_hed(self, sd: Dict[str, torch.Tensor], finalize: bool = True):
        """ControlNetHED_Apache2().state_dict() names (condition/hed.py:36-44: norm, block1.convs.0.weight ... block5.projection.bias), or a
        HEDdetector's own with the 'netNetwork.' prefix; the C ABI namespaces them under 'hed.'."""
        pre = "netNetwork."
        self.load_state_dict({"hed." + (k[len(pre):] if k.startswith(pre) else k): v for k, v in sd.items()}, finalize=finalize)

    def hed(self, img: torch.Tensor, want_control: bool = False):
        """HEDdetector.__call__ (condition/hed.py:67-81) on the GPU.  img [B,3,H,W] uint8 or float, raw 0..255 values -> fp32 [B,H,W] in 0..255; with
        want_control also the control tensor [B,3,H,W] = 2*(out/255 - 0.5) in the context's element type (sample_t2i.py:128,141)."""
        assert img.dim() == 4 and img.shape[1] == 3, "expected an image batch [B, 3, H, W]"
        x = img.to(device=self.device, dtype=torch.float32).contiguous()
        B, _, H, W = x.shape
        out = torch.empty(B, H, W, dtype=torch.float32, device=self.device)
        ctrl = torch.empty(B, 3, H, W, dtype=self.dtype, device=self.device) if want_control else None
        self._check(self.lib.car_hed(self._h, C.c_void_p(x.data_ptr()), B, H, W, C.c_void_p(out.data_ptr()),
                                     C.c_void_p(ctrl.data_ptr() if ctrl is not None else 0), C.c_void_p(_stream_ptr())), "car_hed")
        return (out, ctrl) if want_control else out

    def depth_configure(self, dcfg):
        """car_depth_configure from a config.DPTConfig.  A config outside the shipped family (hybrid, readout other than 'project', batch norm in the
        fusion residual units, ...) is refused here, before any tensor is loaded."""
        bad = dcfg.family_errors()
        if bad:
            raise ValueError("DPT config outside the supported family: " + "; ".join(bad))
        dc = L.CarDptConfig()
        dc.hidden, dc.layers, dc.heads, dc.mlp = dcfg.hidden_size, dcfg.num_hidden_layers, dcfg.num_attention_heads, dcfg.intermediate_size
        dc.pos_grid, dc.fusion_hidden, dc.ln_eps = dcfg.pos_grid, dcfg.fusion_hidden_size, dcfg.layer_norm_eps
        for i in range(4):
            dc.out_indices[i], dc.neck_hidden[i] = dcfg.backbone_out_indices[i], dcfg.neck_hidden_sizes[i]
        self._check(self.lib.car_depth_configure(self._h, C.byref(dc)), "car_depth_configure")
        self.dptcfg = dcfg

    def load_depth(self, sd: Dict[str, torch.Tensor], cfg, finalize: bool = True):
        """DPTForDepthEstimation.state_dict() names (dpt.embeddings.cls_token ... head.head.4.bias); the C ABI namespaces them under 'depth.'."""
        self.depth_configure(cfg)
        self.load_state_dict({"depth." + k: v for k, v in sd.items()}, finalize=finalize)

    def depth(self, pixel_values: torch.Tensor, want_control: bool = False):
        """DPTForDepthEstimation(pixel_values).predicted_depth on the GPU.  pixel_values [B,3,S,S] float, what the HF image processor hands the model
        (rescaled and normalised); S a multiple of 32 -> fp32 [B,S,S] >= 0; with want_control also the control tensor [B,3,S,S] = 2*(d/max - 0.5), the
        maximum taken per image, in the context's element type (sample_t2i.py:133-141)."""
        assert pixel_values.dim() == 4 and pixel_values.shape[1] == 3, "expected pixel_values [B, 3, H, W]"
        x = pixel_values.to(device=self.device, dtype=torch.float32).contiguous()
        B, _, H, W = x.shape
        out = torch.empty(B, H, W, dtype=torch.float32, device=self.device)
        ctrl = torch.empty(B, 3, H, W, dtype=self.dtype, device=self.device) if want_control else None
        self._check(self.lib.car_depth(self._h, C.c_void_p(x.data_ptr()), B, H, W, C.c_void_p(out.data_ptr()),
                                       C.c_void_p(ctrl.data_ptr() if ctrl is not None else 0), C.c_void_p(_stream_ptr())), "car_depth")
        return (out, ctrl) if want_control else out

    # ------------------------------------------------------------------ caption encoder (language/t5.py)
    def t5_configure(self, t5cfg):
        tc = L.CarT5Config()
        tc.vocab_size, tc.d_model, tc.d_kv, tc.num_heads = t5cfg.vocab_size, t5cfg.d_model, t5cfg.d_kv, t5cfg.num_heads
        tc.d_ff, tc.num_layers = t5cfg.d_ff, t5cfg.num_layers
        tc.rel_buckets, tc.rel_max_distance = t5cfg.relative_attention_num_buckets, t5cfg.relative_attention_max_distance
        tc.ln_eps = t5cfg.layer_norm_epsilon
        self._check(self.lib.car_t5_configure(self._h, C.byref(tc)), "car_t5_configure")
        self.t5cfg = t5cfg

    def load_t5_state_dict(self, sd: Dict[str, torch.Tensor], finalize: bool = True):
        """HF T5EncoderModel / T5ForConditionalGeneration state-dict names; the C ABI namespaces them under 't5.'."""
        self.load_state_dict({"t5." + k: v for k, v in sd.items()}, finalize=finalize)

    def t5_encode(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """T5EncoderModel(input_ids, attention_mask)['last_hidden_state'] (language/t5.py:194-199) -> [B,T,d_model] in self.dtype."""
        assert input_ids.dim() == 2
        ids = input_ids.to(device=self.device, dtype=torch.int64).contiguous()
        mk = None if attention_mask is None else attention_mask.to(device=self.device, dtype=torch.int64).contiguous()
        B, T = ids.shape
        out = torch.empty(B, T, self.t5cfg.d_model, dtype=self.dtype, device=self.device)
        self._check(self.lib.car_t5_encode(self._h, C.c_void_p(ids.data_ptr()), C.c_void_p(mk.data_ptr() if mk is not None else 0), B, T,
                                           C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr())), "car_t5_encode")
        return out

    # ------------------------------------------------------------------ CLIP score (evaluations/t2i/evaluation.py:129-176)
    def clip_configure(self, ccfg):
        """car_clip_configure from a config.CLIPConfig."""
        cc = L.CarClipConfig()
        cc.vision_width, cc.vision_layers, cc.vision_heads, cc.vision_mlp = ccfg.vision_width, ccfg.vision_layers, ccfg.vision_heads, ccfg.vision_mlp
        cc.image_size, cc.patch = ccfg.image_size, ccfg.patch
        cc.text_width, cc.text_layers, cc.text_heads, cc.text_mlp = ccfg.text_width, ccfg.text_layers, ccfg.text_heads, ccfg.text_mlp
        cc.vocab_size, cc.context_length, cc.proj_dim, cc.ln_eps = ccfg.vocab_size, ccfg.context_length, ccfg.proj_dim, ccfg.ln_eps
        self._check(self.lib.car_clip_configure(self._h, C.byref(cc)), "car_clip_configure")
        self.clipcfg = ccfg

    def load_clip_state_dict(self, sd: Dict[str, torch.Tensor], finalize: bool = True):
        """HF CLIPModel state-dict names; the C ABI namespaces them under 'clip.'."""
        self.load_state_dict({"clip." + k: v for k, v in sd.items()}, finalize=finalize)

    def _clip_proj(self) -> int:
        ccfg = getattr(self, "clipcfg", None)
        return ccfg.proj_dim if ccfg is not None else 1          # not configured: the library refuses the call and says why

    def clip_encode_image(self, img: torch.Tensor, requant: bool = False, want_pixel_values: bool = False, want_embedding: bool = True):
        """CLIP's preprocessor and image tower on the GPU (car_clip_encode_image).  img uint8 [B,H,W,3] (or [H,W,3]); requant: the evaluation script's
        ToTensor / Normalize(0.5) / tensor2pil round trip first.  Returns fp32 [B,proj_dim]; with want_pixel_values also fp32 [B,3,n_px,n_px]."""
        if img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[-1] != 3 or img.numel() == 0:
            raise ValueError(f"clip_encode_image: expected a non-empty uint8 image [B,H,W,3] or [H,W,3], got {img.dtype} {tuple(img.shape)}")
        x = (img[None] if img.dim() == 3 else img).to(self.device).contiguous()
        B, H, W, _ = x.shape
        n = self.clipcfg.image_size if getattr(self, "clipcfg", None) is not None else 1
        emb = torch.empty(B, self._clip_proj(), dtype=torch.float32, device=self.device) if want_embedding else None
        pv = torch.empty(B, 3, n, n, dtype=torch.float32, device=self.device) if want_pixel_values else None
        self._check(self.lib.car_clip_encode_image(self._h, C.c_void_p(x.data_ptr()), B, H, W, int(bool(requant)),
                                                   C.c_void_p(emb.data_ptr() if emb is not None else 0), C.c_void_p(pv.data_ptr() if pv is not None else 0),
                                                   C.c_void_p(_stream_ptr())), "car_clip_encode_image")
        out = tuple(t for t in (emb, pv) if t is not None)
        return out[0] if len(out) == 1 else out

    def clip_encode_text(self, ids: torch.Tensor) -> torch.Tensor:
        """CLIP's text tower on the GPU (car_clip_encode_text).  ids integer [B,T], T <= context_length -> fp32 [B,proj_dim].  An id outside [0, vocab) on
        a host tensor raises here; on a device tensor it raises the sticky flag (check_errors)."""
        if not torch.is_tensor(ids) or ids.dim() != 2 or ids.dtype.is_floating_point or ids.numel() == 0:
            raise ValueError(f"clip_encode_text: expected non-empty integer ids [B,T], got {tuple(getattr(ids, 'shape', ()))}")
        proj = self._clip_proj()
        if ids.device.type == "cpu" and getattr(self, "clipcfg", None) is not None:
            lo, hi = int(ids.min()), int(ids.max())
            if lo < 0 or hi >= self.clipcfg.vocab_size:
                raise RuntimeError(f"car_clip_encode_text: token id out of range [0,{self.clipcfg.vocab_size}) (got {lo}..{hi})")
        x = ids.to(device=self.device, dtype=torch.int64).contiguous()
        B, T = x.shape
        emb = torch.empty(B, proj, dtype=torch.float32, device=self.device)
        self._check(self.lib.car_clip_encode_text(self._h, C.c_void_p(x.data_ptr()), B, T, C.c_void_p(emb.data_ptr()), C.c_void_p(_stream_ptr())),
                    "car_clip_encode_text")
        return emb

    def clip_score(self, img_emb: torch.Tensor, txt_emb: torch.Tensor, n_mean: Optional[int] = None):
        """F.cosine_similarity(img_emb, txt_emb, dim=1) on the GPU (car_clip_score): fp32 [B]; with n_mean also the fp64 mean of the first n_mean values
        as a 0-dim device tensor."""
        proj = self._clip_proj()
        a = img_emb.to(device=self.device, dtype=torch.float32).contiguous()
        b = txt_emb.to(device=self.device, dtype=torch.float32).contiguous()
        if a.dim() != 2 or a.shape != b.shape or a.shape[1] != proj or a.shape[0] == 0:
            raise ValueError(f"clip_score: expected two [B,{proj}] tensors, got {tuple(a.shape)} and {tuple(b.shape)}")
        B = a.shape[0]
        out = torch.empty(B, dtype=torch.float32, device=self.device)
        mean = torch.empty(1, dtype=torch.float64, device=self.device) if n_mean is not None else None
        self._check(self.lib.car_clip_score(self._h, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), B, int(n_mean or 0), C.c_void_p(out.data_ptr()),
                                            C.c_void_p(mean.data_ptr() if mean is not None else 0), C.c_void_p(_stream_ptr())), "car_clip_score")
        return (out, mean[0]) if mean is not None else out

    def check_errors(self):
        """Waits for the work enqueued on this context and raises if device code reported an error no entry could fail on synchronously
        (today: a c2i class label outside [0, num_classes] in a device-resident label tensor — include/controlar_hip.h, car_generate_c2i)."""
        self._check(self.lib.car_check_errors(self._h), "car_check_errors")

    def stats(self) -> dict:
        s = L.CarStats()
        self._check(self.lib.car_get_stats(self._h, C.byref(s)), "car_get_stats")
        self._check(self.lib.car_check_errors(self._h), "car_check_errors")          # car_get_stats waited for the stream: a sticky device error is visible now
        return dict(decode_ms=s.decode_ms, prefill_ms=s.prefill_ms, decode_steps=s.decode_steps,
                    decode_algo_bytes=s.decode_algo_bytes, decode_kernels_per_step=s.decode_kernels_per_step,
                    graph_used=bool(s.graph_used), dev_knobs_active=int(s.dev_knobs_active))

    def control_tokens(self, k: int, b: int, n_tok: int) -> torch.Tensor:
        n = b * n_tok * self.cfg.gpt.dim
        buf = torch.empty(n, dtype=torch.float32)
        self._check(self.lib.car_debug_control_tokens(self._h, k, C.c_void_p(buf.data_ptr()), n), "car_debug_control_tokens")
        return buf.view(b, n_tok, self.cfg.gpt.dim)
