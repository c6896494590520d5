"""CPU: the host side of the split-bf16 VQ decoder (car_config.vq_split_bf16) — the operand split itself against torch's bf16 rounding,
the refusals of car_create, and the place of the new field in car_config."""
import ctypes as C

import numpy as np
import torch

from controlar_amd import _lib as L


def _split(x: torch.Tensor):
    lib = L.load()
    x = x.float().contiguous()
    hi = np.empty(x.numel(), dtype=np.uint16)
    lo = np.empty(x.numel(), dtype=np.uint16)
    assert lib.car_debug_split_bf16(C.c_void_p(x.data_ptr()), x.numel(), C.c_void_p(hi.ctypes.data), C.c_void_p(lo.ctypes.data)) == 0
    return torch.from_numpy(hi.astype(np.int16)), torch.from_numpy(lo.astype(np.int16))


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).view(torch.int16)


def test_split_matches_torch_bf16_rounding():
    """hi = RNE bf16 of x and lo = RNE bf16 of x - float(hi), bit for bit as torch rounds; lo = 0 where hi is not finite; hi + lo == x for finite values
    of at most 16 significant bits.  About 50 000 values: normal numbers at several scales, +-0, subnormal fp32, the neighbourhood of every kind of
    rounding tie, +-FLT_MAX (rounds to inf), +-inf and NaN."""
    g = torch.Generator().manual_seed(0)
    flt_max = torch.finfo(torch.float32).max
    parts = [torch.randn(12000, generator=g), torch.randn(8000, generator=g) * 1e-3, torch.randn(8000, generator=g) * 3e4,
             torch.randn(4000, generator=g) * 1e30, torch.randn(4000, generator=g) * 1e-30]
    # subnormal fp32 (and the smallest normals): raw bit patterns below and around 2^-126
    sub = torch.randint(1, 1 << 24, (6000,), generator=g, dtype=torch.int32)
    sub = torch.where(torch.arange(6000) % 2 == 0, sub, sub | torch.tensor(-2 ** 31, dtype=torch.int32))
    parts.append(sub.view(torch.float32))
    # within one bf16 ulp of a rounding tie: a bf16 number (random sign / exponent / mantissa, finite) plus half an ulp plus -2 .. +2 fp32 ulps, odd and even mantissas alike
    base = torch.randint(0, 1 << 15, (900,), generator=g, dtype=torch.int32)
    base = base[((base >> 7) & 0xff) < 0xfe]
    tie = (base << 16) | 0x8000
    near = torch.cat([tie + d for d in (-2, -1, 0, 1, 2)])
    near = torch.cat([near, near | torch.tensor(-2 ** 31, dtype=torch.int32)])
    parts.append(near.view(torch.float32))
    parts.append(torch.tensor([0.0, -0.0, flt_max, -flt_max, float("inf"), float("-inf"), float("nan"), 1.0, -1.0, 2.0 ** -126, 2.0 ** -149, -2.0 ** -149,
                               3.3895313892515355e38, 3.3961775292304601e38]))     # the largest finite bf16, and the tie between it and inf
    x = torch.cat(parts).float()
    assert 45000 <= x.numel() <= 60000
    hi, lo = _split(x)
    want_hi = _bits(x)
    num = ~torch.isnan(x)            # torch's own bits for a NaN depend on the code path (0x7fc0 scalar, 0xffff vectorised): a NaN has to stay a NaN, checked below
    assert torch.equal(hi[num], want_hi[num]), int((hi[num] != want_hi[num]).sum())
    hf = hi.view(torch.bfloat16).float()
    fin = torch.isfinite(hf)
    assert not bool(fin.all()) and bool(fin[:1000].all())
    want_lo = _bits(x - hf)
    assert torch.equal(lo[fin], want_lo[fin]), int((lo[fin] != want_lo[fin]).sum())
    assert bool((lo[~fin] == 0).all())
    # an inf or a NaN stays what it is
    assert bool(torch.isnan(hf[torch.isnan(x)]).all()) and torch.equal(hf[torch.isinf(x)], x[torch.isinf(x)])
    # at most 16 significant bits: the two halves ARE the value
    ints = torch.randint(-65535, 65536, (5000,), generator=g).float()
    scaled = torch.cat([ints, ints * 2.0 ** -20, ints * 2.0 ** 40, ints * 2.0 ** -100])
    h16, l16 = _split(scaled)
    assert torch.equal(h16.view(torch.bfloat16).float() + l16.view(torch.bfloat16).float(), scaled)
    assert bool((l16.view(torch.bfloat16).float() != 0).any())


def _config(mode):
    """car_config as Engine.__init__ fills it for tiny_t2i() (no GPU needed up to car_create's validation)"""
    from controlar_amd import config as Cfg
    cfg = Cfg.tiny_t2i()
    g, v, q = cfg.gpt, cfg.vit, cfg.vq
    cc = L.CarConfig()
    cc.abi_version, cc.mode = L.CAR_ABI_VERSION, mode
    cc.dim, cc.n_layer, cc.n_head, cc.ffn_hidden, cc.vocab_size = g.dim, g.n_layer, g.n_head, g.ffn_hidden, g.vocab_size
    cc.cls_token_num, cc.block_size, cc.caption_dim = g.cls_token_num, g.block_size, g.caption_dim
    cc.norm_eps, cc.rope_base = g.norm_eps, g.rope_base
    cc.vit_hidden, cc.vit_layers, cc.vit_heads, cc.vit_mlp = v.hidden, v.layers, v.heads, v.mlp
    cc.vit_patch, cc.vit_pos_grid, cc.vit_ln_eps = v.patch, v.pos_grid, v.ln_eps
    cc.resize_mode = L.CAR_RESIZE_NEAREST
    cc.num_classes = g.num_classes
    cc.codebook_size, cc.codebook_dim, cc.z_channels, cc.vq_ch = q.codebook_size, q.codebook_embed_dim, q.z_channels, q.ch
    cc.vq_num_res_blocks, cc.vq_n_mult, cc.gn_eps = q.num_res_blocks, len(q.ch_mult), q.gn_eps
    for i, m in enumerate(q.ch_mult):
        cc.vq_ch_mult[i] = m
    return cc


def test_create_refuses_the_option_outside_fp32_and_values_other_than_0_and_1():
    lib = L.load()
    for mode, val in ((L.CAR_BF16, 1), (L.CAR_F32, 2), (L.CAR_F32, -1)):
        cc = _config(mode)
        cc.vq_split_bf16 = val
        h = C.c_void_p()
        assert lib.car_create(C.byref(h), C.byref(cc)) != 0, (mode, val)
        assert h.value is None
        assert b"vq_split_bf16" in lib.car_last_error(None), lib.car_last_error(None)


def test_field_takes_the_first_reserved_word():
    assert C.sizeof(L.CarConfig) == 172
    names = [f[0] for f in L.CarConfig._fields_]
    assert names[-3:] == ["kv_cache_fp8", "vq_split_bf16", "reserved"]
    assert L.CarConfig.vq_split_bf16.offset == 164 and L.CarConfig.vq_split_bf16.size == 4       # where reserved[0] was
    assert L.CarConfig.reserved.offset == 168 and L.CarConfig.reserved.size == 4
    assert L.CarConfig.kv_cache_fp8.offset == 160
    assert "car_debug_split_bf16" in L.SYMBOLS
