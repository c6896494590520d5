"""GPU tests of car_score (pytest -m gpu): per-token nll of given image tokens in one parallel pass, against the reference's teacher-forced logits in
tests/golden (fp64 log-softmax: tests/score_ref.py), against its own logits, against the token loop, and the fused projection + cross-entropy kernel
alone against torch fp64 on the host.

Bounds.  Logits: the ones the project holds teacher-forced logits to against the same fixtures (test_parity_gpu.py): fp32 atol 5e-4 / rtol 1e-4, bf16
max <= 0.6 k and mean <= 0.08 k with k = 1 or sqrt(s^2 + (s-1)^2) under CFG scale s.  nll against the reference: log-sum-exp and the gather are each
1-Lipschitz in the max norm, so twice the logits bound (maximum; and the mean in bf16).  nll against the fp64 loss of the call's OWN logits: the fp32
exp / sum / log alone, worst case (V + 64) 2^-24 + 2^-22 |nll| (score_ref.fused_bound)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests.cases import CASES, GOLDEN, load_case
from tests.score_ref import fused_bound, nll_ref

pytestmark = pytest.mark.gpu
PRECS = ("fp32", "bf16")
F32_ATOL, F32_RTOL = 5e-4, 1e-4


def _mask(cs):
    return cs["mask"].cuda() if cs["mask"] is not None else None


def _engine(cs, prec):
    from controlar_amd.engine import Engine
    eng = Engine(cs["cfg"], prec)
    eng.load_state_dict(cs["gsd"]); eng.finalize()
    return eng


def _kw(cs, **over):
    kw = dict(emb_masks=_mask(cs), cfg_scale=cs["cfg_scale"], cfg_interval=cs["cfg_interval"], control_strength=cs["control_strength"])
    kw.update(over)
    return kw


def _k(s):
    return 1.0 if s <= 1 else float(np.sqrt(s ** 2 + (s - 1) ** 2))


def _random_tokens(cs, seed=11):
    V = cs["cfg"].gpt.vocab_size
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, V, (cs["B"], cs["n_new"]), generator=g, dtype=torch.int32)
    t[:, 0] = 0; t[:, 1] = V - 1; t[0, -1] = V - 1; t[-1, -1] = 0
    return t


def _check_own_logits(nll, logits, tokens, V):
    """item 3: the fused loss equals the fp64 loss of the very logits the call returned"""
    own = nll_ref(logits, tokens)
    d = np.abs(nll.astype(np.float64) - own)
    bound = fused_bound(own, V)
    assert (d <= bound).all(), (float(d.max()), float(bound[np.unravel_index(d.argmax(), d.shape)]))
    return float(d.max())


# ------------------------------------------------------------------ 1 + 3: against the reference, every case, both modes
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", list(CASES))
def test_score_against_reference(name, prec):
    cs = load_case(name); gold = cs["gold"]; V = cs["cfg"].gpt.vocab_size
    eng = _engine(cs, prec)
    eng.encode_control(cs["img"].cuda())
    tokens = torch.from_numpy(gold["tokens"])
    nll, logits = eng.score(cs["emb"].cuda(), tokens.cuda(), return_logits=True, **_kw(cs))
    nll, logits = nll.cpu().numpy(), logits.cpu().numpy()
    eng.close()
    want = nll_ref(gold["logits"], gold["tokens"])
    d = np.abs(logits - gold["logits"]); dn = np.abs(nll - want)
    own = _check_own_logits(nll, logits, gold["tokens"], V)
    print("SCORE_PARITY " + json.dumps(dict(case=name, prec=prec, logits_max=float(d.max()), logits_mean=float(d.mean()), nll_max=float(dn.max()),
                                            nll_mean=float(dn.mean()), nll_vs_own_logits_max=own)))
    assert tuple(nll.shape) == (cs["B"], cs["n_new"]) and np.isfinite(nll).all()
    if prec == "fp32":
        np.testing.assert_allclose(logits, gold["logits"], atol=F32_ATOL, rtol=F32_RTOL)
        eps = F32_ATOL + F32_RTOL * np.abs(gold["logits"]).max(axis=-1)
        assert (dn <= 2 * eps).all(), float((dn - 2 * eps).max())
    else:
        k = _k(cs["cfg_scale"])
        assert d.max() <= 0.6 * k and d.mean() <= 0.08 * k, (d.max(), d.mean(), k)
        assert dn.max() <= 2 * 0.6 * k and dn.mean() <= 2 * 0.08 * k, (dn.max(), dn.mean(), k)


# ------------------------------------------------------------------ 2 + 3: GPT-B, 256 tokens, cfg 4
@pytest.mark.parametrize("prec", PRECS)
def test_score_gpt_b_256_cfg4(prec):
    from controlar_amd import config as Cfg, synth
    from controlar_amd.engine import Engine
    gold = dict(np.load(os.path.join(GOLDEN, "b_canny_256_cfg4.npz")))
    B, H, W, seed, _ = [int(x) for x in gold["meta"]]
    cfg = Cfg.b_t2i(256, "small", "canny")
    gsd, _ = synth.path_state_dicts(cfg, seed=seed)
    img = synth.canny_like_control(B, H, W)
    emb, mask = synth.text_embeddings(B, cfg.gpt.cls_token_num, cfg.gpt.caption_dim)
    eng = Engine(cfg, prec); eng.load_state_dict(gsd); eng.finalize()
    eng.encode_control(img.cuda())
    s = float(gold["cfg_scale"])
    nll, logits = eng.score(emb.cuda(), torch.from_numpy(gold["tokens"]).cuda(), mask.cuda(), cfg_scale=s, return_logits=True)
    nll, logits = nll.cpu().numpy(), logits.cpu().numpy()
    eng.close()
    got = logits[:, gold["logits_steps"]][:, :, ::4]
    d = np.abs(got - gold["logits"])
    own = _check_own_logits(nll, logits, gold["tokens"], cfg.gpt.vocab_size)
    print("SCORE_PARITY " + json.dumps(dict(case="b_canny_256_cfg4", prec=prec, logits_max=float(d.max()), logits_mean=float(d.mean()), nll_vs_own_logits_max=own)))
    if prec == "fp32":
        np.testing.assert_allclose(got, gold["logits"], atol=2e-3, rtol=1e-4)          # test_parity_gpu.py:325
    else:
        assert d.max() <= 0.6 * _k(s) and d.mean() <= 0.08 * _k(s), (d.max(), d.mean())


# ------------------------------------------------------------------ 4: against the token loop, arbitrary tokens
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["tiny_depth_cfg4", "tiny_mask_edges"])
def test_score_against_token_loop(name, prec):
    cs = load_case(name); V = cs["cfg"].gpt.vocab_size
    tokens = _random_tokens(cs)
    eng = _engine(cs, prec)
    eng.encode_control(cs["img"].cuda())
    _, lg_loop = eng.generate(cs["emb"].cuda(), cs["n_new"], forced_tokens=tokens, return_logits=True, **_kw(cs))
    nll, lg = eng.score(cs["emb"].cuda(), tokens.cuda(), return_logits=True, **_kw(cs))
    lg_loop, lg, nll = lg_loop.cpu().numpy(), lg.cpu().numpy(), nll.cpu().numpy()
    eng.close()
    d = np.abs(lg - lg_loop); dn = np.abs(nll - nll_ref(lg_loop, tokens.numpy()))
    print("SCORE_VS_LOOP " + json.dumps(dict(case=name, prec=prec, logits_max=float(d.max()), logits_mean=float(d.mean()), nll_max=float(dn.max()), nll_mean=float(dn.mean()))))
    _check_own_logits(nll, lg, tokens.numpy(), V)
    if prec == "fp32":
        np.testing.assert_allclose(lg, lg_loop, atol=F32_ATOL, rtol=F32_RTOL)
        assert (dn <= 2 * (F32_ATOL + F32_RTOL * np.abs(lg_loop).max(axis=-1))).all(), float(dn.max())
    else:
        k = _k(cs["cfg_scale"])
        assert d.max() <= 0.6 * k and d.mean() <= 0.08 * k, (d.max(), d.mean(), k)
        assert dn.max() <= 2 * 0.6 * k and dn.mean() <= 2 * 0.08 * k, (dn.max(), dn.mean(), k)


# ------------------------------------------------------------------ 5: invariances, bit for bit
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["tiny_depth_cfg4", "tiny_mask_edges"])
def test_score_invariances_bit_for_bit(name, prec):
    cs = load_case(name); V = cs["cfg"].gpt.vocab_size; B, N = cs["B"], cs["n_new"]
    tokens = _random_tokens(cs, seed=5).cuda()
    emb, img = cs["emb"].cuda(), cs["img"].cuda()
    eng = _engine(cs, prec)
    eng.encode_control(img)
    toks_before = eng.generate(emb, N, **_kw(cs)).cpu()
    algo_bytes = eng.stats()["decode_algo_bytes"]
    nll, lg = eng.score(emb, tokens, return_logits=True, **_kw(cs))
    assert eng.stats()["decode_algo_bytes"] == algo_bytes                      # the token loop's device scalars (read lazily by car_get_stats) are not the pass's scratch
    nll2 = eng.score(emb, tokens, **_kw(cs))                                  # a second call; without logits_out
    assert torch.equal(nll, nll2)
    nll3, lg3 = eng.score(emb, tokens, return_logits=True, **_kw(cs))
    assert torch.equal(nll, nll3) and torch.equal(lg, lg3)
    toks_after = eng.generate(emb, N, **_kw(cs)).cpu()                        # car_generate is untouched by a car_score on the same context
    assert torch.equal(toks_before, toks_after)
    # causality: positions before i do not see tokens[:, i:]
    eng.encode_control(img)
    i = N // 2
    t2 = tokens.clone(); t2[:, i:] = (t2[:, i:] + 17) % V
    nll_c = eng.score(emb, t2, **_kw(cs))
    assert torch.equal(nll_c[:, :i], nll[:, :i]) and not torch.equal(nll_c[:, i:], nll[:, i:])
    # each image alone equals its slice of the batch (its own prompt length decides the window when it is alone)
    for j in range(B):
        eng.encode_control(img[j:j + 1])
        kw = _kw(cs)
        if kw["emb_masks"] is not None:
            kw["emb_masks"] = kw["emb_masks"][j:j + 1]
        n1, l1 = eng.score(emb[j:j + 1], tokens[j:j + 1], return_logits=True, **kw)
        assert torch.equal(n1[0], nll[j]) and torch.equal(l1[0], lg[j]), (name, prec, j, float((n1[0] - nll[j]).abs().max()))
    eng.close()


@pytest.mark.parametrize("prec", PRECS)
def test_score_chunked_batch_equals_single_images(prec):
    """128 images under cfg 4 are more than the 16384 rows of one chunk (engine_score.hip's chunk rule: 2 chunks of 64 images or 3 of 43, by the window
    the prompts leave).  Images on both sides of either boundary return the bits they return alone."""
    from controlar_amd.engine import first_valid_position
    cs = load_case("tiny_depth_cfg4"); V = cs["cfg"].gpt.vocab_size; N = cs["n_new"]; B = 128; T = cs["cfg"].gpt.cls_token_num
    Ts = T - min(first_valid_position(cs["mask"]) // 32 * 32, 96) + N - 1
    assert cs["B"] == 2 and cs["cfg_scale"] > 1 and 2 * B * Ts > 16384
    rep = lambda t: t.repeat(B // 2, *([1] * (t.dim() - 1))).cuda()
    emb, img, mask = rep(cs["emb"]), rep(cs["img"]), rep(cs["mask"])
    tokens = torch.randint(0, V, (B, N), generator=torch.Generator().manual_seed(7), dtype=torch.int32).cuda()
    eng = _engine(cs, prec)
    eng.encode_control(img)
    kw = _kw(cs, emb_masks=mask)
    nll = eng.score(emb, tokens, **kw)
    assert torch.isfinite(nll).all() and not torch.equal(nll[0], nll[2])          # same prompt and control, other tokens
    for j in (0, 42, 43, 63, 64, 85, 86, 127):
        eng.encode_control(img[j:j + 1])
        n1 = eng.score(emb[j:j + 1], tokens[j:j + 1], **_kw(cs, emb_masks=mask[j:j + 1]))
        assert torch.equal(n1[0], nll[j]), (prec, j, float((n1[0] - nll[j]).abs().max()))
    eng.close()


# ------------------------------------------------------------------ 6: semantics
@pytest.mark.parametrize("prec", PRECS)
def test_score_control_and_strength_semantics(prec):
    cs = load_case("tiny_depth_cfg4")
    tokens = torch.from_numpy(cs["gold"]["tokens"]).cuda(); emb = cs["emb"].cuda()
    eng = _engine(cs, prec)
    eng.encode_control(cs["img"].cuda())
    base = eng.score(emb, tokens, **_kw(cs, cfg_scale=4.0, control_strength=1.0))
    assert not torch.equal(base, eng.score(emb, tokens, use_control=False, **_kw(cs, cfg_scale=4.0, control_strength=1.0)))
    assert not torch.equal(base, eng.score(emb, tokens, **_kw(cs, cfg_scale=4.0, control_strength=0.6)))
    one = eng.score(emb, tokens, **_kw(cs, cfg_scale=1.0, control_strength=1.0))
    assert torch.equal(one, eng.score(emb, tokens, **_kw(cs, cfg_scale=1.0, control_strength=0.6)))          # the reference's quirk (generate.py:87-92)
    eng.close()


@pytest.mark.parametrize("prec", PRECS)
def test_score_cfg_interval_semantics(prec):
    cs = load_case("tiny_cfg_interval"); iv = cs["cfg_interval"]
    assert cs["cfg_scale"] > 1 and 0 < iv + 2 < cs["n_new"] and cs["control_strength"] == 1.0
    tokens = torch.from_numpy(cs["gold"]["tokens"]).cuda(); emb = cs["emb"].cuda()
    eng = _engine(cs, prec)
    eng.encode_control(cs["img"].cuda())
    mixed = eng.score(emb, tokens, **_kw(cs))
    plain = eng.score(emb, tokens, **_kw(cs, cfg_scale=1.0, cfg_interval=-1))
    first = iv + 2                                        # the token loop drops the mix once step - 1 > cfg_interval
    assert torch.equal(mixed[:, first:], plain[:, first:])
    assert not torch.isclose(mixed[:, :first], plain[:, :first]).all()
    eng.close()


def test_generate_score_loss_with_and_without_valid():
    from controlar_amd.generate import score
    from controlar_amd.models import Transformer
    cs = load_case("tiny_depth_cfg4"); cfg = cs["cfg"]
    gpt = Transformer(cfg.gpt, cfg.vit).to("cuda", dtype=torch.float32)
    gpt.load_state_dict(cs["gsd"], strict=False); gpt.eval()
    tokens = torch.from_numpy(cs["gold"]["tokens"]).cuda()
    args = dict(emb_masks=_mask(cs), condition=cs["img"].cuda(), cfg_scale=cs["cfg_scale"], control_strength=cs["control_strength"])
    nll, loss = score(gpt, cs["emb"].cuda(), tokens, **args)
    assert nll.dtype == torch.float32 and tuple(nll.shape) == (cs["B"], cs["n_new"]) and loss.dim() == 0 and loss.dtype == torch.float64
    np.testing.assert_allclose(float(loss), float(nll.double().mean()), rtol=1e-12)
    d = np.abs(nll.cpu().numpy() - nll_ref(cs["gold"]["logits"], cs["gold"]["tokens"]))
    assert d.max() <= 2 * (F32_ATOL + F32_RTOL * np.abs(cs["gold"]["logits"]).max())
    valid = torch.zeros(cs["B"], device="cuda"); valid[0] = 1
    _, lv = score(gpt, cs["emb"].cuda(), tokens, valid=valid, **args)
    np.testing.assert_allclose(float(lv), float(nll[0].double().mean()), rtol=1e-12)
    _, l0 = score(gpt, cs["emb"].cuda(), tokens, valid=torch.zeros(cs["B"], device="cuda"), **args)
    assert float(l0) == 0.0


# ------------------------------------------------------------------ 7: errors, without a fault
def test_score_refusals_leave_the_context_usable():
    from controlar_amd import _lib as L, config as Cfg
    from controlar_amd.engine import Engine
    c2i = Engine(Cfg.tiny_c2i(), "bf16")
    sp = L.CarSampling(); sp.cfg_scale = 1.0
    assert c2i.lib.car_score(c2i._h, None, 0, None, 1, 4, 0, C.byref(sp), None, None, None, None) != 0          # refused before any argument is read
    assert b"c2i" in c2i.lib.car_last_error(c2i._h)
    with pytest.raises(RuntimeError, match="c2i"):
        c2i.score(torch.zeros(1, 1, 8), torch.zeros(1, 4, dtype=torch.int32))
    c2i.close()

    cs = load_case("tiny_canny_cfg1"); V = cs["cfg"].gpt.vocab_size; B, N = cs["B"], cs["n_new"]
    emb = cs["emb"].cuda(); tokens = torch.from_numpy(cs["gold"]["tokens"]).cuda()
    eng = _engine(cs, "bf16")
    with pytest.raises(RuntimeError, match="control tokens"):                  # use_control without a preceding car_encode_control
        eng.score(emb, tokens, **_kw(cs))
    eng.encode_control(cs["img"].cuda())
    good = eng.score(emb, tokens, **_kw(cs))
    with pytest.raises(RuntimeError, match="block_size"):
        eng.score(emb, torch.zeros(B, cs["cfg"].gpt.block_size + 1, dtype=torch.int32).cuda(), use_control=False, **_kw(cs))
    for bad in (tokens[0], tokens[:1], tokens[:, :, None], tokens.float()):
        with pytest.raises(ValueError, match="tokens"):
            eng.score(emb, bad, **_kw(cs))
    with pytest.raises(RuntimeError, match="out of range"):                    # a host tensor is checked for free
        eng.score(emb, torch.full((B, N), V, dtype=torch.int32), **_kw(cs))
    bad = tokens.clone(); bad[0, 3] = V                                        # a device tensor: the sticky flag, no host read-back
    eng.score(emb, bad, **_kw(cs))
    with pytest.raises(RuntimeError, match="car_score"):
        eng.check_errors()
    assert torch.equal(eng.score(emb, tokens, **_kw(cs)), good)               # the context stays usable
    eng.check_errors()
    eng.close()


# ------------------------------------------------------------------ the kernel alone (car_debug_score_rows) against torch fp64 on the host
def _kernel_inputs(R, V, D, bf16, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, D, generator=g); w = torch.randn(V, D, generator=g) / D ** 0.5
    if bf16:
        x, w = x.bfloat16().float(), w.bfloat16().float()
    t = torch.randint(0, V, (R,), generator=g, dtype=torch.int32)
    t[0] = 0; t[-1] = V - 1
    return x, w, t


def _to200(x, w, rows, bf16):
    """rows whose logits reach about +-200: x = +-200 w[n] / |w[n]|^2 — a sum of exp without the running maximum overflows fp32 (e^200)"""
    for i, (r, n) in enumerate(rows):
        v = (200.0 if i % 2 == 0 else -200.0) * w[n] / float(w[n].double().pow(2).sum())
        x[r] = v.bfloat16().float() if bf16 else v
    return x


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("V,D", [(1024, 256), (16384, 1280)])
def test_score_kernel_against_fp64(V, D, prec):
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    bf16 = prec == "bf16"
    eng = Engine(Cfg.tiny_t2i(), prec)
    w64 = None
    for R in (1, 37, 130):
        for pair in (None, "1", "4", "mixed"):
            rows = R if pair is None else 2 * R
            x, w, t = _kernel_inputs(rows, V, D, bf16, seed=R)
            t = t[:R].clone(); t[0] = 0; t[-1] = V - 1
            if R > 1:
                x = _to200(x, w, [(1, 7), (R // 2, V - 3)] if pair is None else [(1, 7), (R + 1, 7)], bf16)
            w64 = w.double()
            lg = x.double() @ w64.T
            ps = None
            if pair is not None:
                ps = torch.full((R,), 4.0) if pair == "4" else torch.ones(R)
                if pair == "mixed":
                    ps = torch.tensor([1.0, 4.0, 1.5, 7.5])[torch.arange(R) % 4]
                c, u = lg[:R], lg[R:]
                lg = torch.where(ps[:, None] == 1.0, c, u + (c - u) * ps.double()[:, None])
            want = nll_ref(lg.numpy(), t.numpy())
            nll, got = eng.score_rows(x, w, t, pair_scale=ps, return_logits=True)
            nll_only = eng.score_rows(x, w, t, pair_scale=ps)
            assert torch.equal(nll, nll_only)
            nll, got = nll.cpu().numpy().astype(np.float64), got.cpu().numpy().astype(np.float64)
            eps = F32_ATOL + F32_RTOL * np.abs(lg.numpy())
            dl = np.abs(got - lg.numpy())
            assert (dl <= eps).all(), (R, pair, float(dl.max()))
            dn = np.abs(nll - want)
            bound = fused_bound(want, V) + eps.max(axis=-1)
            assert np.isfinite(nll).all() and (dn <= bound).all(), (R, pair, float(dn.max()), float(bound.min()))
            if R > 1 and pair is None:
                assert np.abs(lg.numpy()).max() > 150          # the overflow case is really in the input
    eng.check_errors()
    eng.close()
