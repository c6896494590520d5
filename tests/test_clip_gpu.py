"""The CLIP score on the GPU (pytest -m gpu): car_clip_encode_image / car_clip_encode_text / car_clip_score against the HF CLIPModel goldens of
tests/golden/make_clip_golden.py (weights regenerated from synth.clip_state_dict; the goldens hold inputs and outputs only).

Tolerances, all read from tests/golden/clip_measured.json:
  pixel_values   bit-equal (the uint8 resize is Pillow-exact, the float steps are correctly rounded)
  fp32 mode      embeddings and cosines within 16 x the fp32-vs-fp64 deviation of HF itself on that fixture (the summation order differs, nothing else)
  bf16 mode      mean error <= 1.5 x and max error <= 2 x HF's own bf16-vs-fp32 deviation on that fixture, plus the absolute slack of the T5 test
                 (1e-3 on the mean, 1e-2 on the max)"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
MEASURED = json.load(open(os.path.join(GOLD, "clip_measured.json")))
_CACHE = {}


def _cfg(name):
    from controlar_amd import config as C
    return {"clip_tiny": C.tiny_clip, "clip_small": C.small_clip, "clip_b32": C.clip_vit_b32}[name]()


def _scorer(name, precision):
    """One scorer per (fixture, precision) for the whole module; the full-size one is not kept."""
    from controlar_amd import synth
    from controlar_amd.clip import CLIPScorer
    key = (name, precision)
    if key in _CACHE:
        return _CACHE[key]
    s = CLIPScorer(_cfg(name), synth.clip_state_dict(_cfg(name)), precision=precision, device="cuda")
    if name != "clip_b32":
        _CACHE[key] = s
    return s


def _run_fixture(name, precision):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    s = _scorer(name, precision)
    img = torch.cat([s.encode_image(torch.from_numpy(g[f"img{i}"]).cuda()[None]) for i in range(4)])
    txt = s.encode_text(torch.from_numpy(g["ids"]).cuda())
    cos, mean = s.engine.clip_score(img, txt, n_mean=3)
    s.engine.check_errors()
    assert abs(float(mean) - float(cos[:3].double().mean())) < 1e-12
    out = {"img_emb": img.cpu().numpy(), "txt_emb": txt.cpu().numpy(), "cos": cos.cpu().numpy()}
    if name == "clip_b32":
        s.engine.close()
    return g, out


@pytest.mark.parametrize("requant", [False, True])
def test_pixel_values_bit_equal(requant):
    from controlar_amd import config as C
    from controlar_amd.engine import Engine
    g = np.load(os.path.join(GOLD, "clip_tiny.npz"))
    eng = Engine(C.tiny_t2i(), "fp32")
    eng.clip_configure(C.tiny_clip())               # the pixel path needs no weights
    want = g["pixel_values_requant" if requant else "pixel_values"]
    for i in range(4):
        src = torch.from_numpy(g[f"img{i}"]).cuda()
        keep = src.clone()
        pv = eng.clip_encode_image(src[None], requant=requant, want_pixel_values=True, want_embedding=False)
        assert pv.shape == (1, 3, 32, 32)
        assert np.array_equal(pv[0].cpu().numpy(), want[i]), (i, tuple(src.shape))
        assert torch.equal(src, keep)                # requant works on a copy
    both = torch.stack([torch.from_numpy(g["img2"]).flip(0), torch.from_numpy(g["img2"])]).cuda()      # a batch of two: the second image starts at an odd byte offset
    pv2 = eng.clip_encode_image(both, requant=requant, want_pixel_values=True, want_embedding=False)
    assert np.array_equal(pv2[1].cpu().numpy(), want[2])
    eng.close()


@pytest.mark.parametrize("name", ["clip_tiny", "clip_small", "clip_b32"])
def test_fp32_within_16x_of_the_references_own_fp32_noise(name):
    g, out = _run_fixture(name, "fp32")
    for k in ("img_emb", "txt_emb", "cos"):
        err, bound = float(np.abs(out[k].astype(np.float64) - g[k]).max()), 16.0 * MEASURED[name]["fp32_vs_fp64_max"][k]
        print(f"{name} fp32 {k}: max err {err:.3e} bound {bound:.3e}")
    for k in ("img_emb", "txt_emb", "cos"):
        err, bound = float(np.abs(out[k].astype(np.float64) - g[k]).max()), 16.0 * MEASURED[name]["fp32_vs_fp64_max"][k]
        assert err <= bound, (name, k, err, bound)


@pytest.mark.parametrize("name", ["clip_tiny", "clip_small", "clip_b32"])
def test_bf16_within_the_references_bf16_roundoff(name):
    g, out = _run_fixture(name, "bf16")
    m = MEASURED[name]
    for k in ("img_emb", "txt_emb", "cos"):
        e = np.abs(out[k].astype(np.float64) - g[k])
        print(f"{name} bf16 {k}: mean {e.mean():.3e} max {e.max():.3e}  hf mean {m['bf16_vs_fp32_mean'][k]:.3e} max {m['bf16_vs_fp32_max'][k]:.3e}")
    for k in ("img_emb", "txt_emb", "cos"):
        e = np.abs(out[k].astype(np.float64) - g[k])
        assert e.mean() <= 1.5 * m["bf16_vs_fp32_mean"][k] + 1e-3, (name, k, e.mean())
        assert e.max() <= 2.0 * m["bf16_vs_fp32_max"][k] + 1e-2, (name, k, e.max())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_text_is_causal(precision):
    s = _scorer("clip_tiny", precision)
    cfg = s.config
    g = np.load(os.path.join(GOLD, "clip_tiny.npz"))
    ids = torch.from_numpy(g["ids"]).cuda()                    # lengths 2, 9, 40, 77
    base = s.encode_text(ids)
    after = ids.clone()
    after[0, 2:] = 7; after[1, 9:] = 3; after[2, 40:] = cfg.eot_id       # ids behind the end-of-text id, a second end-of-text id among them
    got = s.encode_text(after)
    assert torch.equal(got, base)
    before = ids.clone()
    before[1, 4] = (before[1, 4] + 1) % (cfg.eot_id - 1) + 1
    got = s.encode_text(before)
    assert not torch.equal(got[1], base[1]) and torch.equal(got[0], base[0]) and torch.equal(got[2:], base[2:])
    short = s.encode_text(ids[:2, :9].contiguous())               # T = 9 < context length: the same rows
    assert torch.equal(short, base[:2])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_batch_invariance_across_the_chunk_boundary(precision):
    """Chunks hold at most 16384 activation rows: 212 captions of 77 tokens, 3276 tiny images of 5 tokens.  Both batches cross the boundary."""
    from controlar_amd import synth
    s = _scorer("clip_tiny", precision)
    Bt, Bi = 215, 3280
    gen = torch.Generator().manual_seed(5)
    imgs = torch.randint(0, 256, (Bi, 40, 56, 3), generator=gen, dtype=torch.uint8).cuda()
    ids = synth.clip_tokens(Bt, s.config, lengths=[2 + (11 * i) % 76 for i in range(Bt)]).cuda()
    img, txt = s.encode_image(imgs, requant=True), s.encode_text(ids)
    cos = s.engine.clip_score(img[:Bt], txt)
    for i in (0, 211, 212, 214):
        t = s.encode_text(ids[i:i + 1].contiguous())
        a = s.encode_image(imgs[i:i + 1].contiguous(), requant=True)
        assert torch.equal(t[0], txt[i]) and torch.equal(a[0], img[i]), i
        assert torch.equal(s.engine.clip_score(a, t)[0], cos[i]), i
    for i in (3275, 3276, 3279):
        assert torch.equal(s.encode_image(imgs[i:i + 1].contiguous(), requant=True)[0], img[i]), i
    assert torch.equal(s.encode_image(imgs, requant=True), img) and torch.equal(s.encode_text(ids), txt)      # a second call
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        img2, txt2 = s.encode_image(imgs, requant=True), s.encode_text(ids)
        cos2 = s.engine.clip_score(img2[:Bt], txt2)
    side.synchronize()
    assert torch.equal(img2, img) and torch.equal(txt2, txt) and torch.equal(cos2, cos)
    assert not torch.equal(s.encode_image(imgs[:2], requant=False), img[:2])                                   # requant changes the pixels CLIP sees


def test_full_size_rows_keep_their_bits_when_the_batch_changes_the_gemm_kernel():
    """At ViT-B/32 a full chunk gives the wide linears enough tiles for car_launch_gemm's LDS-DMA kernel, a small batch takes the register-staged one:
    the bits of a row must not depend on which.  216 captions (chunks of 212 + 4) and 330 images (327 + 3) against the same rows encoded four at a time."""
    g = np.load(os.path.join(GOLD, "clip_b32.npz"))
    s = _scorer("clip_b32", "bf16")
    ids = torch.from_numpy(g["ids"]).cuda()
    im = torch.from_numpy(g["img3"]).cuda()
    assert tuple(im.shape) == (224, 224, 3)
    four = torch.stack([im, im.flip(0), im.flip(1), im.flip(0).flip(1)])
    txt4, img4 = s.encode_text(ids), s.encode_image(four)
    txt, img = s.encode_text(ids.repeat(54, 1)), s.encode_image(torch.cat([four.repeat(82, 1, 1, 1), four[:2]]))
    s.engine.check_errors()
    assert torch.equal(txt, txt4.repeat(54, 1))
    assert torch.equal(img, torch.cat([img4.repeat(82, 1), img4[:2]]))
    s.engine.close()


def test_score_equals_the_assembled_path_and_clipscore_cuts_at_how_many():
    from controlar_amd import synth
    from controlar_amd.clip import center_crop_offset
    from controlar_amd.metrics import CLIPScore
    s = _scorer("clip_tiny", "bf16")
    e = s.engine
    gen = torch.Generator().manual_seed(9)
    pixels = (torch.rand(5, 3, 72, 100, generator=gen) * 2.4 - 1.2).cuda()          # landscape, values beyond [-1, 1] are clamped
    ids = synth.clip_tokens(5, s.config, lengths=[2, 5, 20, 60, 77]).cuda()
    got = s.score(pixels, ids, eval_res=48)
    u8 = e.pixels_to_u8(pixels)
    left = center_crop_offset(100, 72)
    sq = e.resize(u8, (48, 48), "lanczos", box=(left, 0, left + 72, 72))
    want = e.clip_score(e.clip_encode_image(sq, requant=True), e.clip_encode_text(ids))
    assert got.shape == (5,) and got.dtype == torch.float32 and torch.equal(got, want)
    assert float(got.abs().max()) <= 1.0 + 1e-6 and float(got.abs().max()) > 0
    m = CLIPScore(s, how_many=7, eval_res=48)
    m.update(pixels[:3], ids[:3]); m.update(pixels[3:], ids[3:]); m.update(pixels, ids)
    assert m.per_image.shape == (10,) and torch.equal(m.per_image[:5], got)
    assert m.calculate() == float(m.per_image[:7].double().mean())


def test_refusals_leave_the_context_usable():
    import dataclasses
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    cfg = C.tiny_clip()
    eng = Engine(C.tiny_t2i(), "bf16")
    img = torch.zeros(1, 40, 40, 3, dtype=torch.uint8).cuda()
    ids = synth.clip_tokens(2, cfg, lengths=[3, 10]).cuda()
    with pytest.raises(RuntimeError, match="car_clip_configure"):
        eng.clip_encode_image(img)
    with pytest.raises(RuntimeError, match="car_clip_configure"):
        eng.clip_encode_text(ids)
    with pytest.raises(RuntimeError, match="64 wide"):
        eng.clip_configure(dataclasses.replace(cfg, vision_width=192, vision_heads=2))          # head width 96
    with pytest.raises(RuntimeError, match="multiple of patch"):
        eng.clip_configure(dataclasses.replace(cfg, image_size=40))
    with pytest.raises(RuntimeError, match="multiples of 32"):
        eng.clip_configure(dataclasses.replace(cfg, text_mlp=250))
    eng.clip_configure(cfg)
    with pytest.raises(RuntimeError, match="not loaded"):
        eng.clip_encode_text(ids)
    eng.load_clip_state_dict(synth.clip_state_dict(cfg))
    base = eng.clip_encode_text(ids)
    with pytest.raises(RuntimeError, match="78 tokens exceed"):
        eng.clip_encode_text(torch.ones(1, 78, dtype=torch.int64).cuda())
    with pytest.raises(RuntimeError, match="out of range"):
        eng.clip_encode_text(torch.full((1, 4), cfg.vocab_size, dtype=torch.int64))             # host ids are checked for free
    bad = ids.clone(); bad[1, 2] = cfg.vocab_size                                              # device ids: read as 0, sticky flag, no fault
    as_zero = ids.clone(); as_zero[1, 2] = 0
    got = eng.clip_encode_text(bad)
    with pytest.raises(RuntimeError, match="token id outside"):
        eng.check_errors()
    assert torch.equal(got, eng.clip_encode_text(as_zero))
    assert torch.equal(eng.clip_encode_text(ids), base)                                        # the context still works, the flag is cleared
    eng.check_errors()
    eng.close()


def test_packed_cache_carries_clip(tmp_path):
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    cfg = C.tiny_clip()
    ids = synth.clip_tokens(3, cfg, lengths=[2, 30, 77]).cuda()
    src = _scorer("clip_tiny", "bf16").engine
    path = str(tmp_path / "clip.pack").encode()
    src._check(src.lib.car_export_packed(src._h, path), "car_export_packed")
    dst = Engine(C.tiny_t2i(), "bf16")
    dst.clip_configure(cfg)
    dst._check(dst.lib.car_import_packed(dst._h, path), "car_import_packed")
    assert torch.equal(dst.clip_encode_text(ids), src.clip_encode_text(ids))
    dst.close()
