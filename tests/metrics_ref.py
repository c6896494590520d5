"""Test infrastructure for the control-consistency metrics: plain-torch and NumPy restatements of what car_ms_ssim, car_f1, car_rmse and
car_pixels_to_u8 compute, and the seeded inputs the tests share.  Nothing here is product code and nothing here touches the GPU.

ms_ssim is the LITERAL definition (torchmetrics' MultiScaleStructuralSimilarityIndexMeasure(data_range=1.0), 1.x defaults): reflect padding by 5, a
grouped 11 x 11 convolution of the five maps, the clamp of both variances, the crop of 5, relu of the means, floor-mode avg_pool2d.  Its keyword
arguments exist to state wrong variants (crop, ceil_mode, sigma) and the valid-convolution form the kernel uses (valid=True); the oracle of every test is
the call without any of them, in fp64."""
import numpy as np
import torch
import torch.nn.functional as F

BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2


def gaussian(dtype, sigma=1.5, size=11):
    d = (torch.arange(size, dtype=dtype) - (size - 1) / 2) / sigma
    g = torch.exp(-d * d / 2)
    return g / g.sum()


def ms_ssim(pred, target, scale=(1.0, 1.0), dtype=torch.float64, crop=5, ceil_mode=False, sigma=1.5, valid=False):
    """pred, target [B,C,H,W] -> (per-image value [B], per-scale table [B,5,2] of the (ssim, cs) means after relu), both in `dtype`."""
    H, W = pred.shape[-2:]
    if min(H, W) < 32:
        raise ValueError(f"both sides must be at least 32, got {H} x {W}")
    if H // 16 <= 10 or W // 16 <= 10:
        raise ValueError(f"both sides must be at least 176 (side // 16 > 10), got {H} x {W}")
    p = (pred.to(dtype) * scale[0]).clamp(0, 1)
    t = (target.to(dtype) * scale[1]).clamp(0, 1)
    B, C = p.shape[:2]
    g = gaussian(dtype, sigma).to(p.device)
    w = torch.outer(g, g).expand(C, 1, 11, 11).contiguous()
    table = []
    for _ in range(5):
        pp, tt = (p, t) if valid else (F.pad(p, (5, 5, 5, 5), mode="reflect"), F.pad(t, (5, 5, 5, 5), mode="reflect"))
        mp, mt, epp, ett, ept = F.conv2d(torch.cat([pp, tt, pp * pp, tt * tt, pp * tt]), w, groups=C).split(B)
        vp, vt, cov = (epp - mp * mp).clamp(min=0), (ett - mt * mt).clamp(min=0), ept - mp * mt
        cs = (2 * cov + C2) / (vp + vt + C2)
        ss = (2 * mp * mt + C1) / (mp * mp + mt * mt + C1) * cs
        if not valid:
            ss, cs = ss[..., crop:-crop, crop:-crop], cs[..., crop:-crop, crop:-crop]
        table.append(torch.stack([ss.reshape(B, -1).mean(-1), cs.reshape(B, -1).mean(-1)], dim=-1).relu())
        p, t = F.avg_pool2d(p, 2, ceil_mode=ceil_mode), F.avg_pool2d(t, 2, ceil_mode=ceil_mode)
    table = torch.stack(table, dim=1)                       # [B,5,2]
    b = torch.tensor(BETAS, dtype=dtype, device=p.device)
    val = (table[:, :4, 1] ** b[:4]).prod(-1) * table[:, 4, 0] ** b[4]
    return val, table


def positive(x, value=None, threshold=None):
    x = np.asarray(x)
    return x == value if value is not None else x > threshold


def f1_counts(pred_pos, target_pos):
    """boolean maps [B,H,W] -> (int64 [B,3] = TP, FP, FN; float64 [B] F1, 0 where the denominator is 0)"""
    p, t = pred_pos.reshape(len(pred_pos), -1), target_pos.reshape(len(target_pos), -1)
    cnt = np.stack([(p & t).sum(1), (p & ~t).sum(1), (~p & t).sum(1)], axis=1).astype(np.int64)
    den = 2 * cnt[:, 0] + cnt[:, 1] + cnt[:, 2]
    return cnt, np.where(den > 0, 2.0 * cnt[:, 0] / np.maximum(den, 1), 0.0)


def rmse(pred, label, scale_to_max=False, dtype=torch.float64):
    """pred, label [B,H,W] -> [B] in `dtype`; in fp32 with the script's own expression pred * 255 / pred.max() (evaluations/depth_rmse.py:59)."""
    p, l = pred.to(dtype), label.to(dtype)
    if scale_to_max:
        p = p * 255 / p.amax(dim=(1, 2), keepdim=True)
    return ((p - l) ** 2).mean(dim=(1, 2)).sqrt()


def pixels_to_u8(x):
    """torchvision's save_image(normalize=True, value_range=(-1, 1)) on fp32 [B,3,H,W] -> uint8 [B,H,W,3]"""
    v = ((x.float().clamp(-1, 1) + 1) / 2 * 255 + 0.5).clamp(0, 255).floor()
    return v.to(torch.uint8).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ seeded inputs
def soft_edge_maps(B, C, H, W, seed, disc=True):
    """(target, pred) fp32 [B,C,H,W] in [0,1]: mostly EXACT zeros with a few blurred curves and one flat grey disc — on a flat non-zero patch
    E[p^2] - mu^2 rounds below zero in fp32, so the clamp of the variance matters — and pred a perturbed copy: one curve missing, one extra, the rest
    blended with a two-pixel shift, noise on the strokes only.  disc=False leaves the disc out: curves on exact zeros only."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.arange(H, dtype=torch.float32)[:, None], torch.arange(W, dtype=torch.float32)[None, :]

    def circle():
        cy, cx, r = (torch.rand(3, generator=g) * torch.tensor([H, W, min(H, W) / 2.0])).tolist()
        return ((yy - cy) ** 2 + (xx - cx) ** 2).sqrt().sub(r + 4).abs() < 0.75

    def wave():
        a, ph, y0 = (torch.rand(3, generator=g) * torch.tensor([H / 6.0, 6.28, float(H)])).tolist()
        return (yy - (y0 + a * torch.sin(xx / 17.0 + ph))).abs() < 0.75

    t, p = torch.zeros(B * C, H, W), torch.zeros(B * C, H, W)
    for n in range(B * C):
        strokes = [circle(), wave(), circle(), wave(), circle(), wave()]
        for m in strokes[:5]:
            t[n][m] = 1.0
        for m in strokes[1:]:
            p[n][m] = 1.0
        cy, cx = (torch.rand(2, generator=g) * torch.tensor([float(H), float(W)])).tolist()
        if disc:
            m = (yy - cy) ** 2 + (xx - cx) ** 2 < 14.0 ** 2
            t[n][m] = 0.7
            p[n][m] = 0.7
    k = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0]) / 16
    blur = lambda v: F.conv2d(v[:, None], torch.outer(k, k)[None, None], padding=2)[:, 0].reshape(B, C, H, W).clamp(0, 1)
    t, p = blur(t), blur(p)
    noise = torch.randn(B, C, H, W, generator=g) * 0.08
    p = (0.6 * p + 0.4 * torch.roll(p, 2, dims=-1) + noise * (p > 0)).clamp(0, 1)
    return t.contiguous(), p.contiguous()


# (name, B, C, H, W, seed): the minimum side (scale 5 keeps one pixel per plane); odd at several scales (pooling floor, partial tiles in both axes); three
# channels and three images; the evaluation scripts' own batch
MS_CASES = [("min_176", 2, 1, 176, 176, 101), ("odd_181x203", 2, 1, 181, 203, 102), ("rgb_256x192", 3, 3, 256, 192, 103), ("eval_512", 16, 1, 512, 512, 104)]
MS_FORMS = {"min_176": ("f32", "u8"), "odd_181x203": ("f32", "u8", "same", "inv"), "rgb_256x192": ("f32", "u8"), "eval_512": ("u8",)}


def ms_inputs(name, form):
    """(pred, target, scale) of one case.  f32: both fp32 in 0..1, scale 1.  u8: pred fp32 in 0..255 against a uint8 target, scale 1/255 (the scripts' form).
    same: target against itself.  inv: 1 - target against target (negative means: the relu path).  The last two are curves on exact zeros, without the
    flat disc: on a flat patch the literal definition itself clamps sigma_p^2 but not sigma_pt, and an identical pair no longer scores exactly 1."""
    _, B, C, H, W, seed = next(c for c in MS_CASES if c[0] == name)
    t, p = soft_edge_maps(B, C, H, W, seed, disc=form in ("f32", "u8"))
    if form == "f32":
        return p, t, (1.0, 1.0)
    if form == "u8":
        return (p * 255).contiguous(), (t * 255).round().to(torch.uint8), (1.0 / 255.0, 1.0 / 255.0)
    if form == "same":
        return t.clone(), t, (1.0, 1.0)
    if form == "inv":
        return (1 - t).contiguous(), t, (1.0, 1.0)
    raise KeyError(form)


RMSE_CASES = [(64, 64, False), (64, 64, True), (512, 512, False), (512, 512, True)]


def rmse_inputs(H, W, scale_to_max, B=3):
    """pred: a smooth positive depth-like map (0..~20 under scale_to_max as a DPT emits, 0..255 otherwise); label: uint8"""
    g = torch.Generator().manual_seed(7 * H + W + int(scale_to_max))
    base = F.interpolate(torch.rand(B, 1, 8, 8, generator=g), size=(H, W), mode="bilinear", align_corners=False)[:, 0]
    label = (base * 255).round().clamp(0, 255).to(torch.uint8)
    pred = (base + 0.03 * torch.randn(B, H, W, generator=g)).clamp(min=0) * (20.0 if scale_to_max else 255.0)
    return pred.contiguous(), label


def binary_maps(B, H, W, seed, kind="u8"):
    """two correlated sparse maps: uint8 in {0, 255} or fp32 in 0..255"""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(B, H, W, generator=g) < 0.1
    b = a ^ (torch.rand(B, H, W, generator=g) < 0.03)
    if kind == "u8":
        return (a.to(torch.uint8) * 255), (b.to(torch.uint8) * 255)
    return (a.float() * 200 + torch.rand(B, H, W, generator=g) * 50).contiguous(), (b.float() * 200 + torch.rand(B, H, W, generator=g) * 50).contiguous()
