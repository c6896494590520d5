"""Mints tests/golden/resize_*.npz, the fixtures of car_resize, from Pillow itself: Image.fromarray(x).resize(size, f, box=box).

    python tests/golden/make_resize_golden.py            # rewrites every fixture (needs Pillow)

Each case holds two inputs from a seeded numpy generator, one of noise and one of {0, 255} cells (the binary one drives the negative lobes of BICUBIC and
LANCZOS into the clamp), Pillow's output for the five filters on both, and the coefficient tables (`kk`, `bounds`) of both axes for the five filters
as the NumPy restatement below computes them.  The restatement is the specification car_resize implements (ImagingResample for 8-bit images:
per-axis taps in double, 22-bit fixed point, a horizontal pass into a uint8 intermediate, then a vertical pass, int32 sums); before anything is
written it is asserted equal to Pillow, bit for bit, on every case, input and filter.  The seed of a case is the first one, counting up from the
case's base seed, whose binary input meets the fixture conditions tests/test_resize_cpu.py checks (a 0 and a 255 in the BICUBIC and LANCZOS
outputs; tap sums below 0 and above 255 before the clamp wherever the geometry allows them; five pairwise different outputs on the noise input).
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PRECISION_BITS = 22
# Pillow's Image.Resampling codes
LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 1, 2, 3, 4, 5
FILTERS = {"lanczos": LANCZOS, "bilinear": BILINEAR, "bicubic": BICUBIC, "box": BOX, "hamming": HAMMING}

# name -> (input shape (H, W[, 3]), output (Ho, Wo), box (x0, y0, x1, y1) or None, base seed, overshoot possible)
CASES = {
    "down_53x37": ((53, 37, 3), (16, 16), None, 100, True),                      # non-integer downscale
    "up_l_31x20": ((31, 20), (48, 64), None, 200, True),                          # upscale, C = 1
    "half_64x64": ((64, 64, 3), (32, 32), None, 300, True),                       # exact half: BOX taps land on cell edges
    "vonly_70x50": ((70, 50, 3), (35, 50), None, 400, True),                      # vertical pass only
    "honly_70x50": ((70, 50, 3), (70, 25), None, 500, True),                      # horizontal pass only
    "copy_64x48": ((64, 48, 3), (64, 48), (0, 0, 48, 64), 600, False),            # both passes skipped: a copy
    "box_60x48": ((60, 48, 3), (32, 32), (3.5, 2, 40.25, 30), 700, True),         # fractional box
    "box_96x96": ((96, 96, 3), (32, 32), (10.5, 7.25, 80, 91.5), 800, True),      # fractional box
    "deep_l_200x300": ((200, 300), (16, 24), None, 900, True),                    # Lanczos ksize 77
    "up_33x47": ((33, 47, 3), (144, 160), None, 1000, True),                      # large upscale: edge-clipped taps dominate
    "tiny_2x3": ((2, 3, 3), (4, 5), None, 1100, True),                            # smaller than the filter support
    "one_1x1": ((1, 1, 3), (8, 8), None, 1200, False),                            # one pixel: every tap sum is the pixel itself
    "sq_40x56": ((40, 56, 3), (64, 64), None, 1400, True),                        # what resize_image(., 64) and the DPT processor at size 64 make of it
}
CROP_CASE = ("crop_150x210", (150, 210, 3), 32, 1300)                            # center_crop_arr(., 32): BOX, BOX, BICUBIC to 45 x 32, crop


# ----------------------------------------------------------------------------------------------- the restatement
def _f_box(x):
    return 1.0 if (x > -0.5 and x <= 0.5) else 0.0


def _f_bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _f_hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x *= math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


def _f_bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x *= math.pi
    return math.sin(x) / x


def _f_lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


_F = {BOX: (_f_box, 0.5), BILINEAR: (_f_bilinear, 1.0), HAMMING: (_f_hamming, 1.0), BICUBIC: (_f_bicubic, 2.0), LANCZOS: (_f_lanczos, 3.0)}


def coeffs(in_size, in0, in1, out_size, flt):
    """One axis: (kk int32 [out_size, ksize], bounds int32 [out_size, 2] = (xmin, xmax))."""
    f, sup = _F[flt]
    scale = filterscale = (in1 - in0) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = sup * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return kk, bounds


def _pass(a, kk, bounds, axis, stat):
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((len(bounds),) + a.shape[1:], np.uint8)
    for i, (x0, n) in enumerate(bounds):
        s = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[i, :n].astype(np.int64), a[x0:x0 + n], axes=(0, 0))
        assert int(np.abs(s).max()) < 2 ** 31                      # Pillow accumulates in int32, and so does the kernel
        s >>= PRECISION_BITS
        stat[0] += int((s < 0).sum())
        stat[1] += int((s > 255).sum())
        out[i] = np.clip(s, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(a, size, flt, box=None, stat=None):
    """a uint8 [H, W] or [H, W, C]; size = (Wo, Ho) as PIL orders it.  stat, if given, is a two-element list that receives the number of tap sums
    below 0 and above 255 before the clamp (both passes)."""
    stat = [0, 0] if stat is None else stat
    H, W = a.shape[:2]
    Wo, Ho = size
    if box is None:
        box = (0, 0, W, H)
    flat = a.ndim == 2
    if flat:
        a = a[:, :, None]
    need_h = Wo != W or box[0] != 0 or box[2] != W
    need_v = Ho != H or box[1] != 0 or box[3] != H
    if need_h:
        a = _pass(a, *coeffs(W, box[0], box[2], Wo, flt), 1, stat)
    if need_v:
        a = _pass(a, *coeffs(H, box[1], box[3], Ho, flt), 0, stat)
    a = np.ascontiguousarray(a)
    return a[:, :, 0] if flat else a


def center_crop_sizes(H, W, image_size):
    """The chain of (Wo, Ho, filter) resizes ADM's centre crop takes, and the crop window (y, x) of the last one."""
    steps = []
    while min(W, H) >= 2 * image_size:
        W, H = W // 2, H // 2
        steps.append((W, H, BOX))
    scale = image_size / min(W, H)
    W, H = round(W * scale), round(H * scale)
    steps.append((W, H, BICUBIC))
    return steps, ((H - image_size) // 2, (W - image_size) // 2)


# ----------------------------------------------------------------------------------------------- minting
def _inputs(shape, seed):
    """(noise, binary): uniform 8-bit noise, and a {0, 255} image of random cells, about four per side and independent per channel.  Flat cells with
    sharp edges are what makes the negative lobes overshoot: single-pixel binary noise averages to grey in any downscale and never reaches the clamp."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, shape, dtype=np.uint8)
    H, W = shape[:2]
    ch, cw = max(1, H // 4), max(1, W // 4)
    cells = rng.integers(0, 2, (-(-H // ch), -(-W // cw)) + tuple(shape[2:]))
    binary = np.repeat(np.repeat(cells, ch, axis=0), cw, axis=1)[:H, :W]
    return noise, np.ascontiguousarray(binary * 255).astype(np.uint8)


def _conditions(noise_out, binary_out, over, overshoot):
    for f in (BICUBIC, LANCZOS):
        if binary_out[f].min() != 0 or binary_out[f].max() != 255:
            return False
        if overshoot and (over[f][0] == 0 or over[f][1] == 0):
            return False
    codes = sorted(noise_out)
    return overshoot is False or all(not np.array_equal(noise_out[a], noise_out[b]) for i, a in enumerate(codes) for b in codes[i + 1:])


def build_case(name):
    """The arrays of one fixture, from Pillow; the restatement is asserted equal to it on the way."""
    from PIL import Image
    shape, (Ho, Wo), box, seed0, overshoot = CASES[name]
    H, W = shape[:2]
    for seed in range(seed0, seed0 + 100):
        noise, binary = _inputs(shape, seed)
        out = {"noise": {}, "binary": {}}
        over = {}
        for fname, f in FILTERS.items():
            for kind, x in (("noise", noise), ("binary", binary)):
                ref = np.asarray(Image.fromarray(x).resize((Wo, Ho), f, box=box))
                stat = [0, 0]
                got = resize(x, (Wo, Ho), f, box, stat)
                assert np.array_equal(ref, got), (name, fname, kind, "the restatement differs from Pillow")
                out[kind][f] = ref
                if kind == "binary":
                    over[f] = stat
        if _conditions(out["noise"], out["binary"], over, overshoot):
            break
    else:
        raise RuntimeError(f"{name}: no seed in {seed0}..{seed0 + 99} meets the fixture conditions")
    b = box if box is not None else (0, 0, W, H)
    arrs = dict(x_noise=noise, x_binary=binary, out_size=np.array([Ho, Wo], np.int32), box=np.array(b, np.float64), has_box=np.array(box is not None),
                seed=np.array(seed, np.int64))
    for fname, f in FILTERS.items():
        arrs[f"noise_{fname}"] = out["noise"][f]
        arrs[f"binary_{fname}"] = out["binary"][f]
        arrs[f"over_{fname}"] = np.array(over[f], np.int64)
        arrs[f"kkh_{fname}"], arrs[f"bh_{fname}"] = coeffs(W, b[0], b[2], Wo, f)
        arrs[f"kkv_{fname}"], arrs[f"bv_{fname}"] = coeffs(H, b[1], b[3], Ho, f)
    return arrs


def build_crop_case():
    from PIL import Image
    name, shape, image_size, seed = CROP_CASE
    arrs = dict(image_size=np.array(image_size, np.int32))
    steps, (cy, cx) = center_crop_sizes(shape[0], shape[1], image_size)
    arrs["resized_size"] = np.array(steps[-1][:2], np.int32)
    for kind, x in zip(("noise", "binary"), _inputs(shape, seed)):
        im, mine = Image.fromarray(x), x
        for Wn, Hn, f in steps:
            im = im.resize((Wn, Hn), resample=f)
            mine = resize(mine, (Wn, Hn), f)
        ref = np.asarray(im)
        assert np.array_equal(ref, mine), (name, kind, "the restatement differs from Pillow")
        arrs[f"x_{kind}"] = x
        arrs[f"resized_{kind}"] = ref
        arrs[f"crop_{kind}"] = np.ascontiguousarray(ref[cy: cy + image_size, cx: cx + image_size])
    return arrs


def mint(name, out_dir=HERE):
    arrs = build_crop_case() if name == CROP_CASE[0] else build_case(name)
    path = os.path.join(out_dir, f"resize_{name}.npz")
    np.savez_compressed(path, **arrs)
    return path


if __name__ == "__main__":
    total = 0
    for n in list(CASES) + [CROP_CASE[0]]:
        p = mint(n, sys.argv[1] if len(sys.argv) > 1 else HERE)
        total += os.path.getsize(p)
        print(f"{os.path.basename(p)}: {os.path.getsize(p)} bytes")
    print(f"total {total} bytes")
