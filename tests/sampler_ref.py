"""Host reference of the stochastic sampler (sample_stochastic_kernel, controlar_amd/csrc/ops.hip): plain Python and numpy, nothing of the package.

The sampler draws ONE uniform number per (image, step) from a documented Philox4x32-10 stream and inverts the CDF of the filtered softmax with it, so a
token is not merely "distributed right": it is a function of the logits row, the parameters and the counter.  This module computes that function.

  philox4x32_10(counter4, key2)     the generator, Python integers
  uniform(seed, a, b)               the sampler's stream: word 0 of the block at counter (a, b, 0x243F6A88, 0x85A308D3), top 24 bits
  keys32(v, T)                      the fp32 keys x = fl32(v * fl32(1 / max(T, 1e-5))) the kernel filters and exponentiates
  filtered_support_and_cdf(x32, top_k, top_p)   fp64 from there on: support mask, running sum of exp(x - max) in index order, total
  accepts(token, u, cdf, total, m)  token is in the support and u * total lies in [C(token - 1) - m * total, C(token) + m * total]

The margin m (function margin() below), derived from the kernel's arithmetic, NOT measured on it.  Unit: eps = 2^-24, the unit roundoff of fp32; every
error is stated relative to `total`, to first order.

The kernel forms, in fp32, e_j = expf(x_j - mx), thread chunk sums, a block scan, and compares running sums with target = fl(u * total):
  per            keys of one thread's contiguous chunk: 4 * ceil(V / 4096)  (<= 32 at V = 32768)
  loc            a chunk sum, added left to right:                per - 1 roundings
  wave scan      six shuffle levels:                              6 roundings
  wave totals    sixteen waves summed left to right by thread 0:  15 roundings (the first add to 0 is exact)
  excl           sm[w] + inc - v:                                 2 roundings
  run            the owner thread re-adds its chunk onto excl:    per roundings
Each rounding is at most eps times a partial sum, and no partial sum exceeds total, so
  E_sum(run)   = (per - 1) + 6 + 15 + 2 + per
  E_sum(total) = (per - 1) + 6 + 15
Each term carries the error of expf, documented at 1 ulp = 2 eps (HIP math API, single precision), and of its argument: x_j - mx is one fp32 subtraction,
error <= eps * d_j with d_j = mx - x_j, which moves e_j by the factor (1 +- eps * d_j).  Summed over any set of terms that is at most
eps * sum_j e_j * d_j = eps * total * E_p[d] with p the softmax itself, and E_p[d] = H(p) - ln(sum_j e_j) <= ln V because the largest term is 1.  So
  E_term = 2 + ceil(ln V)                     for run and for total alike
The kernel forms x_j with an explicitly rounded multiply (__fmul_rn) wherever it needs it, so x_j - mx sees the same fp32 key as this reference at every
temperature: extreme temperatures need no slack.
target = fl(u * total) adds one rounding; u itself is a 24-bit integer times 2^-24, exact.  The kernel keeps token t iff run(t) > target and
run(t - 1) <= target (or t opens the owner's chunk, whose excl <= target), so against the exact C:
  u * total < C(t) + (E(run) + E(total) + 1) eps total     and     u * total >= C(t - 1) - (same) eps total
  m = [2 * (2 + ceil(ln V)) + 3 * per + 43] * 2^-24
That is 71 at V = 256 or 260, 73 at 1000, 77 at 4096, 115 at 16384, 127 at 16388 (per = 20), 165 at 32768 — the largest the kernel can need.
The filter decisions (k-th value, nucleus cut) get NO margin: the select is exact on the fp32 keys, and the cases keep the cut's cumulative probability
1e-4 away from top_p (tests/test_sampler_cpu.py), fifty times the scan's error.
"""
import math

import numpy as np

M32 = 0xFFFFFFFF
EPS = 2.0 ** -24
# A term exp(x - max) below this is zero in the kernel's fp32 whatever the margin allows (fp32's smallest subnormal is 2^-149, expf returns 0 below about
# e^-104): such a token has no width in the CDF and is not counted into the support.
TINY = 2.0 ** -160


def philox4x32_10(counter4, key2):
    """Philox4x32 with ten rounds (Salmon et al., SC'11; Random123).  counter4, key2: sequences of Python integers < 2^32.  Returns four words."""
    c0, c1, c2, c3 = (int(c) & M32 for c in counter4)
    k0, k1 = (int(k) & M32 for k in key2)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def uniform(seed, a, b):
    """The sampler's stream: one number in [0, 1) per (seed, a, b), a multiple of 2^-24.  Plain calls: a = the image's index in the batch (Engine.sample: step *
    65536 + row), row calls: a = the image's rng_stream (Engine.sample: step * 65536 + rng_stream, modulo 2^32); b = the step of the token loop (Engine.sample: 0)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w0 = philox4x32_10((int(a) & M32, int(b) & M32, 0x243F6A88, 0x85A308D3), (seed & M32, seed >> 32))[0]
    return (w0 >> 8) * 2.0 ** -24


def uniforms(seeds, a, b):
    """uniform() over arrays (broadcast), the same integer arithmetic in numpy uint64 (a 32 x 32 bit product fits); pinned to uniform() in test_sampler_cpu.py."""
    seeds = np.asarray([int(s) & 0xFFFFFFFFFFFFFFFF for s in np.atleast_1d(np.asarray(seeds, dtype=object))], dtype=np.uint64)
    a = np.asarray([int(v) & M32 for v in np.atleast_1d(np.asarray(a, dtype=object))], dtype=np.uint64)
    b = np.asarray([int(v) & M32 for v in np.atleast_1d(np.asarray(b, dtype=object))], dtype=np.uint64)
    seeds, a, b = np.broadcast_arrays(seeds, a, b)
    m = np.uint64(M32)
    sh = np.uint64(32)
    c0, c1 = a.copy(), b.copy()
    c2, c3 = np.full_like(c0, 0x243F6A88), np.full_like(c0, 0x85A308D3)
    k0, k1 = seeds & m, seeds >> sh
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & m, (p0 >> sh) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return (c0 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def keys32(v, temperature):
    """x = fl32(v * fl32(1 / max(T, 1e-5))): one fp32 multiply by the fp32 reciprocal, as the kernel forms it."""
    inv = np.float32(1.0) / np.maximum(np.float32(temperature), np.float32(1e-5))
    return (np.asarray(v, dtype=np.float32) * inv).astype(np.float32)


def margin(V):
    """m of the module header, as a fraction of total."""
    per = 4 * ((V + 4095) // 4096)
    return (2 * (2 + int(math.ceil(math.log(V)))) + 3 * per + 43) * EPS


def filtered_support_and_cdf(x32, top_k, top_p):
    """x32: the fp32 keys of one row (keys32).  Returns (support, cdf, total, info): support a bool mask [V]; cdf[j] = the fp64 sum of exp(x_i - max) over the
    support tokens i <= j (so C(token - 1) = cdf[token - 1], 0 for token 0) and total = cdf[-1].
    top-k: keep x >= the k-th largest value, k clamped to [1, V] (the reference's `logits < kth` removal: ties are kept).
    top-p: on the descending order of the survivors, sorted position a >= 1 goes iff the cumulative probability through a - 1 exceeds top_p; then keep
    x >= the last kept value.
    info: what decidability needs — 'kth', 'next' (the largest value below kth, or None), 'cut_gap' (the distance of top_p from the nearest cumulative
    probability that decides the cut, or None without top-p), 'ties' (how many tokens the value thresholds keep that the reference's index rule would
    remove: copies of the k-th value beyond rank k, copies of the last kept value beyond the nucleus cut)."""
    assert x32.dtype == np.float32 and x32.ndim == 1
    V = x32.shape[0]
    x = x32.astype(np.float64)
    keep = ~np.isnan(x)
    info = {"kth": None, "next": None, "cut_gap": None, "ties": 0}
    if top_k > 0:
        k = min(max(int(top_k), 1), V)
        kth = np.sort(x)[::-1][k - 1]
        keep &= x >= kth
        below = x[x < kth]
        info["kth"], info["next"], info["ties"] = float(kth), (float(below.max()) if below.size else None), int(keep.sum()) - k
    if float(np.float32(top_p)) < 1.0:
        p32 = float(np.float32(top_p))                        # the kernel compares with the fp32 parameter
        s = np.sort(x[keep])[::-1]
        with np.errstate(invalid="ignore"):
            e = np.where(np.isfinite(s), np.exp(s - s[0]), 0.0)
        cp = np.cumsum(e) / e.sum()
        gone = np.concatenate([[False], cp[:-1] > p32])       # position a >= 1 goes iff cp[a - 1] > top_p
        last = s[np.nonzero(~gone)[0].max()]
        info["ties"] += int((s[gone] == last).sum())
        keep &= x >= last
        info["cut_gap"] = float(np.abs(cp - p32).min())
    mx = x[keep].max() if keep.any() else -np.inf
    with np.errstate(invalid="ignore"):
        e = np.where(keep & np.isfinite(x), np.exp(x - mx), 0.0)
    e[e < TINY] = 0.0
    support = e > 0.0
    cdf = np.cumsum(e)
    return support, cdf, float(cdf[-1]) if V else 0.0, info


def accepts(token, u, cdf, total, m, support=None):
    """True iff `token` is in the support and u * total lies in [C(token - 1) - m * total, C(token) + m * total]."""
    token = int(token)
    if token < 0 or token >= cdf.shape[0]:
        return False
    lo = cdf[token - 1] if token > 0 else 0.0
    hi = cdf[token]
    if support is not None and not support[token]:
        return False
    if support is None and not hi > lo:
        return False
    return lo - m * total <= u * total <= hi + m * total


def accepts_all(tokens, us, support, cdf, total, m):
    """accepts() for every draw of one row: (ok [N] bool, needed [N] bool).  needed: accepted, but not at m = 0 with the half-open interval
    C(token - 1) <= u * total < C(token) an exact sampler keeps."""
    tokens = np.asarray(tokens, dtype=np.int64)
    us = np.asarray(us, dtype=np.float64)
    inside = (tokens >= 0) & (tokens < cdf.shape[0])
    t = np.where(inside, tokens, 0)
    lo = np.where(t > 0, cdf[np.maximum(t - 1, 0)], 0.0)
    hi = cdf[t]
    tgt = us * total
    ok = inside & support[t] & (lo - m * total <= tgt) & (tgt <= hi + m * total)
    exact = inside & support[t] & (lo <= tgt) & (tgt < hi)
    return ok, ok & ~exact


def decidable(us, support, cdf, total, m):
    """[N] bool: the target of the draw is farther than m * total from every CDF boundary between two support tokens, so exactly one token is accepted.
    (0 and total are no such boundary: beyond them there is no token to confuse the first or the last one with.)"""
    tgt = np.asarray(us, dtype=np.float64) * total
    bounds = np.concatenate([[-np.inf], np.unique(cdf[support])[:-1], [np.inf]])
    j = np.clip(np.searchsorted(bounds, tgt), 1, bounds.shape[0] - 1)
    return np.minimum(tgt - bounds[j - 1], bounds[j] - tgt) > m * total


def exact_token(u, support, cdf, total):
    """The token an exact inverse CDF returns: the first support token with C(token) > u * total."""
    idx = np.nonzero(support)[0]
    j = int(np.searchsorted(cdf[idx], u * total, side="right"))
    return int(idx[min(j, idx.shape[0] - 1)])
