"""The inputs of tests/test_sampler_gpu.py, built on the host from numpy alone, so that tests/test_sampler_cpu.py can show on the reference that every one of
them is decidable before any kernel runs.  A row whose filter boundary would sit too close to call (k-th and (k+1)-th key within 16 fp32 ulps, a cumulative
probability within 1e-4 of top_p) is not used: the builder takes the first row seed 0, 1, 2, ... whose boundaries are clear — a property of the row and
the parameters alone, judged by tests/sampler_ref.py."""
import functools
import math

import numpy as np

from tests import sampler_ref as R

VS = (256, 260, 1000, 4096, 16384, 16388)      # 260, 1000, 16388: Vp > V, the -inf pad keys; 16388: Vp = 32768, the largest LDS request
KINDS = ("randn", "negative", "peaked")
N_DRAWS = 512
N_EDGE = 4096
LN3 = math.log(3.0)


@functools.lru_cache(maxsize=None)
def logits_row(V, kind, s):
    rng = np.random.default_rng([V, KINDS.index(kind), s])
    base = rng.standard_normal(V) * 2.0
    if kind == "negative":
        base = base - 30.0
    if kind == "peaked":      # twelve tokens whose probabilities fall by 3 per rank (cumulative 1 - 3^-(r+1)) over a background 28 below the top
        base = base - 25.0
        at = rng.choice(V, 12, replace=False)
        base[at] = 3.0 - LN3 * np.arange(12)
    row = base.astype(np.float32)
    row.setflags(write=False)
    return row


def param_sets(V, kind):
    """(temperature, top_k, top_p) of part b for one vocabulary and row kind.  Left out, by the density of the row alone: on the two randn rows a nucleus
    cut deep in the tail (p = 0.999 anywhere; p = 0.8 and (2000, 0.95) from V = 4096 up), where neighbouring cumulative probabilities lie closer than 1e-4
    to each other and NO row is decidable — the peaked row carries those; T = 100 above V = 4096, where a near-uniform draw over 16384 tokens leaves each
    token narrower than five margins."""
    ps = []
    if V >= 4096:
        ps.append((1.0, 2000, 1.0))                                        # the shipped one
    ps.append((1.0, 0, 1.0))
    ps += [(1.0, k, 1.0) for k in (1, 2, V - 1, V, V + 7)]                 # radix select
    ps.append((0.7, 20, 1.0))
    ps += [(1.0, 0, p) for p in (1e-6, 0.5, 0.8, 0.999)]                   # sort
    ps += [(1.3, 40, 0.9), (1.0, 2000, 0.95)]                              # both filters
    ps.append((1e-6, 0, 1.0))
    if V <= 4096:
        ps.append((100.0, 0, 1.0))
    if kind != "peaked":
        ps = [q for q in ps if q[2] != 0.999 and not (V >= 4096 and q[2] in (0.8, 0.95))]
    return ps


def boundaries_clear(x32, info, tie=False, T=1.0):
    if T <= 1e-5:      # greedy in effect: the runner-up's term must vanish in fp32 (e^-200 against expf's zero below e^-104)
        top = np.sort(x32.astype(np.float64))[-2:]
        if top[1] - top[0] <= 200.0:
            return False
    if info["ties"] and not tie:
        return False
    if info["kth"] is not None and info["next"] is not None and not tie:
        if info["next"] > -np.inf and info["kth"] - info["next"] <= 16 * float(np.spacing(np.float32(max(abs(info["kth"]), abs(info["next"]))))):
            return False
    return info["cut_gap"] is None or info["cut_gap"] >= 1e-4


def reference(case):
    """(x32, support, cdf, total, info, m) of a case: the keys, sampler_ref's filter, the margin."""
    x = R.keys32(case["logits"], case["T"])
    support, cdf, total, info = R.filtered_support_and_cdf(x, case["k"], case["p"])
    return x, support, cdf, total, info, R.margin(case["V"])


def _decided_row(V, kind, T, k, p):
    for s in range(64):
        row = logits_row(V, kind, s)
        x = R.keys32(row, T)
        _, _, _, info = R.filtered_support_and_cdf(x, k, p)
        if boundaries_clear(x, info, T=T):
            return row, s
    raise AssertionError(f"no decidable {kind} row at V={V} for (T={T}, k={k}, p={p})")


@functools.lru_cache(maxsize=None)
def replay_cases(V, kind):
    """Part b.  The randn row goes through the plain entry (counter word a = step * 65536 + row), the other two through the row entry with a stream per row."""
    out = []
    for n, (T, k, p) in enumerate(param_sets(V, kind)):
        row, s = _decided_row(V, kind, T, k, p)
        c = dict(name=f"V{V}-{kind}-T{T:g}-k{k}-p{p:g}", V=V, kind=kind, T=T, k=k, p=p, logits=row, row_seed=s, seed=1234567 + 1000 * n + V, step=n % 5,
                 entry="plain" if kind == "randn" else "rows", argmax=(k == 1 or p == 1e-6 or T == 1e-6))
        c["streams"] = None if c["entry"] == "plain" else [(77 + 3 * i + 65521 * n) & R.M32 for i in range(N_DRAWS)]
        c["a"] = [(c["step"] * 65536 + (i if c["streams"] is None else c["streams"][i])) & R.M32 for i in range(N_DRAWS)]
        out.append(c)
    return out


def _edge(name, V, vals, k, p, seed, tie=True):
    """An edge row: `vals` {index: value} over a background of distinct values far below (-40 - j / 8: no mass, never at rank k)."""
    row = (-40.0 - np.arange(V) / 8.0).astype(np.float32)
    for j, v in vals.items():
        row[j] = v
    c = dict(name=name, V=V, kind="edge", T=1.0, k=k, p=p, logits=row, seed=seed, step=2, entry="rows", tie=tie, argmax=False)
    c["streams"] = [(5 + 7 * i) & R.M32 for i in range(N_EDGE)]
    c["a"] = [(c["step"] * 65536 + s) & R.M32 for s in c["streams"]]
    return c


@functools.lru_cache(maxsize=None)
def edge_cases():
    """Part c.  Every case: 4096 draws of one row, the expected support known by construction (`want`), its tokens of comparable probability."""
    out = []
    ninf = -np.inf
    for p in (1.0, 0.999):      # the select path and the sort path
        tag = "select" if p == 1.0 else "sort"
        # the 6th largest value five times, at ranks 4..8, across a thread, a wave and a stride boundary of the select's loop: all five stay
        c = _edge(f"tie5-{tag}", 1000, {10: 1.0, 700: 0.75, 3: 0.5, 63: 0.25, 64: 0.25, 255: 0.25, 256: 0.25, 999: 0.25, 500: 0.0}, 6, p, 11)
        c["want"] = [3, 10, 63, 64, 255, 256, 700, 999]
        out.append(c)
        # +0.0 and -0.0 around rank k: the select orders -0 below +0, the comparison with the threshold must not
        for k in (5, 6):
            c = _edge(f"zeros-k{k}-{tag}", 260, {7: 1.0, 100: 0.75, 259: 0.5, 0: 0.0, 64: -0.0, 130: 0.0, 258: -0.0, 200: -0.25}, k, p, 12 + k)
            c["want"] = [0, 7, 64, 100, 130, 258, 259]
            out.append(c)
        # only ten finite logits and k = 50: the 50th value is -inf, and no -inf token is ever drawn
        fin = {1: 0.5, 63: 0.25, 64: 0.0, 300: -0.25, 511: 0.5, 512: 0.25, 777: 0.0, 900: -0.5, 998: 0.125, 999: -0.125}
        c = _edge(f"ten-finite-{tag}", 1000, fin, 50, p, 14)
        c["logits"][[j for j in range(1000) if j not in fin]] = ninf
        c["want"] = sorted(fin)
        out.append(c)
        # keys of both signs around rank k
        for k in (4, 5):
            c = _edge(f"signs-k{k}-{tag}", 4096, {9: 0.5, 1024: 0.25, 4095: 0.125, 2048: -0.125, 77: -0.25, 3000: -0.5}, k, p, 15 + k, tie=False)
            c["want"] = sorted([9, 1024, 4095, 2048, 77][:k])
            out.append(c)
    # rank k in the last chunk, next to the pad keys: V = 260, k = 259; the one token that goes is the row's minimum at 258, the k-th value sits at 259
    rng = np.random.default_rng(260259)
    vals = {j: float(v) for j, v in enumerate(rng.permutation(258) / 256.0 + 0.25)}
    vals[259], vals[258] = 0.125, 0.0
    c = _edge("pad-adjacent-k259", 260, vals, 259, 1.0, 21, tie=False)
    c["want"] = [j for j in range(260) if j != 258]
    out.append(c)
    for c in out:
        c["logits"].setflags(write=False)
    return out


CFG_SCALES = (1.5, 3.0, 7.5)
CFG_INTERVAL = 5
CFG_STEPS = (3, 12)      # step - 1 = 2 <= 5: mixed; step - 1 = 11 > 5: the conditional row alone
CFG_PARAMS = ((1.0, 0, 1.0), (1.0, 20, 1.0), (1.3, 40, 0.9))


@functools.lru_cache(maxsize=None)
def cfg_cases(V):
    """Part d.  cond and uncond are multiples of 2^-6 in [-16, 16]; with scales 1.5, 3 and 7.5 the mix u + (c - u) * s is exact in fp32, fused or not:
    (c - u) * s is a multiple of 2^-7 below 2^8, and so is the sum.  `logits` is the row the sampler must see: the mix, or cond past the interval."""
    out = []
    for scale in CFG_SCALES:
        for step in CFG_STEPS:
            for n, (T, k, p) in enumerate(CFG_PARAMS):
                for s in range(64):
                    rng = np.random.default_rng([V, int(scale * 2), step, n, s])
                    u = np.clip(np.round(rng.standard_normal(V) * 2.0 * 64.0), -1024, 1024) / 64.0
                    c_ = np.clip(u + np.round(rng.standard_normal(V) * 32.0) / 64.0, -16.0, 16.0)
                    mixed = (u + (c_ - u) * scale) if step - 1 <= CFG_INTERVAL else c_
                    assert np.array_equal(mixed.astype(np.float32).astype(np.float64), mixed)
                    x = R.keys32(mixed, T)
                    _, _, _, info = R.filtered_support_and_cdf(x, k, p)
                    if boundaries_clear(x, info, T=T):
                        break
                else:
                    raise AssertionError("no decidable CFG row")
                c = dict(name=f"cfg-V{V}-s{scale:g}-step{step}-T{T:g}-k{k}-p{p:g}", V=V, kind="cfg", T=T, k=k, p=p, logits=mixed.astype(np.float32),
                         cond=c_.astype(np.float32), uncond=u.astype(np.float32), scale=scale, step=step, seed=99 + n, argmax=False)
                c["streams"] = [(31 + 5 * i) & R.M32 for i in range(N_DRAWS)]
                out.append(c)
    return out


def all_cases():
    """Every case whose draws are replayed with the margin (parts b and d) or checked by support (part c), as (case, counter words a, n draws)."""
    for V in VS:
        for kind in KINDS:
            for c in replay_cases(V, kind):
                yield c
    for c in edge_cases():
        yield c
    for V in (260, 4096):
        for c in cfg_cases(V):
            for entry in ("plain", "rows"):
                yield dict(c, name=c["name"] + "-" + entry, entry=entry, a=cfg_counter(c, entry))


def cfg_counter(c, entry):
    return [(c["step"] * 65536 + (i if entry == "plain" else c["streams"][i])) & R.M32 for i in range(N_DRAWS)]
