"""GPU (pytest -m gpu): sample_stochastic_kernel and sample_greedy_kernel replayed draw by draw against tests/sampler_ref.py.

The sampler's draw is a function of (logits row, temperature, top_k, top_p, seed, counter word a, step): one Philox4x32-10 number inverts the CDF of the
filtered softmax.  The host reference computes the fp64 CDF of the same fp32 keys and the same number, and EVERY token must lie where that number
points, within the margin m that tests/sampler_ref.py derives from the kernel's fp32 summation (71 .. 165 units of 2^-24 of the total mass; never
measured on the kernel).  tests/test_sampler_cpu.py shows on the reference alone that each case is decidable: its filter boundaries are clear and at least
80 % of its draws accept exactly one token.

  a  the stream with no tolerance: a row of zeros makes every partial sum an exact integer, so token == floor(u * V)
  b  filter and draw at V in {256, 260, 1000, 4096, 16384, 16388}, 512 draws per parameter set
  c  threshold edges by support: ties around rank k, +-0, -inf rows, both signs, the pad-adjacent chunk — no tolerance
  d  the CFG mix inside the stochastic kernel, exact by construction, both entries, both sides of cfg_interval
  e  greedy: lowest index on ties across thread, wave and stride boundaries; NaN ignored; a row with no comparable logit gives token 0
  f  Engine.generate: every token of the loop replayed from the returned logits at the counter (image index or rng_stream, step)
Each replay test prints the share of draws that needed the margin."""
import numpy as np
import pytest
import torch

from tests import sampler_cases as K
from tests import sampler_ref as R
from tests.cases import load_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from controlar_amd.engine import Engine
    e = Engine(load_case("tiny_canny_cfg1")["cfg"], "bf16")
    yield e
    e.close()


def _tile(row, n):
    return torch.from_numpy(np.array(row)).cuda()[None].expand(n, row.shape[0]).contiguous()


def _draw(eng, c, lg):
    """The tokens of one case: the plain entry (a = step * 65536 + row) or the row entry (a = step * 65536 + rng_stream)."""
    kw = dict(temperature=c["T"], top_k=c["k"], top_p=c["p"], sample_logits=True, seed=c["seed"], step=c["step"])
    if c["entry"] == "rows":
        kw["rng_stream"] = c["streams"]
    return eng.sample(lg, **kw).cpu().numpy().astype(np.int64)


def _check_replay(c, toks, us=None):
    """Every draw of the case against the reference; returns (draws, draws that needed the margin)."""
    x, support, cdf, total, _, m = K.reference(c)
    us = R.uniforms(c["seed"], c["a"], 0) if us is None else us
    ok, needed = R.accepts_all(toks, us, support, cdf, total, m)
    bad = np.nonzero(~ok)[0]
    assert bad.size == 0, (c["name"], f"{bad.size} of {toks.shape[0]} draws rejected; first: draw {bad[0]} token {toks[bad[0]]} u {us[bad[0]]!r} "
                           f"exact token {R.exact_token(us[bad[0]], support, cdf, total)} m {m / R.EPS:.0f} x 2^-24")
    if c["argmax"]:
        assert (toks == int(np.argmax(x))).all(), c["name"]
    return toks.shape[0], int(needed.sum())


# ------------------------------------------------------------------------------------------------ a. the stream
SEEDS = (0, 42, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 5)                 # both key words count
STREAMS = (0, 1, 65535, 65536, 2 ** 31, 2 ** 32 - 1)


@pytest.mark.parametrize("V", [4096, 32768])
def test_stream_plain_entry_exact(eng, V):
    """A row of zeros: expf(0) = 1, every partial sum is an integer below 2^24, total = V and u * V is exact, so the token is floor(u * V) — the top 12
    (15) bits of the documented stream at counter (step * 65536 + row, 0), with no tolerance."""
    lg = torch.zeros(256, V, device="cuda")
    seen = {}
    for step in (0, 1, 7, 65535):
        for seed in SEEDS:
            got = eng.sample(lg, sample_logits=True, seed=seed, step=step).cpu().numpy().astype(np.int64)
            want = np.floor(R.uniforms(seed, [(step * 65536 + i) & R.M32 for i in range(256)], 0) * V).astype(np.int64)
            assert np.array_equal(got, want), (V, step, seed, np.nonzero(got != want)[0][:8], got[:4], want[:4])
            seen[(step, seed)] = tuple(got)
    assert len(set(seen.values())) == len(seen)                    # every (step, seed) is its own vector: the low and the high seed word, every step


@pytest.mark.parametrize("V", [4096, 32768])
def test_stream_row_entry_exact(eng, V):
    """A seed and a stream per row: counter (step * 65536 + rng_stream mod 2^32, 0) under the row's own key; nothing of the slot."""
    n = 256
    lg = torch.zeros(n, V, device="cuda")
    seeds = [(SEEDS[i % 5] + (i // 5) * 0x100000001) % 2 ** 64 for i in range(n)]
    streams = [STREAMS[i % 6] for i in range(n)]
    seeds[100], streams[100] = seeds[0], streams[0]               # equal (seed, stream, step) at two slots
    seeds[201], streams[201] = seeds[7], streams[7]

    def run(seeds, streams, step):
        got = eng.sample(lg, sample_logits=True, seed=seeds, step=step, rng_stream=streams).cpu().numpy().astype(np.int64)
        want = np.floor(R.uniforms(seeds, [(step * 65536 + s) & R.M32 for s in streams], 0) * V).astype(np.int64)
        assert np.array_equal(got, want), (V, step, np.nonzero(got != want)[0][:8])
        return got
    base = run(seeds, streams, 0)
    assert base[100] == base[0] and base[201] == base[7]
    assert not np.array_equal(run(seeds, streams, 7), base)                                              # the step
    assert not np.array_equal(run([s ^ (1 << 40) for s in seeds], streams, 0), base)                     # the seed (high word)
    assert not np.array_equal(run([s ^ 1 for s in seeds], streams, 0), base)                             # the seed (low word)
    assert not np.array_equal(run(seeds, [(s + 1) & R.M32 for s in streams], 0), base)                   # the stream


# ------------------------------------------------------------------------------------------------ b. filter and draw
@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("V", K.VS)
def test_replay_filter_and_draw(eng, V, kind):
    """512 draws of one logits row per parameter set (tests/sampler_cases.py: the shipped (1, 2000, 1), no filter, k in {1, 2, V - 1, V, V + 7}, (0.7, 20, 1),
    p in {1e-6, 0.5, 0.8, 0.999}, (1.3, 40, 0.9), (1, 2000, 0.95), T in {1e-6, 100}); every token where the stream points, within m."""
    n = needed = 0
    for c in K.replay_cases(V, kind):
        toks = _draw(eng, c, _tile(c["logits"], K.N_DRAWS))
        a, b = _check_replay(c, toks)
        n, needed = n + a, needed + b
    print(f"replay V={V} {kind}: {n} draws, {needed} needed the margin ({100.0 * needed / n:.3f} %)")


# ------------------------------------------------------------------------------------------------ c. threshold edges
EDGES = K.edge_cases()


@pytest.mark.parametrize("c", EDGES, ids=[c["name"] for c in EDGES])
def test_threshold_edges_by_support(eng, c):
    """4096 draws: every token of the expected support appears (the reference says which draws reach it: test_sampler_cpu.py), nothing else does."""
    toks = _draw(eng, c, _tile(c["logits"], K.N_EDGE))
    assert sorted(set(toks.tolist())) == c["want"], (c["name"], sorted(set(toks.tolist()) ^ set(c["want"]))[:16])


@pytest.mark.parametrize("V", [1000, 16384])
def test_nonpositive_top_p_keeps_the_argmax(eng, V):
    """Sorted position 0 never goes (the shift of the reference's nucleus filter), so top_p <= 0 keeps exactly the largest key.  The row entry rejects
    such a top_p; the plain entry passes it to the kernel, whose `a >= 1` this pins."""
    row = K.logits_row(V, "randn", 0)
    for p in (0.0, -1.0):
        toks = eng.sample(_tile(row, 64), sample_logits=True, top_p=p, seed=3, step=1).cpu().numpy()
        assert (toks == int(np.argmax(row))).all(), (V, p, toks[:8])


# ------------------------------------------------------------------------------------------------ d. CFG inside the stochastic kernel
@pytest.mark.parametrize("V", [260, 4096])
def test_replay_under_cfg(eng, V):
    """[cond | uncond] rows of multiples of 2^-6, scales 1.5 / 3 / 7.5: the mix is exact in fp32, so the replay sees the kernel's own row — mixed at step 3,
    the conditional row alone at step 12 (cfg_interval 5) — through the plain and the row entry."""
    n = needed = 0
    for c in K.cfg_cases(V):
        lg = torch.cat([_tile(c["cond"], K.N_DRAWS), _tile(c["uncond"], K.N_DRAWS)])
        for entry in ("plain", "rows"):
            kw = dict(cfg_scale=c["scale"], cfg_interval=K.CFG_INTERVAL, temperature=c["T"], top_k=c["k"], top_p=c["p"], sample_logits=True, seed=c["seed"],
                      step=c["step"])
            if entry == "rows":
                kw["rng_stream"] = c["streams"]
            toks = eng.sample(lg, **kw).cpu().numpy().astype(np.int64)
            a, b = _check_replay(c, toks, R.uniforms(c["seed"], K.cfg_counter(c, entry), 0))
            n, needed = n + a, needed + b
    print(f"replay under CFG V={V}: {n} draws, {needed} needed the margin ({100.0 * needed / n:.3f} %)")


# ------------------------------------------------------------------------------------------------ e. greedy
def _greedy_both(eng, row):
    """The greedy token of `row` from sample_greedy_kernel, and from a greedy row inside a stochastic launch (row 1 is stochastic)."""
    r = torch.from_numpy(row).cuda()
    a = int(eng.sample(r[None], sample_logits=False).cpu()[0])
    b = int(eng.sample(torch.stack([r, torch.zeros_like(r)]), sample_logits=[False, True], seed=[1, 2]).cpu()[0])
    return a, b


def _tie_row(V, at, seed):
    row = -np.abs(np.random.default_rng(seed).standard_normal(V)).astype(np.float32) - 0.5
    row[list(at)] = 1.0
    return row


@pytest.mark.parametrize("V,at", [(16384, (3, 4)), (16384, (255, 256)), (16384, (5, 4101)), (16384, (0, 16383)), (16384, (4095, 4096, 16383)),
                                  (260, (255, 256)), (260, (0, 259)), (4, (1, 2))])
def test_greedy_lowest_index_wins_a_tie(eng, V, at):
    """Thread (3 | 4), wave (255 | 256), stride (5 | 4101: one thread, two trips), first against last; V = 4 is one 64-thread block."""
    assert _greedy_both(eng, _tie_row(V, at, V + at[0])) == (min(at), min(at))


@pytest.mark.parametrize("V", [4, 260, 16384])
def test_greedy_ignores_nan_and_returns_token_0_without_a_comparable_logit(eng, V):
    row = _tie_row(V, (V - 2,), 7)
    row[[0, V - 1]] = np.nan
    assert _greedy_both(eng, row) == (V - 2, V - 2)                                 # a NaN beside finite values is ignored
    row = np.full(V, -np.inf, dtype=np.float32)
    row[V - 3] = -1e30
    assert _greedy_both(eng, row) == (V - 3, V - 3)                                 # one finite logit among -inf
    assert _greedy_both(eng, np.full(V, -np.inf, dtype=np.float32)) == (0, 0)       # no comparable logit: token 0, as the stochastic kernel returns
    assert _greedy_both(eng, np.full(V, np.nan, dtype=np.float32)) == (0, 0)
    # the stochastic kernel on the same rows (its own `t < 0` branch)
    for fill in (-np.inf, np.nan):
        t = eng.sample(torch.full((2, V), fill, device="cuda"), sample_logits=True, top_k=3, seed=5).cpu().tolist()
        assert t == [0, 0]


# ------------------------------------------------------------------------------------------------ f. the token loop
N_NEW = 64


def _gen_engine(prec):
    from controlar_amd.engine import Engine
    cs = load_case("tiny_depth_cfg4")
    e = Engine(cs["cfg"], prec)
    e.load_state_dict(cs["gsd"]); e.finalize()
    return cs, e


def _generate(cs, e, B, n_new, **kw):
    from controlar_amd import synth
    g = cs["cfg"].gpt
    img = synth.smooth_control(B, cs["H"], cs["W"])
    emb, mask = synth.text_embeddings(B, g.cls_token_num, g.caption_dim)
    e.encode_control(img.cuda())
    t, l = e.generate(emb.cuda(), n_new, mask.cuda(), sample_logits=True, return_logits=True, **kw)
    return t.cpu().numpy().astype(np.int64), l.cpu().numpy()


def _replay_loop(tag, toks, logits, seeds, words, T, k, p):
    """Device step numbering (engine_generate.hip): the (pos, step) scalars start at step = 0 for the sampler that follows the prefill, and every decode
    step advances them BEFORE its sampler runs.  So step 0 is the token drawn from the prompt's last row, out[:, 0], and token j of image i is drawn at
    the counter (words[i], j): words[i] = i, the image's index in the whole batch, for the plain call; the image's rng_stream for the row call.
    `logits` are the kernel's own rows after the CFG mix and before the temperature."""
    B, N, V = logits.shape
    n = needed = decided = 0
    for i in range(B):
        for j in range(N):
            x = R.keys32(logits[i, j], T)
            support, cdf, total, _ = R.filtered_support_and_cdf(x, k, p)
            m = R.margin(V)
            u = R.uniform(seeds[i], words[i], j)
            assert R.accepts(toks[i, j], u, cdf, total, m, support), (tag, i, j, int(toks[i, j]), u, R.exact_token(u, support, cdf, total), m / R.EPS)
            ok, need = R.accepts_all([toks[i, j]], [u], support, cdf, total, m)
            n, needed, decided = n + 1, needed + int(need[0]), decided + int(R.decidable([u], support, cdf, total, m)[0])
    print(f"token loop {tag}: {n} draws, {needed} needed the margin ({100.0 * needed / n:.3f} %), {100.0 * decided / n:.1f} % decidable")
    assert decided >= 0.8 * n                                                       # not vacuous: most draws accept exactly one token


@pytest.fixture(scope="module")
def gen32():
    cs, e = _gen_engine("fp32")
    yield cs, e
    e.close()


def test_token_loop_plain_counter_is_image_index_and_step(gen32):
    cs, e = gen32
    t, l = _generate(cs, e, 3, N_NEW, cfg_scale=1.0, temperature=0.9, top_k=20, seed=2 ** 40 + 9)
    assert e.stats()["graph_used"]
    _replay_loop("fp32 B=3 top_k 20 T 0.9", t, l, [2 ** 40 + 9] * 3, [0, 1, 2], 0.9, 20, 1.0)
    assert len({tuple(r) for r in t.tolist()}) == 3


def test_token_loop_under_cfg(gen32):
    cs, e = gen32
    t, l = _generate(cs, e, 3, N_NEW, cfg_scale=3.0, cfg_interval=20, temperature=0.9, top_k=20, seed=77)
    assert e.stats()["graph_used"]
    _replay_loop("fp32 B=3 cfg 3.0 interval 20", t, l, [77] * 3, [0, 1, 2], 0.9, 20, 1.0)


def test_token_loop_row_counter_is_rng_stream_and_step(gen32):
    """Streams (5, 5, 70000): images 0 and 1 share a stream under different seeds; image 2's stream is beyond 16 bits.  Nothing of the slot enters."""
    cs, e = gen32
    seeds, streams = [11, 2 ** 33 + 12, 13], [5, 5, 70000]
    t, l = _generate(cs, e, 3, N_NEW, cfg_scale=1.0, temperature=0.9, top_k=20, seed=seeds, rng_stream=streams)
    assert e.stats()["graph_used"]
    _replay_loop("fp32 B=3 row mode", t, l, seeds, streams, 0.9, 20, 1.0)


def test_token_loop_second_chain_draws_at_the_global_image_index():
    """bf16, 192 sequences: the engine cuts two chains of 96 by itself, and chain 1's sampler numbers its images from row0 = 96."""
    cs, e = _gen_engine("bf16")
    t, l = _generate(cs, e, 192, 8, cfg_scale=1.0, temperature=1.0, top_k=20, seed=5)
    assert e.stats()["graph_used"]
    _replay_loop("bf16 B=192 two chains", t, l, [5] * 192, list(range(192)), 1.0, 20, 1.0)
    e.close()
