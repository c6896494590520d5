"""CPU: the host reference of the stochastic sampler (tests/sampler_ref.py) is itself pinned, and every case of tests/test_sampler_gpu.py is shown to be
decidable on the reference alone — so that no GPU test can pass vacuously.

  - Philox4x32-10 against Random123's known answers; the vectorised stream against the scalar one.
  - The reference's support and probabilities against the oracle's top_k_top_p_filtering wherever the boundary values are distinct.
  - Per case: the k-th and (k+1)-th key more than 16 fp32 ulps apart (unless the case is a deliberate tie), the nucleus cut's cumulative probability at
    least 1e-4 from top_p, and at least 80 % of the draws with their target farther than m * total from every boundary between two tokens (those draws
    have exactly one accepted token)."""
import numpy as np
import pytest
import torch

from tests import sampler_cases as K
from tests import sampler_ref as R

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    assert R.philox4x32_10(counter, key) == want


def test_uniform_is_word0_top24_and_both_key_words_count():
    seed, a, b = 2 ** 63 + 5, 70000, 9
    w0 = R.philox4x32_10((a, b, 0x243F6A88, 0x85A308D3), (seed & R.M32, seed >> 32))[0]
    assert R.uniform(seed, a, b) == (w0 >> 8) / 16777216.0
    assert len({R.uniform(s, a, b) for s in (5, 2 ** 32 + 5, 2 ** 63 + 5)}) == 3
    assert R.uniform(seed, a, b) != R.uniform(seed, a, b + 1) != R.uniform(seed, a + 1, b)


def test_vectorised_stream_equals_the_scalar_one():
    seeds = [0, 42, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 5, 2 ** 64 - 1]
    a = [0, 1, 65535, 65536, 2 ** 31, 2 ** 32 - 1]
    for b in (0, 1, 7, 65535):
        got = R.uniforms(seeds, a, b)
        assert got.tolist() == [R.uniform(s, x, b) for s, x in zip(seeds, a)]
    got = R.uniforms(7, list(range(300)), 3)
    assert got.tolist() == [R.uniform(7, x, 3) for x in range(300)]


def test_margin_multiples():
    assert [round(R.margin(V) / R.EPS) for V in (256, 260, 1000, 4096, 16384, 16388, 32768)] == [71, 71, 73, 77, 115, 127, 165]


def test_accepts_and_exact_token_on_a_small_row():
    x = np.array([0.0, -np.inf, 0.0, 0.0], dtype=np.float32)
    support, cdf, total, _ = R.filtered_support_and_cdf(x, 0, 1.0)
    assert support.tolist() == [True, False, True, True] and cdf.tolist() == [1.0, 1.0, 2.0, 3.0] and total == 3.0
    assert [R.exact_token(u, support, cdf, total) for u in (0.0, 0.3, 1 / 3, 0.5, 0.99)] == [0, 0, 2, 2, 3]
    assert R.accepts(0, 0.3, cdf, total, 0.0) and not R.accepts(2, 0.3, cdf, total, 0.0) and R.accepts(2, 0.3, cdf, total, 0.04)
    assert not R.accepts(1, 1 / 3, cdf, total, 0.5, support) and not R.accepts(1, 1 / 3, cdf, total, 0.5) and not R.accepts(4, 0.5, cdf, total, 1.0)
    ok, needed = R.accepts_all([0, 2, 1, 2], [0.3, 0.3, 0.3, 0.5], support, cdf, total, 0.04)
    assert ok.tolist() == [True, True, False, True] and needed.tolist() == [False, True, False, False]
    assert R.decidable([0.01, 0.3, 0.5, 0.99], support, cdf, total, 0.04).tolist() == [True, False, True, True]      # the outer ends are no boundary


def _us(c):
    return R.uniforms(c["seed"], c["a"], 0)


ALL = list(K.all_cases())


def test_the_case_list_is_what_the_gpu_tests_promise():
    names = [c["name"] for c in ALL]
    assert len(set(names)) == len(names)
    for V in K.VS:
        for kind in K.KINDS:
            ps = K.param_sets(V, kind)
            assert (1.0, 0, 1.0) in ps and (0.7, 20, 1.0) in ps and (1.3, 40, 0.9) in ps and (1e-6, 0, 1.0) in ps and (1.0, 0, 1e-6) in ps and (1.0, 0, 0.5) in ps
            assert all((1.0, k, 1.0) in ps for k in (1, 2, V - 1, V, V + 7))
            assert ((1.0, 2000, 1.0) in ps) == (V >= 4096)
        assert {(1.0, 0, 0.8), (1.0, 0, 0.999), (1.0, 2000, 0.95)} <= set(K.param_sets(V, "peaked"))
    assert any(c["T"] == 100.0 for c in ALL)


@pytest.mark.parametrize("c", ALL, ids=[c["name"] for c in ALL])
def test_case_is_decidable_and_matches_the_oracle(c):
    from oracle import controlar_oracle as O
    x, support, cdf, total, info, m = K.reference(c)
    tie = c.get("tie", False)
    assert tie or info["ties"] == 0
    # boundary separations
    if info["kth"] is not None and info["next"] is not None and info["next"] > -np.inf and not tie:
        ulps = (info["kth"] - info["next"]) / float(np.spacing(np.float32(max(abs(info["kth"]), abs(info["next"])))))
        assert ulps > 16, ulps
    if info["cut_gap"] is not None:
        assert info["cut_gap"] >= 1e-4, info["cut_gap"]
    assert support.any() and total > 0
    # the oracle's filter where the boundary values are distinct (a deliberate tie is kept whole by the value threshold, and cut by the oracle's index rule
    # only in its nucleus branch)
    if not (tie and float(np.float32(c["p"])) < 1.0):
        xt = torch.from_numpy(x.astype(np.float64))[None]
        want = torch.softmax(O.top_k_top_p_filtering(xt, c["k"], float(np.float32(c["p"]))), dim=-1)[0].numpy()
        assert np.array_equal(want * total >= R.TINY, support), (np.nonzero(want > 0)[0][:20], np.nonzero(support)[0][:20])
        probs = np.diff(np.concatenate([[0.0], cdf])) / total
        assert np.abs(probs - want).max() <= 1e-12
    if "want" in c:
        assert np.nonzero(support)[0].tolist() == c["want"]
    # the draws
    us = _us(c)
    share = float(R.decidable(us, support, cdf, total, m).mean())
    print(f"{c['name']}: m = {m / R.EPS:.0f} x 2^-24, support {int(support.sum())}, decidable draws {100 * share:.1f} %")
    assert share >= 0.8, share
    exact = [R.exact_token(u, support, cdf, total) for u in us]
    ok, needed = R.accepts_all(exact, us, support, cdf, total, m)
    assert ok.all() and not needed.any()                                           # the exact inverse CDF is accepted without the margin
    if c["argmax"]:
        assert set(exact) == {int(np.argmax(x))} and int(support.sum()) == 1
    if c["kind"] == "edge":
        assert sorted(set(exact)) == c["want"]                                     # 4096 draws reach every token of the support


def test_nonpositive_top_p_keeps_the_argmax_in_reference_and_oracle():
    """Sorted position 0 always stays (the shift in the reference's nucleus filter): top_p <= 0 keeps exactly the largest key."""
    from oracle import controlar_oracle as O
    x = R.keys32(K.logits_row(1000, "randn", 0), 1.0)
    for p in (0.0, -1.0):
        support, _, _, _ = R.filtered_support_and_cdf(x, 0, p)
        assert np.nonzero(support)[0].tolist() == [int(np.argmax(x))]
        want = O.top_k_top_p_filtering(torch.from_numpy(x.astype(np.float64))[None], 0, p)[0].numpy()
        assert np.array_equal(np.isfinite(want), support)
