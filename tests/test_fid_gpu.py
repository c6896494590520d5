"""car_fid_accumulate / car_fid_finalize, car_manifold_radii / car_manifold_pr, car_debug_pairwise_distances and car_inception_score on the GPU
(pytest -m gpu) against the numpy restatement tests/fid_ref.py.

Where the arithmetic is exact (dyadic features) everything is required bit for bit; on generic features the distances are held to the bound derived in
DESIGN.md §6k, the moments to their fp64 bound against an np.longdouble truth, the Inception Score to 16 x the deviation of the script's literal fp32
arithmetic from fp64 (tests/golden/fid_measured.json).  Each tolerance case prints its figures as one FID_PARITY JSON line (pytest -s) before it asserts.
metrics.frechet_distance is host code and is not called here."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fid_ref as R      # noqa: E402

RB, CB, K = R.ROW_BATCH, R.COL_BATCH, R.K_DEFAULT
SCALED = slice(100, 111)


@pytest.fixture(scope="module")
def eng():
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    e = Engine(Cfg.tiny_t2i(), "bf16")
    yield e
    e.close()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _np(t):
    return t.cpu().numpy()


def _parity(**kw):
    print("FID_PARITY " + json.dumps(kw))


def _gpu_pr(eng, f1, f2, rb=RB, cb=CB):
    a, b = _dev(f1), _dev(f2)
    r1, r2 = eng.manifold_radii(a, K, rb, cb), eng.manifold_radii(b, K, rb, cb)
    s1, s2, pr = eng.manifold_pr(a, r1, b, r2, rb, cb)
    return _np(r1), _np(r2), _np(s1).astype(bool), _np(s2).astype(bool), _np(pr)


@pytest.fixture(scope="module")
def dyadic_ref():
    """the restatement on the dyadic sets, once: (f1, f2, r1, r2, s1, s2, pr, fallen blocks of set 1) per (D, scaled)"""
    res = {}
    for D in R.DIMS:
        for scaled in (False, True):
            f1, f2 = R.dyadic_sets(D, scaled_rows=SCALED if scaled else None)
            r1, fell = R.manifold_radii(f1, K, RB, CB, want_fallback=True)
            r2 = R.manifold_radii(f2, K, RB, CB)
            s1, s2, pr = R.evaluate_pr(f1, r1, f2, r2, RB, CB)
            res[(D, scaled)] = (f1, f2, r1, r2, s1, s2, pr, fell)
    return res


# ----------------------------------------------------------------------------------------------- 1. dyadic features: bit equality
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("D", R.DIMS)
def test_dyadic_bit_equal(eng, dyadic_ref, D, scaled):
    f1, f2, r1, r2, s1, s2, pr, fell = dyadic_ref[(D, scaled)]
    g1, g2, t1, t2, gpr = _gpu_pr(eng, f1, f2)
    assert np.array_equal(g1, r1) and np.array_equal(g2, r2)
    assert np.array_equal(t1, s1) and np.array_equal(t2, s2)
    assert gpr[0] == pr[0] and gpr[1] == pr[1]
    assert 0.1 < pr[0] < 0.9 and 0.1 < pr[1] < 0.9                      # not a trivial case
    # every (row batch, column batch) block of set 1 against itself: the distances and which arithmetic produced them
    for (r0, c0), used in fell.items():
        u, v = f1[r0:r0 + RB], f1[c0:c0 + CB]
        d, flag = eng.debug_pairwise_distances(_dev(u), _dev(v))
        ref, ref_used = R.block_distances(u, v)
        assert ref_used == used and int(flag.item()) == int(used), (r0, c0)
        assert np.array_equal(_np(d), ref), (r0, c0)
    want = {(r0, c0) for (r0, c0) in fell if scaled and (r0 <= SCALED.start < r0 + RB or c0 < SCALED.stop and SCALED.start < c0 + CB)}
    assert {b for b, u in fell.items() if u} == want                    # exactly the blocks that hold the scaled rows fall back


# ----------------------------------------------------------------------------------------------- 2. generic features: the derived bound
GENERIC = [(D, s, R.N1, R.N2) for D in R.DIMS for s in (0.05, 0.4, 3.0)] + [(2048, 0.4, 64, 64)]


@pytest.mark.parametrize("D,scale,n,m", GENERIC)
def test_generic_distances_within_bound(eng, D, scale, n, m):
    u, v = R.generic_sets(D, scale, n, m)
    d, flag = eng.debug_pairwise_distances(_dev(u), _dev(v))
    bound, ref = R.distance_bound(u, v)
    err = np.abs(_np(d).astype(np.float64) - ref)
    _parity(test="distances", D=D, scale=scale, n=n, m=m, max_err=float(err.max()), max_err_over_bound=float((err / bound).max()))
    assert int(flag.item()) == 0
    assert (err <= bound).all()


# ----------------------------------------------------------------------------------------------- 3. precision and recall with a margin
@pytest.mark.parametrize("D", R.DIMS)
def test_pr_with_margin(eng, D):
    f1, f2, recall = R.margin_sets(D)
    _, _, s1, s2, pr = _gpu_pr(eng, f1, f2)
    assert pr[0] == 0.5 and pr[1] == recall
    assert s2[:R.N2 // 2].all() and not s2[R.N2 // 2:].any()
    assert s1[:65].all() and not s1[65:].any()


# ----------------------------------------------------------------------------------------------- 4. invariance, bit for bit
def test_invariance(eng):
    D = 71
    f1, f2 = R.generic_sets(D, 0.4)
    base = _gpu_pr(eng, f1, f2)
    for other in (_gpu_pr(eng, f1, f2, 10000, 10000), _gpu_pr(eng, f1, f2)):          # one block; a second call
        for x, y in zip(base, other):
            assert np.array_equal(x, y)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        other = _gpu_pr(eng, f1, f2)
    st.synchronize()
    for x, y in zip(base, other):
        assert np.array_equal(x, y)
    # the same set in reversed row order: every row keeps its radius and its status
    ra = eng.manifold_radii(_dev(f1[::-1]), K, RB, CB)
    assert np.array_equal(_np(ra)[::-1], base[0])
    s1, s2, pr = eng.manifold_pr(_dev(f1[::-1]), _dev(base[0][::-1]), _dev(f2), _dev(base[1]), RB, CB)
    assert np.array_equal(_np(s1).astype(bool)[::-1], base[2]) and np.array_equal(_np(s2).astype(bool), base[3]) and np.array_equal(_np(pr), base[4])


# ----------------------------------------------------------------------------------------------- 5. moments
UPDATES = (128, 128, 44)


def _run_moments(eng, x, cuts):
    D = x.shape[1]
    st = eng.fid_state(D)
    i = 0
    for n in cuts:
        eng.fid_accumulate(st, _dev(x[i:i + n]))
        i += n
    assert i == len(x)
    return st


def _ref_moments(x, cuts):
    m = R.Moments(x.shape[1])
    i = 0
    for n in cuts:
        m.update(x[i:i + n])
        i += n
    return m


@pytest.mark.parametrize("cuts", [UPDATES, (1, 128, 127, 44)])
@pytest.mark.parametrize("D", R.DIMS)
def test_moments_dyadic_state_exact(eng, D, cuts):
    x = np.concatenate([*R.dyadic_sets(D), R.dyadic_sets(D, seed=1)[0]])[:sum(cuts)]
    x[0] = x[1]                                   # with a single first row c is that row: still dyadic
    st = _np(_run_moments(eng, x, cuts))
    assert np.array_equal(st, _ref_moments(x, cuts).state())
    again = _np(_run_moments(eng, x, cuts))
    assert np.array_equal(st.view(np.int64), again.view(np.int64))


@pytest.mark.parametrize("cuts", [UPDATES, (1, 128, 127, 44)])
@pytest.mark.parametrize("D", R.DIMS)
def test_moments_generic_within_bound(eng, D, cuts):
    x = np.concatenate(R.generic_sets(D, 0.4, 200, 100))
    x = x + np.float32(1.5)                       # a mean well away from 0
    st = _run_moments(eng, x, cuts)
    mu, sigma = (_np(t) for t in eng.fid_finalize(st, D))
    m = _ref_moments(x, cuts)
    tmu, tsig = m.finalize()
    bmu, bsig = m.bound([x])
    emu, esig = np.abs(mu - tmu).astype(np.float64), np.abs(sigma - tsig).astype(np.float64)
    _parity(test="moments", D=D, cuts=list(cuts), mu_err_over_bound=float((emu / bmu).max()), sigma_err_over_bound=float((esig / bsig).max()),
            sigma_max_err=float(esig.max()))
    assert (emu <= bmu).all() and (esig <= bsig).all()
    assert np.array_equal(sigma, sigma.T)


def test_moments_single_row_refused(eng):
    st = eng.fid_state(71)
    eng.fid_accumulate(st, _dev(R.generic_sets(71, 0.4)[0][:1]))
    with pytest.raises(RuntimeError, match="car_fid_finalize: .*at least 2"):
        eng.fid_finalize(st, 71)
    with pytest.raises(RuntimeError, match="car_fid_finalize: .*at least 2"):
        eng.fid_finalize(eng.fid_state(71), 71)
    eng.fid_accumulate(st, _dev(R.generic_sets(71, 0.4)[0][1:2]))          # the context and the state stay usable
    mu, sigma = eng.fid_finalize(st, 71)
    assert torch.isfinite(sigma).all()


# ----------------------------------------------------------------------------------------------- 6. Inception Score
def test_inception_score(eng):
    measured = json.load(open(os.path.join(ROOT, "tests", "golden", "fid_measured.json")))["inception_score"]
    acts, w = R.is_inputs()
    out = _np(eng.inception_score(_dev(acts), _dev(w), R.IS_SPLIT))
    score, splits = R.inception_score(acts, w, R.IS_SPLIT, np.float64)
    assert out.shape == (4,) and splits.shape == (3,)
    tol = measured["tolerance_factor"] * measured["fp32_vs_fp64_max_abs"]
    err = max(abs(out[0] - score), float(np.abs(out[1:] - splits).max()))
    _parity(test="inception_score", err=err, tol=tol, score=float(out[0]))
    assert score == measured["score_fp64"]
    assert err <= tol
    assert out[0] == np.mean(out[1:])


def test_inception_score_zero_probability_is_nan(eng):
    acts, w = R.is_inputs()
    acts = acts.copy()
    acts[60] *= 400.0                             # a logit gap far above 104: exp underflows to exactly 0, 0 * log 0 is NaN, as in the script
    z = acts[60].astype(np.float64) @ w.astype(np.float64)
    assert z.max() - z.min() > 104
    out = _np(eng.inception_score(_dev(acts), _dev(w), R.IS_SPLIT))
    score, splits = R.inception_score(acts, w, R.IS_SPLIT, np.float32)
    assert np.isnan(score) and np.isnan(splits[1]) and not np.isnan(splits[0])
    assert np.isnan(out[0]) and np.isnan(out[2]) and np.isfinite(out[1]) and np.isfinite(out[3])


# ----------------------------------------------------------------------------------------------- 7. refusals
def test_refusals(eng):
    f = _dev(R.generic_sets(71, 0.4)[0])
    with pytest.raises(RuntimeError, match="car_manifold_radii: .*k \\+ 1 <= N"):
        eng.manifold_radii(f[:3], 3)
    with pytest.raises(RuntimeError, match="car_manifold_radii: .*row_batch and col_batch must be positive"):
        eng.manifold_radii(f, 3, 0, 48)
    with pytest.raises(RuntimeError, match="car_manifold_pr: .*row_batch and col_batch must be positive"):
        eng.manifold_pr(f, torch.ones(150), f, torch.ones(150), 64, 0)
    import ctypes as C
    out = torch.empty(150, dtype=torch.float32, device="cuda")
    assert eng.lib.car_manifold_radii(eng._h, C.c_void_p(f.data_ptr()), 150, 0, 3, 64, 48, C.c_void_p(out.data_ptr()), None) != 0
    assert b"car_manifold_radii: D must be in" in eng.lib.car_last_error(eng._h)
    assert eng.lib.car_fid_state_bytes(0) == 0
    st = eng.fid_state(4)
    assert eng.lib.car_fid_accumulate(eng._h, C.c_void_p(f.data_ptr()), 10, 0, C.c_void_p(st.data_ptr()), None) != 0
    assert b"car_fid_accumulate: D must be in" in eng.lib.car_last_error(eng._h)
    assert eng.manifold_radii(f, 3, 64, 48).shape == (150,)              # a refused call leaves the context usable
