"""The host side of the sample-quality statistics (no GPU): metrics.frechet_distance against the unmodified FIDStatistics.frechet_distance of the
reference's evaluations/c2i/evaluator.py, the logic of the numpy restatement tests/fid_ref.py against a literal loop over the script's block structure,
the sensitivity of the fixtures to the deviations a kernel could hide, and the premises of the GPU tests (exactness of the dyadic fixtures, the margin
of the margin fixture, the derived bounds on the restatement itself, the committed measured tolerance)."""
import importlib.util
import json
import os
import sys
import types
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fid_ref as R      # noqa: E402

REF = os.environ.get("CONTROLAR_REFERENCE", "/root/reference")
RB, CB, K = R.ROW_BATCH, R.COL_BATCH, R.K_DEFAULT


# ----------------------------------------------------------------------------------------------- the Fréchet function
def _reference_evaluator():
    """evaluator.py as it is, with stub modules where it imports TensorFlow and requests at module level: FIDStatistics needs neither."""
    path = os.path.join(REF, "evaluations", "c2i", "evaluator.py")
    if not os.path.isfile(path):
        pytest.skip("the reference tree is absent")
    pytest.importorskip("scipy")
    stubs = {"tensorflow": types.ModuleType("tensorflow"), "tensorflow.compat": types.ModuleType("tensorflow.compat"),
             "tensorflow.compat.v1": types.ModuleType("tensorflow.compat.v1"), "requests": types.ModuleType("requests")}
    stubs["tensorflow"].compat = stubs["tensorflow.compat"]
    stubs["tensorflow.compat"].v1 = stubs["tensorflow.compat.v1"]
    if importlib.util.find_spec("tqdm") is None:
        stubs["tqdm"] = types.ModuleType("tqdm")
        stubs["tqdm.auto"] = types.ModuleType("tqdm.auto")
        stubs["tqdm.auto"].tqdm = lambda x, *a, **k: x
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location("reference_c2i_evaluator", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def _stats(n, D, seed, shift=0.0):
    rng = np.random.default_rng(seed)
    x = (np.maximum(rng.standard_normal((n, D)), 0) * 0.4 + shift).astype(np.float32)
    return np.mean(x, axis=0), np.cov(x, rowvar=False)


def _frechet_cases():
    nil = np.zeros((6, 6))
    nil[0, 1] = 1.0                                # sigma1 . I is nilpotent: it has no square root, sqrtm returns NaN, the eps retry is taken
    return {
        "full_rank": (_stats(200, 24, 1), _stats(220, 24, 2, 0.1), False),
        "singular_product": (_stats(10, 24, 3), _stats(12, 24, 4, 0.1), False),          # n < D
        "eps_retry": ((np.arange(6.0), nil), (np.ones(6), np.eye(6)), True),
    }


@pytest.mark.parametrize("case", ["full_rank", "singular_product", "eps_retry"])
def test_frechet_distance_is_the_reference(case):
    ev = _reference_evaluator()
    from controlar_amd.metrics import frechet_distance
    (mu1, s1), (mu2, s2), retry = _frechet_cases()[case]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        want = ev.FIDStatistics(mu1, s1).frechet_distance(ev.FIDStatistics(mu2, s2))
        n_ref = sum("singular product" in str(w.message) for w in rec)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = frechet_distance(mu1, s1, mu2, s2)
        n_got = sum("singular product" in str(w.message) for w in rec)
    assert n_ref == n_got == (1 if retry else 0)
    assert np.isfinite(want) and got == want


def test_frechet_distance_without_scipy(monkeypatch):
    from controlar_amd.metrics import frechet_distance
    monkeypatch.setitem(sys.modules, "scipy", None)
    with pytest.raises(ImportError, match="scipy"):
        frechet_distance(np.zeros(2), np.eye(2), np.zeros(2), np.eye(2))


# ----------------------------------------------------------------------------------------------- the restatement's logic against the script's loop
def _literal_radii(feats, k, row_batch, col_batch):
    """manifold_radii as the script walks it: a row batch's distances into one buffer, column batch by column batch, then a partition of its rows."""
    n = len(feats)
    radii = np.zeros(n)
    buf = np.zeros((row_batch, n))
    for b1 in range(0, n, row_batch):
        e1 = min(b1 + row_batch, n)
        for b2 in range(0, n, col_batch):
            e2 = min(b2 + col_batch, n)
            buf[0:e1 - b1, b2:e2] = R.exact_distances(feats[b1:e1], feats[b2:e2])[0]
        radii[b1:e1] = np.partition(buf[0:e1 - b1], np.arange(k + 1), axis=1)[:, k]
    return radii


def _literal_pr(f1, r1, f2, r2, row_batch, col_batch):
    s1, s2 = np.zeros(len(f1), bool), np.zeros(len(f2), bool)
    for b1 in range(0, len(f1), row_batch):
        for b2 in range(0, len(f2), col_batch):
            d = R.exact_distances(f1[b1:b1 + row_batch], f2[b2:b2 + col_batch])[0]
            for i in range(d.shape[0]):
                for j in range(d.shape[1]):
                    if d[i, j] <= r2[b2 + j]:
                        s1[b1 + i] = True
                    if d[i, j] <= r1[b1 + i]:
                        s2[b2 + j] = True
    return s1, s2, (np.mean(s2.astype(np.float64)), np.mean(s1.astype(np.float64)))


@pytest.mark.parametrize("blocks", [(RB, CB), (10000, 10000)])
def test_restatement_logic_is_the_scripts_loop(blocks):
    f1, f2 = R.generic_sets(71, 0.4, 90, 70)
    r1 = R.manifold_radii(f1, K, *blocks, dist=R.exact_distances)
    r2 = R.manifold_radii(f2, K, *blocks, dist=R.exact_distances)
    assert np.array_equal(r1, _literal_radii(f1, K, *blocks).astype(np.float32))
    assert np.array_equal(r2, _literal_radii(f2, K, *blocks).astype(np.float32))
    s1, s2, pr = R.evaluate_pr(f1, r1, f2, r2, *blocks, dist=R.exact_distances)
    l1, l2, lpr = _literal_pr(f1, r1, f2, r2, *blocks)
    assert np.array_equal(s1, l1) and np.array_equal(s2, l2) and pr == tuple(lpr)
    assert 0 < pr[0] < 1 or 0 < pr[1] < 1


# ----------------------------------------------------------------------------------------------- fixtures: exactness, sensitivity, margin
@pytest.mark.parametrize("D", R.DIMS)
def test_dyadic_fixture_is_exact_in_fp16(D):
    f1, f2 = R.dyadic_sets(D)
    for u, v in ((f1, f1), (f2, f2), (f1, f2)):
        assert (u * 4 == np.round(u * 4)).all() and u.min() >= 0 and u.max() <= 3.75
        d, used = R.block_distances(u, v)
        assert not used and np.array_equal(d.astype(np.float64), R.exact_distances(u, v)[0])
    # with rows scaled by 64 exactly the blocks that hold them fall back, and the fp32 arithmetic is exact there
    fs, _ = R.dyadic_sets(D, scaled_rows=slice(100, 111))
    _, fell = R.manifold_radii(fs, K, RB, CB, want_fallback=True)
    assert {b for b, u in fell.items() if u} == {(64, 0), (64, 48), (64, 96), (64, 144), (0, 96), (128, 96)}
    d, used = R.block_distances(fs[64:128], fs[96:144])
    assert used and np.array_equal(d.astype(np.float64), R.exact_distances(fs[64:128], fs[96:144])[0])


@pytest.mark.parametrize("D", R.DIMS)
def test_sensitivity(D):
    """each deviation a kernel could hide changes the result on the dyadic fixtures"""
    f1, f2 = R.dyadic_sets(D)
    r1, r2 = R.manifold_radii(f1, K, RB, CB), R.manifold_radii(f2, K, RB, CB)
    s1, s2, pr = R.evaluate_pr(f1, r1, f2, r2, RB, CB)
    t1, t2, prs = R.evaluate_pr(f1, r1, f2, r2, RB, CB, mutate="strict")                 # < instead of <=
    assert prs != pr and ((t1 != s1).any() or (t2 != s2).any())
    assert (R.manifold_radii(f1, K, RB, CB, mutate="kth") != r1).any()                   # index k - 1 instead of k
    # (nu + nv) - 2 mm instead of (nu - 2 mm) + nv: on the exact fixture no order can matter, so this one is shown on the heavy dyadic set, where the
    # defined order is still exact and nu + nv is not
    h = R.dyadic_heavy(D)
    good = R.pairwise_fp16(h, h)
    assert np.array_equal(good.astype(np.float64), R.exact_distances(h, h)[0])
    assert (R.pairwise_fp16(h, h, mutate="assoc") != good).any()
    assert (R.manifold_radii(h, K, RB, CB, mutate="assoc") != R.manifold_radii(h, K, RB, CB)).any()
    m = R.Moments(D)                                                                     # ddof 0
    m.update(f1)
    assert (m.finalize(ddof=0)[1] != m.finalize()[1]).any()


@pytest.mark.parametrize("D", R.DIMS)
def test_margin_fixture_decides_every_comparison(D):
    """every d <= r of the margin sets is decided by at least 4 x the distance bound, in fp64; precision and recall are the constructed values"""
    f1, f2, recall = R.margin_sets(D)
    e11, e22, e12 = (R.exact_distances(a, b)[0] for a, b in ((f1, f1), (f2, f2), (f1, f2)))
    b11, b22, b12 = (R.distance_bound(a, b)[0] for a, b in ((f1, f1), (f2, f2), (f1, f2)))
    for e, b in ((e11, b11), (e22, b22)):          # the radius itself: the 4th smallest is apart from its neighbours in the row
        order = np.argsort(e, axis=1)
        srt, sb = np.take_along_axis(e, order, 1), np.take_along_axis(b, order, 1)
        assert (srt[:, K + 1] - srt[:, K] >= 4 * np.maximum(sb[:, K + 1], sb[:, K])).all()
        assert (srt[:, K] - srt[:, K - 1] >= 4 * np.maximum(sb[:, K - 1], sb[:, K])).all()
    q1, q2 = np.sort(e11, 1)[:, K], np.sort(e22, 1)[:, K]
    assert (np.abs(e12 - q2[None, :]) >= 4 * b12).all() and (np.abs(e12 - q1[:, None]) >= 4 * b12).all()
    s1, s2, pr = R.evaluate_pr(f1, q1, f2, q2, RB, CB, dist=R.exact_distances)
    assert pr == (0.5, recall) and s2[:R.N2 // 2].all() and not s2[R.N2 // 2:].any()
    t1, t2, pr16 = R.evaluate_pr(f1, R.manifold_radii(f1, K, RB, CB), f2, R.manifold_radii(f2, K, RB, CB), RB, CB)
    assert pr16 == pr and np.array_equal(t1, s1) and np.array_equal(t2, s2)


# ----------------------------------------------------------------------------------------------- the bounds hold for the restatement itself
@pytest.mark.parametrize("D,scale,n,m", [(D, s, R.N1, R.N2) for D in R.DIMS for s in (0.05, 0.4, 3.0)] + [(2048, 0.4, 64, 64)])
def test_distance_bound_holds_for_the_restatement(D, scale, n, m):
    u, v = R.generic_sets(D, scale, n, m)
    bound, ref = R.distance_bound(u, v)
    d, used = R.block_distances(u, v)
    assert not used
    ratio = np.abs(d.astype(np.float64) - ref) / bound
    assert ratio.max() <= 0.6                      # measured 0.36 .. 0.57: the derivation has room, as a worst-case bound should


@pytest.mark.parametrize("D", R.DIMS)
def test_moment_bound_holds_for_numpy(D):
    """np.mean / np.cov on the same rows in fp64 stay within the bound the device is held to"""
    x = np.concatenate(R.generic_sets(D, 0.4, 200, 100)) + np.float32(1.5)
    m = R.Moments(D)
    for i, n in ((0, 128), (128, 128), (256, 44)):
        m.update(x[i:i + n])
    tmu, tsig = m.finalize()
    bmu, bsig = m.bound([x])
    x64 = x.astype(np.float64)
    assert (np.abs(np.mean(x64, axis=0) - tmu) <= bmu).all()
    assert (np.abs(np.cov(x64, rowvar=False) - tsig) <= bsig).all()
    assert np.array_equal(m.state()[0:1], [300.0]) and m.state().shape == (1 + 2 * D + D * D,)


def test_measured_tolerance_is_reproducible():
    spec = importlib.util.spec_from_file_location("make_fid_measured", os.path.join(ROOT, "tests", "golden", "make_fid_measured.py"))
    assert spec is not None
    committed = json.load(open(os.path.join(ROOT, "tests", "golden", "fid_measured.json")))["inception_score"]
    acts, w = R.is_inputs()
    s64, p64 = R.inception_score(acts, w, R.IS_SPLIT, np.float64)
    s32, p32 = R.inception_score(acts, w, R.IS_SPLIT, np.float32)
    assert s64 == pytest.approx(committed["score_fp64"], rel=1e-13)
    dev = max(abs(s32 - s64), float(np.max(np.abs(p32 - p64))))
    assert 0 < committed["fp32_vs_fp64_max_abs"] and dev <= 4 * committed["fp32_vs_fp64_max_abs"]      # BLAS builds differ in their fp32 order
    assert committed["tolerance_factor"] == 16 and len(committed["splits_fp64"]) == 3


def test_abi_lists_the_new_entries():
    from controlar_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "controlar_hip.h")).read()
    for name in ("car_fid_state_bytes", "car_fid_accumulate", "car_fid_finalize", "car_manifold_radii", "car_manifold_pr", "car_debug_pairwise_distances",
                 "car_inception_score"):
        assert name in _lib.SYMBOLS and name + "(" in hdr
