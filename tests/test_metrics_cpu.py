"""CPU: the restatements the GPU tests grade the metric kernels against are sound (tests/metrics_ref.py), the inputs can tell a wrong kernel from a
right one, the size rule, and the arithmetic of the accumulators and of ControlConsistency's dispatch with a stub engine.  (That the header and the
symbol table agree on car_ms_ssim / car_f1 / car_rmse / car_pixels_to_u8 is test_abi_cpu.py's.)"""
import json
import os

import numpy as np
import pytest
import torch

from tests import metrics_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def measured():
    return json.load(open(os.path.join(GOLDEN, "metrics_measured.json")))


@pytest.fixture(scope="module")
def oracle():
    """the fp64 literal definition on the three small cases, once"""
    out = {}
    for name in ("min_176", "odd_181x203", "rgb_256x192"):
        p, t, sc = R.ms_inputs(name, "f32")
        out[name] = R.ms_ssim(p, t, sc)
    return out


def test_symbols_and_methods_exist():
    from controlar_amd import _lib as L
    from controlar_amd.engine import Engine
    lib = L.load()
    for name in ("car_ms_ssim", "car_f1", "car_rmse", "car_pixels_to_u8"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    for name in ("ms_ssim", "f1", "rmse", "pixels_to_u8"):
        assert callable(getattr(Engine, name))


def test_literal_definition_equals_the_valid_convolution(oracle):
    """The crop equals the padding, so no kept pixel's window touches the padding: the literal pad-and-crop definition and a plain valid convolution of
    the un-padded image are the same sums.  This is what lets the kernel run without reflect indexing."""
    for name, (val, tab) in oracle.items():
        p, t, sc = R.ms_inputs(name, "f32")
        v2, t2 = R.ms_ssim(p, t, sc, valid=True)
        # the same 121-term sums, possibly added in another order by the convolution that serves the other image size: one fp64 rounding (1.1e-16) of a
        # moment moves cs by at most 4 / c2 times as much, 5e-13; nothing larger is tolerated (six orders below the fp32-derived bound of the GPU tests)
        assert float((val - v2).abs().max()) <= 1e-12 and float((tab - t2).abs().max()) <= 1e-12, name


def test_identical_and_inverted_pairs():
    p, t, sc = R.ms_inputs("odd_181x203", "same")
    val, tab = R.ms_ssim(p, t, sc)
    assert torch.equal(val, torch.ones_like(val)) and torch.equal(tab, torch.ones_like(tab))
    p, t, sc = R.ms_inputs("odd_181x203", "inv")
    raw = R.ms_ssim(p, t, sc)[1]
    assert torch.equal(R.ms_ssim(p, t, sc)[0], torch.zeros(p.shape[0], dtype=torch.float64))
    assert bool((raw[:, :, 1] == 0).any())          # a contrast mean went negative and the relu caught it


def test_inputs_exercise_the_variance_clamp():
    """mostly exact zeros with a few soft curves: in fp32 E[p^2] - mu^2 rounds below zero somewhere, so a kernel without the clamp would differ"""
    p, t, _ = R.ms_inputs("min_176", "f32")
    assert float((t == 0).float().mean()) > 0.5
    g = R.gaussian(torch.float32)
    w = torch.outer(g, g)[None, None]
    mu, e2 = torch.nn.functional.conv2d(t, w), torch.nn.functional.conv2d(t * t, w)
    assert float((e2 - mu * mu).min()) < 0


def test_a_real_mistake_lies_far_outside_the_tolerance(oracle, measured):
    """The inputs must be able to tell a wrong kernel from a right one: a crop of 4, ceil-mode pooling (on the odd case) and sigma 1.4 each move the
    result by more than ten times the tolerance the GPU test allows (measured here: 100 x to 2500 x)."""
    tol = measured["ms_ssim"]["bound_result"]
    moved = {}
    for name, (val, _) in oracle.items():
        p, t, sc = R.ms_inputs(name, "f32")
        moved[name, "crop4"] = float((R.ms_ssim(p, t, sc, crop=4)[0] - val).abs().min())
        moved[name, "sigma1.4"] = float((R.ms_ssim(p, t, sc, sigma=1.4)[0] - val).abs().min())
        if name == "odd_181x203":
            moved[name, "ceil"] = float((R.ms_ssim(p, t, sc, ceil_mode=True)[0] - val).abs().min())
    print("METRICS_MISTAKES " + json.dumps({f"{k[0]}/{k[1]}": v for k, v in moved.items()}))
    assert all(v > 10 * tol for v in moved.values()), moved


def test_measured_file_states_its_bounds_as_16x_the_fp32_deviation(measured):
    m = measured["ms_ssim"]
    assert m["bound_result"] == 16 * m["fp32_vs_fp64_result"] and m["bound_scale_mean"] == 16 * m["fp32_vs_fp64_scale_mean"]
    assert measured["rmse"]["bound"] == 16 * measured["rmse"]["fp32_vs_fp64"]
    assert 0 < m["bound_result"] < 1e-4 and 0 < m["bound_scale_mean"] < 1e-4 and 0 < measured["rmse"]["bound"] < 1e-2


def test_size_rule_refuses_175_and_accepts_176():
    x = torch.rand(1, 1, 176, 176)
    assert R.ms_ssim(x, x)[0].shape == (1,)
    for shape in ((175, 176), (176, 175), (31, 400)):
        with pytest.raises(ValueError):
            R.ms_ssim(torch.rand(1, 1, *shape), torch.rand(1, 1, *shape))


def test_f1_restatement_equals_sklearn_in_both_orders():
    from sklearn.metrics import f1_score
    for kind, rule in (("u8", dict(value=255)), ("f32", dict(threshold=128))):
        a, b = R.binary_maps(3, 33, 40, seed=5, kind=kind)
        pa, pb = R.positive(a.numpy(), **rule), R.positive(b.numpy(), **rule)
        for x, y in ((pa, pb), (pb, pa)):
            cnt, f1 = R.f1_counts(x, y)
            for i in range(3):
                assert abs(f1[i] - f1_score(y[i].ravel().astype(int), x[i].ravel().astype(int))) <= 1e-12
            assert cnt.sum(1).max() <= 33 * 40
    z = np.zeros((1, 8, 8), dtype=bool)
    assert R.f1_counts(z, z)[1][0] == 0.0 and f1_score(z.ravel().astype(int), z.ravel().astype(int), zero_division=0) == 0.0


def test_pixel_quantiser_restatement_on_known_values():
    x = torch.tensor([-2.0, -1.0, -0.0, 0.0, 1.0, 3.0, 1 / 255.0, -1 + 1 / 255.0]).view(1, 1, 1, -1).expand(1, 3, 1, -1)
    assert R.pixels_to_u8(x)[0, 0, :, 0].tolist() == [0, 0, 128, 128, 255, 255, 128, 1]


# ------------------------------------------------------------------------------------------------ accumulators and dispatch, with a stub engine
class _StubEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def ms_ssim(self, a, b, scale=None, want_scales=False):
        self.calls.append(("ms_ssim", tuple(a.shape), a.dtype, scale))
        return a.double().mean(dim=(1, 2, 3)) if a.dim() == 4 else a.double().mean(dim=(1, 2))

    def f1(self, a, b, value=None, threshold=None, **kw):
        self.calls.append(("f1", tuple(a.shape), value, threshold))
        return a.double().mean(dim=(1, 2))

    def rmse(self, a, b, scale_to_max=False):
        self.calls.append(("rmse", tuple(a.shape), scale_to_max))
        return (a.double() - b.double()).pow(2).mean(dim=(1, 2)).sqrt()

    def pixels_to_u8(self, x, want_float=False):
        self.calls.append(("pixels_to_u8", tuple(x.shape), want_float))
        q = R.pixels_to_u8(x)
        return (q, q.permute(0, 3, 1, 2).float().contiguous()) if want_float else q

    def canny(self, x, lo, hi):
        self.calls.append(("canny", tuple(x.shape), lo, hi))
        return x[..., 0].contiguous()

    def hed(self, x):
        self.calls.append(("hed", tuple(x.shape)))
        return x[:, 0].contiguous()

    def lineart(self, x):
        self.calls.append(("lineart", tuple(x.shape)))
        return (x[:, :1] / 255).contiguous()


def test_accumulators_add_batch_means_and_count_batches():
    from controlar_amd import metrics as M
    eng = _StubEngine()
    acc = M.SSIM(engine=eng)
    with pytest.raises(ValueError):
        acc.calculate()
    a = torch.stack([torch.full((176, 176), 10.0), torch.full((176, 176), 30.0)])          # batch mean 20
    b = torch.full((1, 176, 176), 50.0)                                                      # batch mean 50
    acc.update(a, a); acc.update(b, b)
    assert acc.count == 2 and acc.calculate() == pytest.approx((20 + 50) / 2)               # the mean of batch means, as the scripts append ssim(batch)
    assert acc.per_image.tolist() == [10.0, 30.0, 50.0]
    assert eng.calls[0] == ("ms_ssim", (2, 176, 176), torch.float32, 1.0 / 255.0)
    f = M.F1score(engine=eng)
    f.update(np.full((4, 4), 200, dtype=np.uint8), np.full((4, 4), 100, dtype=np.uint8))    # metric.py's call: arrays [H,W]
    assert f.count == 1 and eng.calls[-1] == ("f1", (1, 4, 4), None, 128)
    r = M.RMSE(engine=eng)
    r.update(np.full((4, 4), 3.0, dtype=np.float32), np.zeros((4, 4), dtype=np.uint8))
    r.update(np.full((4, 4), 5.0, dtype=np.float32), np.zeros((4, 4), dtype=np.uint8))
    assert r.count == 2 and r.calculate() == pytest.approx(4.0)


def test_control_consistency_dispatch():
    from controlar_amd import metrics as M

    class _Ex:
        def __init__(self):
            self._eng = _StubEngine()

    g = torch.Generator().manual_seed(0)
    px, ctrl = torch.rand(2, 3, 16, 16, generator=g) * 2 - 1, torch.rand(2, 3, 16, 16, generator=g) * 2 - 1
    for kind, scorer, scale in (("canny", "f1", None), ("hed", "ms_ssim", (1 / 255.0, 1 / 255.0)), ("lineart", "ms_ssim", (1.0, 1 / 255.0))):
        ex = _Ex()
        vals, mean = M.ControlConsistency(kind, ex)(px, ctrl)
        names = [c[0] for c in ex._eng.calls]
        assert names == ["pixels_to_u8", kind, "pixels_to_u8", scorer], names
        assert vals.shape == (2,) and float(mean) == pytest.approx(float(vals.mean()))
        if kind == "canny":
            assert ex._eng.calls[1][2:] == (100, 200) and ex._eng.calls[-1][2:] == (255, None)
        else:
            assert ex._eng.calls[-1][3] == scale
    with pytest.raises(ValueError):
        M.ControlConsistency("seg", _Ex())
    with pytest.raises(ValueError):
        M.ControlConsistency("hed")
