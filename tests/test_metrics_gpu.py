"""car_ms_ssim, car_f1, car_rmse, car_pixels_to_u8 and controlar_amd.metrics on the GPU (pytest -m gpu) against the restatements of tests/metrics_ref.py.

Tolerances are read from tests/golden/metrics_measured.json: 16 x the largest deviation of the fp32 CPU restatement from the fp64 one over exactly the
inputs used here (tests/golden/make_metrics_measured.py) — for MS-SSIM one bound for the result and one for a per-scale mean, for RMSE one absolute
bound.  The fp64 restatement is the oracle; it is computed once per case and shared.  F1 counts and the pixel quantiser are exact.  Each comparison
prints what the GPU reached as one METRICS_MEASURED JSON line (pytest -s) before it asserts."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import metrics_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MS_PARAMS = [(name, form) for name, *_ in R.MS_CASES for form in R.MS_FORMS[name]]


def _stream():
    return C.c_void_p(int(torch.cuda.current_stream().cuda_stream))


@pytest.fixture(scope="module")
def measured():
    return json.load(open(os.path.join(GOLDEN, "metrics_measured.json")))


@pytest.fixture(scope="module")
def eng():
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    e = Engine(Cfg.tiny_t2i(), "bf16")          # the metric kernels need no weights: any context serves
    yield e
    e.close()


@pytest.fixture(scope="module")
def ms(eng):
    """every case once: the inputs, the fp64 oracle and the kernel's result with its per-scale table; shared and left unchanged"""
    out = {}
    for name, form in MS_PARAMS:
        p, t, sc = R.ms_inputs(name, form)
        val, tab = eng.ms_ssim(p.cuda(), t.cuda(), scale=sc, want_scales=True)
        torch.cuda.synchronize()
        out[name, form] = dict(p=p, t=t, scale=sc, ref=R.ms_ssim(p, t, sc), got=(val.cpu(), tab.cpu()))
    return out


@pytest.mark.parametrize("name,form", MS_PARAMS)
def test_ms_ssim_matches_the_fp64_definition(ms, measured, name, form):
    c = ms[name, form]
    (val, tab), (rv, rt) = c["got"], c["ref"]
    assert val.dtype == torch.float64 and tuple(val.shape) == (c["p"].shape[0],) and tuple(tab.shape) == (c["p"].shape[0], 5, 2)
    dv, dt = float((val - rv).abs().max()), float((tab - rt).abs().max())
    rec = dict(what="ms_ssim", case=name, form=form, result=dv, scale_mean=dt, bound_result=measured["ms_ssim"]["bound_result"],
               bound_scale_mean=measured["ms_ssim"]["bound_scale_mean"], value=[float(v) for v in val[:3]])
    print("METRICS_MEASURED " + json.dumps(rec))
    assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(tab).all())
    assert dv <= measured["ms_ssim"]["bound_result"], rec
    assert dt <= measured["ms_ssim"]["bound_scale_mean"], rec            # the per-scale table is held to its own bound
    if form == "same":
        assert float((val - 1).abs().max()) <= measured["ms_ssim"]["bound_result"]
    if form == "inv":
        assert torch.equal(val, torch.zeros_like(val))                    # a negative mean, relu, and 0 ** beta = 0


def test_default_scale_follows_the_dtype(eng, ms):
    c = ms["min_176", "u8"]
    got = eng.ms_ssim((c["p"] / 255).cuda(), c["t"].cuda())              # float: 1, uint8: 1/255
    want = eng.ms_ssim((c["p"] / 255).cuda(), c["t"].cuda(), scale=(1.0, 1.0 / 255.0))
    assert torch.equal(got, want)
    assert torch.equal(eng.ms_ssim(c["p"][:, 0].cuda(), c["t"][:, 0].cuda(), scale=c["scale"]).cpu(), c["got"][0])      # [B,H,W] is one channel


def test_refused_sizes_name_the_limit_and_leave_the_context_usable(eng, ms):
    c = ms["min_176", "f32"]
    x = torch.rand(1, 1, 176, 176, device="cuda")
    out = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
    for H, W in ((175, 176), (176, 175), (20, 400)):
        rc = eng.lib.car_ms_ssim(eng._h, C.c_void_p(x.data_ptr()), 0, C.c_void_p(x.data_ptr()), 0, 1, 1, H, W, 1.0, 1.0, C.c_void_p(out.data_ptr()), None, _stream())
        msg = eng.lib.car_last_error(eng._h).decode()
        assert rc != 0 and "176" in msg and f"{H} x {W}" in msg, msg
        with pytest.raises(ValueError, match="176|32"):
            eng.ms_ssim(torch.rand(1, 1, H, W), torch.rand(1, 1, H, W))
    rc = eng.lib.car_ms_ssim(eng._h, C.c_void_p(x.data_ptr()), 1, C.c_void_p(x.data_ptr()), 0, 1, 1, 176, 176, 1.0, 1.0, C.c_void_p(out.data_ptr()), None, _stream())
    assert rc != 0 and "dtype" in eng.lib.car_last_error(eng._h).decode()             # bf16 is not a metric input
    with pytest.raises(ValueError):
        eng.ms_ssim(torch.rand(1, 1, 176, 176), torch.rand(1, 1, 176, 180))
    torch.cuda.synchronize()
    assert float(out[0]) == -7.0                                                          # a refused call writes nothing
    assert torch.equal(eng.ms_ssim(c["p"].cuda(), c["t"].cuda(), scale=c["scale"]).cpu(), c["got"][0])      # the context works on
    eng.check_errors()


def test_ms_ssim_is_deterministic_batch_invariant_and_stream_agnostic(eng, ms):
    c = ms["rgb_256x192", "f32"]
    p, t = c["p"].cuda(), c["t"].cuda()
    val, tab = eng.ms_ssim(p, t, scale=c["scale"], want_scales=True)
    assert torch.equal(val.cpu(), c["got"][0]) and torch.equal(tab.cpu(), c["got"][1])       # a second call: the same bits
    eng.ms_ssim(ms["odd_181x203", "f32"]["p"].cuda(), ms["odd_181x203", "f32"]["t"].cuda())     # another shape in between reuses the workspace
    for i in range(p.shape[0]):                                                                # an image alone = its slice of the batch of 3
        v1, t1 = eng.ms_ssim(p[i:i + 1], t[i:i + 1], scale=c["scale"], want_scales=True)
        assert torch.equal(v1.cpu(), c["got"][0][i:i + 1]) and torch.equal(t1.cpu(), c["got"][1][i:i + 1]), i
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        v2, t2 = eng.ms_ssim(p, t, scale=c["scale"], want_scales=True)
    s.synchronize()
    assert torch.equal(v2.cpu(), c["got"][0]) and torch.equal(t2.cpu(), c["got"][1])


# ------------------------------------------------------------------------------------------------ F1
@pytest.mark.parametrize("H,W", [(33, 40), (512, 512)])
@pytest.mark.parametrize("kind,rule", [("u8", dict(value=255)), ("f32", dict(threshold=128))])
def test_f1_counts_are_exact_and_f1_equals_sklearn(eng, H, W, kind, rule):
    from sklearn.metrics import f1_score
    a, b = R.binary_maps(3, H, W, seed=H + W, kind=kind)
    a[2], b[2] = 0, 0                                                          # an all-negative pair: F1 = 0
    pa, pb = R.positive(a.numpy(), **rule), R.positive(b.numpy(), **rule)
    for (x, y), (px, py) in (((a, b), (pa, pb)), ((b, a), (pb, pa))):
        f1, cnt = eng.f1(x.cuda(), y.cuda(), want_counts=True, **rule)
        want_cnt, want_f1 = R.f1_counts(px, py)
        assert cnt.dtype == torch.int64 and np.array_equal(cnt.cpu().numpy(), want_cnt)
        assert f1.dtype == torch.float64 and float(f1[2]) == 0.0
        for i in range(3):
            sk = f1_score(py[i].ravel().astype(int), px[i].ravel().astype(int), zero_division=0)
            assert abs(float(f1[i]) - sk) <= 1e-12 and abs(want_f1[i] - sk) <= 1e-12, (i, float(f1[i]), sk)
    one = eng.f1(a[0].cuda(), b[0].cuda(), **rule)                              # [H,W] in, a scalar out, the same bits
    assert one.dim() == 0 and float(one) == float(eng.f1(a.cuda(), b.cuda(), **rule)[0])


def test_f1_mixed_rules_and_dtypes(eng):
    """canny_f1score.py's '== 255' on a uint8 map against metric.py's '> 128' on a float one"""
    a, _ = R.binary_maps(2, 33, 40, seed=3, kind="u8")
    _, b = R.binary_maps(2, 33, 40, seed=3, kind="f32")
    f1, cnt = eng.f1(a.cuda(), b.cuda(), value=255, target_threshold=128, want_counts=True)
    want_cnt, want_f1 = R.f1_counts(R.positive(a.numpy(), value=255), R.positive(b.numpy(), threshold=128))
    assert np.array_equal(cnt.cpu().numpy(), want_cnt) and np.abs(f1.cpu().numpy() - want_f1).max() <= 1e-12
    with pytest.raises(ValueError):
        eng.f1(a, b)                                                           # no rule
    with pytest.raises(ValueError):
        eng.f1(a, b, value=255, threshold=128)                                 # two rules


# ------------------------------------------------------------------------------------------------ RMSE
@pytest.mark.parametrize("H,W,scale_to_max", R.RMSE_CASES)
def test_rmse_matches_fp64(eng, measured, H, W, scale_to_max):
    pred, label = R.rmse_inputs(H, W, scale_to_max)
    want = R.rmse(pred, label, scale_to_max)
    got = eng.rmse(pred.cuda(), label.cuda(), scale_to_max=scale_to_max).cpu()
    got_f = eng.rmse(pred.cuda(), label.float().cuda(), scale_to_max=scale_to_max).cpu()          # a float label: the same values, the same bits
    d = float((got - want).abs().max())
    print("METRICS_MEASURED " + json.dumps(dict(what="rmse", case=f"{H}x{W}/{'max' if scale_to_max else 'plain'}", abs=d, bound=measured["rmse"]["bound"],
                                                value=[float(v) for v in got])))
    assert got.dtype == torch.float64 and tuple(got.shape) == (3,) and torch.equal(got, got_f)
    assert d <= measured["rmse"]["bound"]
    assert torch.equal(eng.rmse(pred[1:2].cuda(), label[1:2].cuda(), scale_to_max=scale_to_max).cpu(), got[1:2])      # per image: batch-invariant
    assert float(eng.rmse(pred[0].cuda(), label[0].cuda(), scale_to_max=scale_to_max)) == float(got[0])


# ------------------------------------------------------------------------------------------------ the pixel quantiser
def test_pixels_to_u8_is_bit_equal_to_the_torch_expression(eng):
    g = torch.Generator().manual_seed(21)
    B, H, W = 2, 37, 53
    x = torch.randn(B, 3, H, W, generator=g) * 0.8                                             # a good share beyond +-1
    k = torch.arange(256, dtype=torch.float32)
    halves = (k + 0.5) / 255 * 2 - 1                                                          # pixel values that land on or next to an exact half
    special = torch.cat([halves, torch.nextafter(halves, torch.tensor(2.0)), torch.nextafter(halves, torch.tensor(-2.0)), k / 255 * 2 - 1,
                         torch.tensor([0.0, -0.0, 1.0, -1.0, 1.5, -1.5, 1e30, -1e30, float("inf"), float("-inf"), 1e-40, -1e-40])])
    x.view(-1)[:special.numel()] = special
    want = R.pixels_to_u8(x)
    u8, fl = eng.pixels_to_u8(x.cuda(), want_float=True)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (B, H, W, 3) and torch.equal(u8.cpu(), want)
    assert fl.dtype == torch.float32 and torch.equal(fl.cpu(), want.permute(0, 3, 1, 2).float())
    assert torch.equal(eng.pixels_to_u8(x.cuda()).cpu(), want)
    with pytest.raises(ValueError):
        eng.pixels_to_u8(torch.zeros(1, 1, 8, 8))


# ------------------------------------------------------------------------------------------------ accumulators and ControlConsistency, end to end
def test_accumulators_on_the_device(eng, ms, measured):
    from controlar_amd import metrics as M
    c = ms["min_176", "u8"]
    acc = M.SSIM(engine=eng)
    acc.update(c["p"], c["t"]); acc.update(c["p"][:1], c["t"][:1])                              # raw 0..255 maps, as metric.py's callers pass them
    want = (float(c["ref"][0].mean()) + float(c["ref"][0][0])) / 2
    assert acc.count == 2 and abs(acc.calculate() - want) <= measured["ms_ssim"]["bound_result"] and acc.per_image.shape == (3,)
    a, b = R.binary_maps(2, 33, 40, seed=9, kind="f32")
    f = M.F1score(engine=eng)
    f.update(a[0].numpy(), b[0].numpy()); f.update(a[1].numpy(), b[1].numpy())
    assert abs(f.calculate() - R.f1_counts(R.positive(b.numpy(), threshold=128), R.positive(a.numpy(), threshold=128))[1].mean()) <= 1e-12
    pred, label = R.rmse_inputs(64, 64, False)
    r = M.RMSE(engine=eng)
    r.update(pred.numpy(), label.numpy())
    assert abs(r.calculate() - float(R.rmse(pred, label).mean())) <= measured["rmse"]["bound"]


def _pixels(B, H, W, seed):
    """blocky colour patches under a soft gradient, in [-1.2, 1.2]: edges for Canny, structure for HED / LineArt / DPT, and values to clamp"""
    g = torch.Generator().manual_seed(seed)
    blocks = torch.nn.functional.interpolate(torch.rand(B, 3, (H + 15) // 16, (W + 15) // 16, generator=g), size=(H, W), mode="nearest")
    ramp = torch.nn.functional.interpolate(torch.rand(B, 3, 3, 3, generator=g), size=(H, W), mode="bilinear", align_corners=True)
    return ((0.7 * blocks + 0.3 * ramp) * 2.4 - 1.2).contiguous()


def test_control_consistency_canny(eng):
    from controlar_amd import condition, metrics as M, synth
    det = condition.CannyDetector()
    cc = M.ControlConsistency("canny", det)
    B, H, W = 2, 128, 97
    px, ctrl = _pixels(B, H, W, 31), synth.canny_like_control(B, H, W, seed=5)
    vals, mean = cc(px.cuda(), ctrl.cuda())
    q = R.pixels_to_u8(px)
    edges = np.stack([det(q[i].numpy()) for i in range(B)])                                 # the detector's own public call, image by image
    assert edges.any() and np.array_equal(cc.extract(px.cuda()).cpu().numpy(), edges)
    label = R.pixels_to_u8(ctrl)[..., 0].numpy()
    want = R.f1_counts(edges == 255, label == 255)[1]
    assert vals.is_cuda and vals.dtype == torch.float64 and np.abs(vals.cpu().numpy() - want).max() <= 1e-12
    assert abs(float(mean) - want.mean()) <= 1e-12
    # the image's own edge map as the control: the re-extracted map is the label, F1 = 1
    own = eng.canny(eng.pixels_to_u8(px.cuda()), 100, 200, want_control=True)[1].float()
    assert torch.equal(cc(px.cuda(), own)[0].cpu(), torch.ones(B, dtype=torch.float64))
    assert torch.equal(M.ControlConsistency("canny")(px.cuda(), own)[0].cpu(), torch.ones(B, dtype=torch.float64))      # the default extractor


@pytest.mark.parametrize("kind", ["hed", "lineart"])
def test_control_consistency_hed_and_lineart(measured, kind):
    from controlar_amd import condition, metrics as M, synth
    if kind == "hed":
        det = condition.HEDdetector(precision="fp32").load_state_dict(synth.hed_state_dict())
    else:
        det = condition.LineArt(precision="fp32").load_state_dict(synth.lineart_state_dict())
    B, H, W = 2, 176, 176
    px = _pixels(B, H, W, 41)
    # the control: the map of a disturbed copy of the image, so that the score lies strictly between 0 and 1 (an unrelated control scores 0 after the relu)
    near = (px + 0.15 * torch.randn(px.shape, generator=torch.Generator().manual_seed(8))).clamp(-1, 1)
    m = det(R.pixels_to_u8(near).permute(0, 3, 1, 2).float().contiguous().cuda()).cpu()
    m = (m[:, None] / 255 if kind == "hed" else m).clamp(0, 1)
    ctrl = (2 * m - 1).expand(B, 3, H, W).contiguous()
    vals, mean = M.ControlConsistency(kind, det)(px.cuda(), ctrl.cuda())
    assert bool(((vals > 0.01) & (vals < 0.999)).all()), vals
    x = R.pixels_to_u8(px).permute(0, 3, 1, 2).float().contiguous()                          # raw 0..255, as the scripts hand the PNG to the model
    out = det(x.cuda()).cpu()                                                                  # the extractor's own public call
    label = R.pixels_to_u8(ctrl)[..., 0][:, None]
    if kind == "hed":
        want = R.ms_ssim(out[:, None], label, (1 / 255.0, 1 / 255.0))[0]
    else:
        want = R.ms_ssim(out, label, (1.0, 1 / 255.0))[0]
    d = float((vals.cpu() - want).abs().max())
    print("METRICS_MEASURED " + json.dumps(dict(what="consistency", case=kind, result=d, value=[float(v) for v in vals])))
    assert d <= measured["ms_ssim"]["bound_result"] and abs(float(mean) - float(want.mean())) <= measured["ms_ssim"]["bound_result"]


def test_control_consistency_depth(measured):
    from controlar_amd import condition, config as Cfg, metrics as M, synth
    cfg = Cfg.tiny_dpt()
    est = condition.DepthEstimator(cfg, synth.dpt_state_dict(cfg), precision="fp32")
    S = 32                                                                                     # the smallest square car_depth accepts
    B = 2
    px, ctrl = _pixels(B, 48, 40, 51), synth.smooth_control(B, S, S, seed=9)
    vals, mean = M.ControlConsistency("depth", est, depth_size=(S, S))(px.cuda(), ctrl.cuda())
    q = R.pixels_to_u8(px).permute(0, 3, 1, 2)
    d = est(pixel_values=est.preprocess(q.cuda(), size=(S, S))).predicted_depth.cpu()         # the processor's resize and the model's own public call
    want = R.rmse(d, R.pixels_to_u8(ctrl)[..., 0], True)
    dev = float((vals.cpu() - want).abs().max())
    print("METRICS_MEASURED " + json.dumps(dict(what="consistency", case="depth", abs=dev, value=[float(v) for v in vals])))
    assert dev <= measured["rmse"]["bound"] and abs(float(mean) - float(want.mean())) <= measured["rmse"]["bound"]
    with pytest.raises(ValueError):
        M.ControlConsistency("depth", est, depth_size=(S, S))(px.cuda(), synth.smooth_control(B, 64, 64).cuda())      # a label of another size
