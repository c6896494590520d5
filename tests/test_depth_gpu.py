"""car_depth on the GPU (pytest -m gpu) against the fixtures minted from transformers' DPTForDepthEstimation (tests/golden/make_depth_golden.py).

Tolerances come from the fixtures, per case: exact mode max|out - ref| <= 8 x the reference's own fp32-vs-fp64 deviation; fast mode max and mean deviation
<= 2 x those of the same model under .bfloat16() on the CPU.  Each case prints its measured figures as one DEPTH_PARITY JSON line (pytest -s) before it
asserts.  The control tensor is computed as 2*(d/max - 0.5) in fp32 with a correctly rounded division and rounded once: it is compared bit for bit."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"b2_32": "tiny_dpt", "b1_64": "tiny_dpt", "b1_96": "tiny_dpt", "b1_128": "tiny_dpt", "wide_b1_64": "tiny_dpt_wide"}
WEIGHT_SEED = 13


def _x(name):
    return torch.from_numpy(np.load(os.path.join(GOLDEN, f"depth_{name}.npz"))["x"])


def _pv(x):
    return (x.to(torch.float32) / 255 - 0.5) / 0.5


def _stream():
    return C.c_void_p(int(torch.cuda.current_stream().cuda_stream))


@pytest.fixture(scope="module")
def weights():
    from controlar_amd import config as Cfg, synth
    return {n: (getattr(Cfg, n)(), synth.dpt_state_dict(getattr(Cfg, n)(), WEIGHT_SEED)) for n in ("tiny_dpt", "tiny_dpt_wide")}


@pytest.fixture(scope="module")
def engines(weights):
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    e = {}
    for prec in ("fp32", "bf16"):
        for cn, (cfg, sd) in weights.items():
            e[prec, cn] = Engine(Cfg.tiny_t2i(), prec)
            e[prec, cn].load_depth(sd, cfg)
    yield e
    for v in e.values():
        v.close()


@pytest.fixture(scope="module")
def outputs(engines):
    """every case once per mode, with the control tensor: shared by the tests below and left unchanged"""
    res = {}
    for prec in ("fp32", "bf16"):
        for name, cn in CASES.items():
            out, ctrl = engines[prec, cn].depth(_pv(_x(name)), want_control=True)
            torch.cuda.synchronize()
            res[prec, name] = (out.cpu(), ctrl.cpu())
    return res


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_depth_matches_the_reference(outputs, prec, name):
    z = np.load(os.path.join(GOLDEN, f"depth_{name}.npz"))
    out = outputs[prec, name][0].numpy()
    assert out.shape == z["ref"].shape and out.dtype == np.float32
    d = np.abs(out.astype(np.float64) - z["ref"])
    rec = dict(case=name, mode=prec, max_abs=float(d.max()), mean_abs=float(d.mean()), ref_f32_vs_f64_max=float(z["ref_f32_vs_f64_max"]),
               bf16_native_max=float(z["bf16_native_max"]), bf16_native_mean=float(z["bf16_native_mean"]))
    print("DEPTH_PARITY " + json.dumps(rec))
    assert np.isfinite(out).all() and out.min() >= 0
    if prec == "fp32":
        assert d.max() <= 8 * float(z["ref_f32_vs_f64_max"]), rec
    else:
        assert d.max() <= 2 * float(z["bf16_native_max"]) and d.mean() <= 2 * float(z["bf16_native_mean"]), rec


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_control_output_is_the_scaled_map_on_three_channels(outputs, engines, prec):
    for name, cn in CASES.items():
        out, ctrl = outputs[prec, name]
        assert ctrl.dtype == engines[prec, cn].dtype and tuple(ctrl.shape) == (out.shape[0], 3) + tuple(out.shape[1:])
        want = (2 * (out / out.amax(dim=(1, 2), keepdim=True) - 0.5)).to(ctrl.dtype)
        for ch in range(3):
            assert torch.equal(ctrl[:, ch], want), (name, ch)                          # bit-equal: the same fp32 expression, rounded once
        assert float(ctrl.float().min()) >= -1 and float(ctrl.float().max()) == 1     # every image reaches its own maximum


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_second_call_and_control_only_call_give_the_same_bits(outputs, engines, prec):
    eng = engines[prec, "tiny_dpt"]
    for name in ("b1_96", "b2_32"):
        x = _x(name)
        again, ctrl = eng.depth(_pv(x), want_control=True)
        assert torch.equal(again.cpu(), outputs[prec, name][0]) and torch.equal(ctrl.cpu(), outputs[prec, name][1]), name
    # out = NULL: only the control tensor is written
    xg = _pv(x).cuda().contiguous()
    ctrl2 = torch.empty_like(ctrl)
    rc = eng.lib.car_depth(eng._h, C.c_void_p(xg.data_ptr()), 2, 32, 32, C.c_void_p(0), C.c_void_p(ctrl2.data_ptr()), _stream())
    assert rc == 0 and torch.equal(ctrl2.cpu(), outputs[prec, "b2_32"][1])
    # neither output: refused
    rc = eng.lib.car_depth(eng._h, C.c_void_p(xg.data_ptr()), 2, 32, 32, C.c_void_p(0), C.c_void_p(0), _stream())
    assert rc != 0


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_an_image_alone_equals_its_slice_of_the_batch(outputs, engines, prec):
    x = _x("b2_32")
    both, cboth = outputs[prec, "b2_32"]
    assert not torch.equal(both[0], both[1])
    for i in (1, 0):
        alone, calone = engines[prec, "tiny_dpt"].depth(_pv(x[i:i + 1]), want_control=True)
        assert torch.equal(alone.cpu()[0], both[i]) and torch.equal(calone.cpu()[0], cboth[i]), i


def test_an_all_zero_map_writes_minus_one(weights):
    """head.head.4.bias = -1000 clips every pixel at the final ReLU: the reference's 0/0 would be NaN, car_depth writes -1."""
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    cfg, sd = weights["tiny_dpt"]
    eng = Engine(Cfg.tiny_t2i(), "bf16")
    eng.load_depth(dict(sd, **{"head.head.4.bias": torch.full((1,), -1000.0)}), cfg)
    out, ctrl = eng.depth(_pv(_x("b2_32")), want_control=True)
    assert float(out.abs().max()) == 0 and bool((ctrl.float() == -1).all())
    eng.close()


def test_bad_shapes_missing_weights_and_foreign_configs_are_clean_errors(engines, weights):
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    eng = engines["bf16", "tiny_dpt"]
    for shape in ((48, 80), (64, 96), (32, 64)):
        with pytest.raises(RuntimeError, match="must be square"):
            eng.depth(torch.zeros(1, 3, *shape))
    for side in (48, 16, 0):
        with pytest.raises(RuntimeError, match="multiple of 32"):
            eng.depth(torch.zeros(1, 3, side, side))
    assert tuple(eng.depth(torch.zeros(1, 3, 32, 32)).shape) == (1, 32, 32)               # the boundary itself runs
    cfg, sd = weights["tiny_dpt"]
    bare = Engine(Cfg.tiny_t2i(), "bf16")
    with pytest.raises(RuntimeError, match="no DPT weights"):
        bare.depth(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="car_depth_configure before"):
        bare.load_state_dict({"depth.head.head.4.bias": torch.zeros(1)})
    part = {k: v for k, v in sd.items() if k != "neck.fusion_stage.layers.2.residual_layer1.convolution2.bias"}
    with pytest.raises(RuntimeError, match="depth.neck.fusion_stage.layers.2.residual_layer1.convolution2.bias"):
        bare.load_depth(part, cfg)                                                         # finalize names the missing tensor
    with pytest.raises(RuntimeError, match="depth.neck.convs.9.weight: not a tensor of the configured DPT"):
        bare.load_state_dict({"depth.neck.convs.9.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match=r"depth.neck.convs.1.weight: expected \[64,64,3,3\]"):
        bare.load_state_dict({"depth.neck.convs.1.weight": torch.zeros(64, 32, 3, 3)})
    bare.load_state_dict({"depth.dpt.layernorm.weight": torch.zeros(128), "depth.dpt.pooler.dense.weight": torch.zeros(128, 128)})   # accepted, ignored
    bare.close()
    # configs outside the family are refused at configure time, before any tensor is loaded
    other = Engine(Cfg.tiny_t2i(), "bf16")
    for kw in (dict(is_hybrid=True), dict(readout_type="add"), dict(use_batch_norm_in_fusion_residual=True)):
        with pytest.raises(ValueError, match="outside the supported family"):
            other.depth_configure(Cfg.DPTConfig(**kw))
    with pytest.raises(RuntimeError, match="64-wide-head"):                               # bf16: head dim 32 is outside the fused attention kernel
        other.depth_configure(Cfg.DPTConfig(hidden_size=128, num_attention_heads=4, num_hidden_layers=4, intermediate_size=512, image_size=64,
                                            backbone_out_indices=(0, 1, 2, 3), neck_hidden_sizes=(64, 64, 128, 128), fusion_hidden_size=64))
    with pytest.raises(RuntimeError, match="out_indices"):
        other.depth_configure(Cfg.DPTConfig(backbone_out_indices=(5, 11, 17, 24)))
    with pytest.raises(RuntimeError, match="neck_hidden"):
        other.depth_configure(Cfg.DPTConfig(neck_hidden_sizes=(48, 96, 192, 384)))
    other.close()


def test_packed_cache_round_trip_reproduces_the_bits(engines, outputs, weights, tmp_path):
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    path = str(tmp_path / "depth.carpk").encode()
    for prec in ("bf16", "fp32"):
        src = engines[prec, "tiny_dpt"]
        src._check(src.lib.car_export_packed(src._h, path), "car_export_packed")
        dst = Engine(Cfg.tiny_t2i(), prec)
        dst.depth_configure(weights["tiny_dpt"][0])
        dst._check(dst.lib.car_import_packed(dst._h, path), "car_import_packed")
        assert torch.equal(dst.depth(_pv(_x("b1_96"))).cpu(), outputs[prec, "b1_96"][0]), prec
        dst.close()


def test_depth_estimator_keeps_the_scripts_use(weights, outputs, engines, tmp_path):
    """condition.DepthEstimator as sample_t2i.py:114-116,133-139 uses the HF pair: from_pretrained(dir), .to(device), .eval(), model(pixel_values=...)."""
    from controlar_amd.condition import DepthEstimator
    cfg, sd = weights["tiny_dpt"]
    with open(tmp_path / "config.json", "w") as f:
        json.dump(dict(cfg.to_hf_dict(), model_type="dpt", architectures=["DPTForDepthEstimation"]), f)
    try:
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    except ImportError:
        torch.save(sd, str(tmp_path / "pytorch_model.bin"))
    model = DepthEstimator.from_pretrained(str(tmp_path)).to("cuda").eval()
    x = _x("b2_32")
    pv = DepthEstimator.preprocess(x)
    assert pv.dtype == torch.float32 and torch.equal(pv, _pv(x))
    y = model(pixel_values=pv).predicted_depth
    assert y.device == pv.device and y.dtype == torch.float32 and torch.equal(y, outputs["bf16", "b2_32"][0])
    yg = model(pixel_values=pv.cuda()).predicted_depth
    assert yg.is_cuda and torch.equal(yg.cpu(), engines["bf16", "tiny_dpt"].depth(pv).cpu())
    model._eng.close()
