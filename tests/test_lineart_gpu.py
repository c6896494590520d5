"""car_lineart on the GPU (pytest -m gpu) against the fixtures minted from the reference's condition/lineart.py (tests/golden/make_lineart_golden.py).

Tolerances come from the fixtures, per case: exact mode max|out - ref| <= 8 x the reference's own fp32-vs-fp64 deviation; fast mode max and mean
deviation <= 2 x those of the reference with every conv's input and weight rounded to bf16.  Each case prints its measured figures as one LINEART_PARITY JSON line (pytest -s) before it asserts."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["b2_16x24", "b1_30x44", "b1_8x8", "b1_72x104"]
WEIGHT_SEED = 11


@pytest.fixture(scope="module")
def weights():
    from controlar_amd import synth
    return synth.lineart_state_dict(WEIGHT_SEED)


@pytest.fixture(scope="module")
def engines(weights):
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    e = {}
    for prec in ("fp32", "bf16"):
        e[prec] = Engine(Cfg.tiny_t2i(), prec)
        e[prec].load_lineart(weights)
    yield e
    for v in e.values():
        v.close()


@pytest.fixture(scope="module")
def outputs(engines):
    """every case once per mode, with the control tensor: shared by the tests below and left unchanged"""
    res = {}
    for prec, eng in engines.items():
        for name in CASES:
            z = np.load(os.path.join(GOLDEN, f"lineart_{name}.npz"))
            out, ctrl = eng.lineart(torch.from_numpy(z["x"]), want_control=True)
            torch.cuda.synchronize()
            res[prec, name] = (out.cpu(), ctrl.cpu())
    return res


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_lineart_matches_the_reference(outputs, prec, name):
    z = np.load(os.path.join(GOLDEN, f"lineart_{name}.npz"))
    out = outputs[prec, name][0].numpy()
    assert out.shape == z["ref"].shape and out.dtype == np.float32
    d = np.abs(out.astype(np.float64) - z["ref"])
    rec = dict(case=name, mode=prec, max_abs=float(d.max()), mean_abs=float(d.mean()), ref_f32_vs_f64_max=float(z["ref_f32_vs_f64_max"]),
               bf16_emul_max=float(z["bf16_emul_max"]), bf16_emul_mean=float(z["bf16_emul_mean"]))
    print("LINEART_PARITY " + json.dumps(rec))
    assert np.isfinite(out).all() and out.min() > 0 and out.max() < 1
    if prec == "fp32":
        assert d.max() <= 8 * float(z["ref_f32_vs_f64_max"]), rec
    else:
        assert d.max() <= 2 * float(z["bf16_emul_max"]) and d.mean() <= 2 * float(z["bf16_emul_mean"]), rec


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_control_output_is_one_minus_two_out_on_three_channels(outputs, engines, prec):
    for name in CASES:
        out, ctrl = outputs[prec, name]
        assert ctrl.dtype == engines[prec].dtype and tuple(ctrl.shape) == (out.shape[0], 3) + tuple(out.shape[2:])
        want = (1 - 2 * out[:, 0]).to(ctrl.dtype)
        for ch in range(3):
            assert torch.equal(ctrl[:, ch], want), (name, ch)
        assert float(ctrl.float().min()) >= -1 and float(ctrl.float().max()) <= 1


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_second_call_and_control_only_call_give_the_same_bits(outputs, engines, prec):
    eng = engines[prec]
    for name in ("b1_72x104", "b2_16x24"):
        x = torch.from_numpy(np.load(os.path.join(GOLDEN, f"lineart_{name}.npz"))["x"])
        again, ctrl = eng.lineart(x, want_control=True)
        assert torch.equal(again.cpu(), outputs[prec, name][0]) and torch.equal(ctrl.cpu(), outputs[prec, name][1]), name
    # out = NULL: only the control tensor is written
    xg = x.cuda().contiguous()
    ctrl2 = torch.empty_like(ctrl)
    rc = eng.lib.car_lineart(eng._h, C.c_void_p(xg.data_ptr()), 2, 16, 24, C.c_void_p(0), C.c_void_p(ctrl2.data_ptr()), C.c_void_p(int(torch.cuda.current_stream().cuda_stream)))
    assert rc == 0 and torch.equal(ctrl2.cpu(), outputs[prec, "b2_16x24"][1])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_an_image_alone_equals_its_slice_of_the_batch(outputs, engines, prec):
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, "lineart_b2_16x24.npz"))["x"])
    both = outputs[prec, "b2_16x24"][0]
    assert not torch.equal(both[0], both[1])
    for i in (1, 0):
        alone = engines[prec].lineart(x[i:i + 1]).cpu()
        assert torch.equal(alone[0], both[i]), i


def test_undersized_image_and_missing_weights_are_clean_errors(engines, weights):
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    eng = engines["bf16"]
    for shape in ((4, 4), (4, 16), (16, 4)):
        with pytest.raises(RuntimeError, match="at least 5 x 5"):
            eng.lineart(torch.zeros(1, 3, *shape))
    assert tuple(eng.lineart(torch.zeros(1, 3, 5, 5)).shape) == (1, 1, 8, 8)          # the boundary itself runs
    bare = Engine(Cfg.tiny_t2i(), "bf16")
    with pytest.raises(RuntimeError, match="no LineArt weights"):
        bare.lineart(torch.zeros(1, 3, 16, 16))
    part = {k: v for k, v in weights.items() if k != "model2.1.conv_block.5.bias"}
    with pytest.raises(RuntimeError, match="lineart.model2.1.conv_block.5.bias"):
        bare.load_lineart(part)                                                        # finalize names the missing tensor
    with pytest.raises(RuntimeError, match="not a tensor of the LineArt generator"):
        bare.load_state_dict({"lineart.model9.weight": torch.zeros(1)})
    bare.close()


def test_lineart_class_keeps_the_reference_use(weights, outputs):
    """condition.LineArt as sample_t2i.py:110-113,129-132 uses the reference's: construct, load_state_dict, .to(device), call on a (B,3,H,W) tensor."""
    from controlar_amd.condition import LineArt
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, "lineart_b2_16x24.npz"))["x"])
    net = LineArt()
    net.load_state_dict(weights)
    y = net.to("cuda").eval()(x)
    assert y.device == x.device and torch.equal(y, outputs["bf16", "b2_16x24"][0])
    net._eng.close()


def test_packed_cache_round_trip_reproduces_the_bits(engines, outputs, tmp_path):
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    path = str(tmp_path / "lineart.carpk").encode()
    for prec in ("bf16", "fp32"):
        src = engines[prec]
        src._check(src.lib.car_export_packed(src._h, path), "car_export_packed")
        dst = Engine(Cfg.tiny_t2i(), prec)
        dst._check(dst.lib.car_import_packed(dst._h, path), "car_import_packed")
        x = torch.from_numpy(np.load(os.path.join(GOLDEN, "lineart_b1_30x44.npz"))["x"])
        assert torch.equal(dst.lineart(x).cpu(), outputs[prec, "b1_30x44"][0]), prec
        dst.close()
