"""car_hed on the GPU (pytest -m gpu) against the fixtures minted from the reference's condition/hed.py (tests/golden/make_hed_golden.py).

Tolerances come from the fixtures, per case, on the 0..255 scale: exact mode max|out - ref| <= 8 x the reference's own fp32-vs-fp64 deviation; fast mode
max and mean deviation <= 2 x those of the reference with every conv's input and weight rounded to bf16.  Each case prints its measured figures as one
HED_PARITY JSON line (pytest -s) before it asserts."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["b2_16x24", "b1_17x31", "b1_35x50", "b1_72x104"]
WEIGHT_SEED = 11


def _x(name):
    return torch.from_numpy(np.load(os.path.join(GOLDEN, f"hed_{name}.npz"))["x"])


@pytest.fixture(scope="module")
def weights():
    from controlar_amd import synth
    return synth.hed_state_dict(WEIGHT_SEED)


@pytest.fixture(scope="module")
def engines(weights):
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    e = {}
    for prec in ("fp32", "bf16"):
        e[prec] = Engine(Cfg.tiny_t2i(), prec)
        e[prec].load_hed(weights)
    yield e
    for v in e.values():
        v.close()


@pytest.fixture(scope="module")
def outputs(engines):
    """every case once per mode, with the control tensor: shared by the tests below and left unchanged"""
    res = {}
    for prec, eng in engines.items():
        for name in CASES:
            out, ctrl = eng.hed(_x(name), want_control=True)
            torch.cuda.synchronize()
            res[prec, name] = (out.cpu(), ctrl.cpu())
    return res


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_hed_matches_the_reference(outputs, prec, name):
    z = np.load(os.path.join(GOLDEN, f"hed_{name}.npz"))
    out = outputs[prec, name][0].numpy()
    assert out.shape == z["ref"].shape and out.dtype == np.float32
    d = np.abs(out.astype(np.float64) - z["ref"])
    rec = dict(case=name, mode=prec, max_abs=float(d.max()), mean_abs=float(d.mean()), ref_f32_vs_f64_max=float(z["ref_f32_vs_f64_max"]),
               bf16_emul_max=float(z["bf16_emul_max"]), bf16_emul_mean=float(z["bf16_emul_mean"]))
    print("HED_PARITY " + json.dumps(rec))
    assert np.isfinite(out).all() and out.min() >= 0 and out.max() <= 255
    if prec == "fp32":
        assert d.max() <= 8 * float(z["ref_f32_vs_f64_max"]), rec
    else:
        assert d.max() <= 2 * float(z["bf16_emul_max"]) and d.mean() <= 2 * float(z["bf16_emul_mean"]), rec


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_control_output_is_the_scaled_edge_map_on_three_channels(outputs, engines, prec):
    for name in CASES:
        out, ctrl = outputs[prec, name]
        assert ctrl.dtype == engines[prec].dtype and tuple(ctrl.shape) == (out.shape[0], 3) + tuple(out.shape[1:])
        want = (2 * (out / 255 - 0.5)).to(ctrl.dtype)
        for ch in range(3):
            assert torch.equal(ctrl[:, ch], want), (name, ch)
        assert float(ctrl.float().min()) >= -1 and float(ctrl.float().max()) <= 1


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_second_call_and_control_only_call_give_the_same_bits(outputs, engines, prec):
    eng = engines[prec]
    for name in ("b1_72x104", "b2_16x24"):
        x = _x(name)
        again, ctrl = eng.hed(x, want_control=True)
        assert torch.equal(again.cpu(), outputs[prec, name][0]) and torch.equal(ctrl.cpu(), outputs[prec, name][1]), name
    # out = NULL: only the control tensor is written
    xg = x.cuda().float().contiguous()
    ctrl2 = torch.empty_like(ctrl)
    rc = eng.lib.car_hed(eng._h, C.c_void_p(xg.data_ptr()), 2, 16, 24, C.c_void_p(0), C.c_void_p(ctrl2.data_ptr()), C.c_void_p(int(torch.cuda.current_stream().cuda_stream)))
    assert rc == 0 and torch.equal(ctrl2.cpu(), outputs[prec, "b2_16x24"][1])
    # neither output: refused
    rc = eng.lib.car_hed(eng._h, C.c_void_p(xg.data_ptr()), 2, 16, 24, C.c_void_p(0), C.c_void_p(0), C.c_void_p(int(torch.cuda.current_stream().cuda_stream)))
    assert rc != 0


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_an_image_alone_equals_its_slice_of_the_batch(outputs, engines, prec):
    x = _x("b2_16x24")
    both = outputs[prec, "b2_16x24"][0]
    assert not torch.equal(both[0], both[1])
    for i in (1, 0):
        alone = engines[prec].hed(x[i:i + 1]).cpu()
        assert torch.equal(alone[0], both[i]), i


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_uint8_and_float_inputs_give_the_same_bits(outputs, engines, prec):
    x = _x("b1_35x50")
    assert x.dtype == torch.uint8
    for xx in (x.float(), x.double(), x.cuda()):
        assert torch.equal(engines[prec].hed(xx).cpu(), outputs[prec, "b1_35x50"][0])


def test_undersized_image_and_missing_weights_are_clean_errors(engines, weights):
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    eng = engines["bf16"]
    for shape in ((15, 15), (15, 64), (64, 15)):
        with pytest.raises(RuntimeError, match="at least 16 x 16"):
            eng.hed(torch.zeros(1, 3, *shape))
    assert tuple(eng.hed(torch.zeros(1, 3, 16, 16)).shape) == (1, 16, 16)             # the boundary itself runs
    bare = Engine(Cfg.tiny_t2i(), "bf16")
    with pytest.raises(RuntimeError, match="no HED weights"):
        bare.hed(torch.zeros(1, 3, 16, 16))
    part = {k: v for k, v in weights.items() if k != "block4.convs.2.bias"}
    with pytest.raises(RuntimeError, match="hed.block4.convs.2.bias"):
        bare.load_hed(part)                                                            # finalize names the missing tensor
    with pytest.raises(RuntimeError, match="hed.block9.weight: not a tensor of the HED network"):
        bare.load_state_dict({"hed.block9.weight": torch.zeros(1)})
    bare.close()


def test_hed_class_keeps_the_reference_use(weights, outputs, tmp_path):
    """condition.HEDdetector as sample_t2i.py:108-109,126-128 uses the reference's: construct, .to(device), .eval(), call on a uint8 (B,3,H,W) tensor."""
    from controlar_amd.condition import HEDdetector
    x = _x("b2_16x24")
    net = HEDdetector()
    net.load_state_dict({"netNetwork." + k: v for k, v in weights.items()})           # a detector's own state dict carries the prefix
    y = net.to("cuda").eval()(x)
    assert y.device == x.device and y.dtype == torch.float32 and torch.equal(y, outputs["bf16", "b2_16x24"][0])
    yg = net(x.cuda())
    assert yg.is_cuda and torch.equal(yg.cpu(), y)
    net._eng.close()
    path = str(tmp_path / "ControlNetHED.pth")                                         # model_path: a local file, as torch.load reads the reference's
    torch.save(weights, path)
    net2 = HEDdetector(model_path=path)
    assert torch.equal(net2(x), y)
    net2._eng.close()


def test_packed_cache_round_trip_reproduces_the_bits(engines, outputs, tmp_path):
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    path = str(tmp_path / "hed.carpk").encode()
    for prec in ("bf16", "fp32"):
        src = engines[prec]
        src._check(src.lib.car_export_packed(src._h, path), "car_export_packed")
        dst = Engine(Cfg.tiny_t2i(), prec)
        dst._check(dst.lib.car_import_packed(dst._h, path), "car_import_packed")
        assert torch.equal(dst.hed(_x("b1_35x50")).cpu(), outputs[prec, "b1_35x50"][0]), prec
        dst.close()
