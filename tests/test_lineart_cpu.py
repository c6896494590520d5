"""CPU side of the LineArt extractor (car_lineart): the C ABI declares, exports and binds it, the drop-in class keeps the reference's call shape,
the output-size rule, the committed fixtures re-mint identically from the reference, and the reference's own lower size limit is 5."""
import ctypes as C
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _minter():
    spec = importlib.util.spec_from_file_location("make_lineart_golden", os.path.join(GOLDEN, "make_lineart_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_header_declares_library_exports_and_binding_has_car_lineart():
    from controlar_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "controlar_hip.h")).read()
    m = re.search(r"int\s+car_lineart\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/controlar_hip.h does not declare car_lineart"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 8 and args[0].startswith("car_ctx*") and args[1].startswith("const float*") and args[5].startswith("float*")
    res, argtypes = L.SYMBOLS["car_lineart"]
    assert res is C.c_int and len(argtypes) == 8 and argtypes[2:5] == [C.c_int32] * 3
    lib = L.load()
    assert hasattr(lib, "car_lineart")
    assert lib.car_abi_version() == 2                      # additive: the ABI version stays


def test_lineart_class_has_the_reference_call_shape():
    from controlar_amd.condition import LineArt
    sig = inspect.signature(LineArt.forward)
    assert list(sig.parameters) == ["self", "x", "cond"] and sig.parameters["cond"].default is None
    assert list(inspect.signature(LineArt.__call__).parameters) == ["self", "x", "cond"]
    init = inspect.signature(LineArt.__init__).parameters
    assert init["precision"].default == "bf16" and init["n_residual_blocks"].default == 3 and init["sigmoid"].default is True
    for name in ("load_state_dict", "to", "eval"):
        assert callable(getattr(LineArt, name))
    mk = _minter()
    if mk.reference_tree_present():
        ref = mk.import_reference_lineart().LineArt
        assert list(inspect.signature(ref.forward).parameters) == list(sig.parameters)
        ri = inspect.signature(ref.__init__).parameters
        assert [(k, ri[k].default) for k in ("input_nc", "output_nc", "n_residual_blocks", "sigmoid")] == \
               [(k, init[k].default) for k in ("input_nc", "output_nc", "n_residual_blocks", "sigmoid")]


def test_output_size_rule():
    """Ho = 4 * ceil(ceil(H/2)/2): two stride-2 convs with padding 1 (floor((n-1)/2)+1 each), two 2x transposed convs."""
    from controlar_amd.engine import Engine
    for n in range(5, 200):
        want = 4 * -(-(-(-n // 2)) // 2)
        assert Engine.lineart_output_size(n, n) == (want, want), n
    assert Engine.lineart_output_size(30, 44) == (32, 44)
    assert Engine.lineart_output_size(512, 768) == (512, 768)
    for name in ("b2_16x24", "b1_30x44", "b1_8x8", "b1_72x104"):
        z = np.load(os.path.join(GOLDEN, f"lineart_{name}.npz"))
        B, _, H, W = z["x"].shape
        assert z["ref"].shape == (B, 1) + Engine.lineart_output_size(H, W), name
        assert z["x"].min() >= 0 and z["x"].max() <= 255 and np.array_equal(z["x"], np.round(z["x"]))       # integer-valued: exact in bf16
        assert 0 < float(z["ref_f32_vs_f64_max"]) < 1e-4 and 0 < float(z["bf16_emul_mean"]) < float(z["bf16_emul_max"]) < 0.2


def test_synthetic_weights_have_the_reference_names_and_spread_the_output():
    from controlar_amd import synth
    sd = synth.lineart_state_dict(11)
    assert len(sd) == 24 and sd["model0.1.weight"].shape == (64, 3, 7, 7) and sd["model3.0.weight"].shape == (256, 128, 3, 3)
    assert sd["model4.1.weight"].shape == (1, 64, 7, 7) and sum(v.numel() for v in sd.values()) == 4_290_945       # 4.29 M parameters
    assert all(torch.equal(v, synth.lineart_state_dict(11)[k]) for k, v in sd.items())
    z = np.load(os.path.join(GOLDEN, "lineart_b1_72x104.npz"))
    assert z["ref"].min() < 0.02 and z["ref"].max() > 0.98 and 0.2 < z["ref"].std() < 0.4             # not the stock init's flat 0.5


def test_reminting_the_smallest_case_reproduces_the_committed_fixture(tmp_path):
    mk = _minter()
    if not mk.reference_tree_present():
        pytest.skip("the reference tree is absent")
    new = np.load(mk.mint("b1_8x8", str(tmp_path)))
    old = np.load(os.path.join(GOLDEN, "lineart_b1_8x8.npz"))
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert np.array_equal(new[k], old[k]), k


def test_reference_accepts_5x5_and_raises_at_4x4():
    """car_lineart refuses H or W below 5 because the reference does: two stride-2 convs turn 4 into 1, where ReflectionPad2d(1) needs 2 (RuntimeError)
    and, at 1 x 1, InstanceNorm2d refuses a single spatial element first (ValueError)."""
    mk = _minter()
    if not mk.reference_tree_present():
        pytest.skip("the reference tree is absent")
    net = mk.build_model(mk.import_reference_lineart())
    with torch.no_grad():
        assert tuple(net(torch.zeros(1, 3, 5, 5)).shape) == (1, 1, 8, 8)
        assert tuple(net(torch.zeros(1, 3, 5, 9)).shape) == (1, 1, 8, 12)
        for shape in ((4, 4), (4, 9), (9, 4)):
            with pytest.raises((RuntimeError, ValueError)):
                net(torch.zeros(1, 3, *shape))
