"""CPU side of the HED extractor (car_hed): the C ABI declares, exports and binds it, the drop-in class keeps the reference's call shape, the synthetic
weights carry the reference's 37 names and shapes, the committed fixtures re-mint identically from the reference and are not graded on a saturated
sigmoid, and the reference's own lower size limit is 16."""
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
CASES = {"b2_16x24": (2, 16, 24), "b1_17x31": (1, 17, 31), "b1_35x50": (1, 35, 50), "b1_72x104": (1, 72, 104)}


def _minter():
    spec = importlib.util.spec_from_file_location("make_hed_golden", os.path.join(GOLDEN, "make_hed_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_header_declares_library_exports_and_binding_has_car_hed():
    from controlar_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "controlar_hip.h")).read()
    m = re.search(r"int\s+car_hed\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/controlar_hip.h does not declare car_hed"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 8 and args[0].startswith("car_ctx*") and args[1].startswith("const float*") and args[5].startswith("float*")
    assert args[6].startswith("void*") and args[7].startswith("void*")
    res, argtypes = L.SYMBOLS["car_hed"]
    assert res is C.c_int and len(argtypes) == 8 and argtypes[2:5] == [C.c_int32] * 3
    lib = L.load()
    assert hasattr(lib, "car_hed")
    assert lib.car_abi_version() == 2                      # additive: the ABI version stays


def test_hed_class_has_the_reference_call_shape():
    from controlar_amd.condition import HEDdetector
    assert list(inspect.signature(HEDdetector.__call__).parameters) == ["self", "input_image"]
    init = inspect.signature(HEDdetector.__init__).parameters
    assert list(init) == ["self", "model_path", "precision", "device"]
    assert init["model_path"].default is None and init["precision"].default == "bf16" and init["device"].default is None
    for name in ("load_state_dict", "to", "eval"):
        assert callable(getattr(HEDdetector, name))
    mk = _minter()
    if mk.reference_tree_present():
        ref = mk.import_reference_hed().HEDdetector
        assert list(inspect.signature(ref.__call__).parameters) == ["self", "input_image"]
        assert list(inspect.signature(ref.__init__).parameters) == ["self"]          # every argument of the drop-in's constructor is optional


def test_synthetic_weights_are_deterministic_and_have_the_reference_names_and_shapes():
    from controlar_amd import synth
    sd = synth.hed_state_dict(11)
    assert len(sd) == 37 and sd["norm"].shape == (1, 3, 1, 1) and sd["block1.convs.0.weight"].shape == (64, 3, 3, 3)
    assert sd["block4.convs.0.weight"].shape == (512, 256, 3, 3) and sd["block5.projection.weight"].shape == (1, 512, 1, 1)
    assert sum(v.numel() for v in sd.values()) == 14_716_168                         # 14.7 M parameters
    again = synth.hed_state_dict(11)
    assert all(torch.equal(v, again[k]) for k, v in sd.items())
    assert not torch.equal(sd["block3.convs.1.weight"], synth.hed_state_dict(12)["block3.convs.1.weight"])
    mk = _minter()
    if mk.reference_tree_present():
        ref = mk.import_reference_hed().ControlNetHED_Apache2().state_dict()
        assert list(ref) == list(sd) and all(tuple(ref[k].shape) == tuple(sd[k].shape) for k in ref)


@pytest.mark.parametrize("name", list(CASES))
def test_fixtures_are_not_graded_on_a_saturated_sigmoid(name):
    z = np.load(os.path.join(GOLDEN, f"hed_{name}.npz"))
    B, H, W = CASES[name]
    assert z["x"].dtype == np.uint8 and z["x"].shape == (B, 3, H, W)
    assert z["ref"].dtype == np.float32 and z["ref"].shape == (B, H, W)
    ref = z["ref"]
    assert ref.min() >= 0 and ref.max() <= 255
    assert ((ref >= 5) & (ref <= 250)).mean() >= 0.5, "at least half of the pixels lie in 5..250"
    assert 0 < float(z["ref_f32_vs_f64_max"]) < 1e-3 and 0 < float(z["bf16_emul_mean"]) < float(z["bf16_emul_max"]) < 5
    assert os.path.getsize(os.path.join(GOLDEN, f"hed_{name}.npz")) < 62555 + B * 3 * H * W      # the largest LineArt fixture plus the uint8 input


def test_reminting_the_smallest_case_reproduces_the_committed_fixture(tmp_path):
    mk = _minter()
    if not mk.reference_tree_present():
        pytest.skip("the reference tree is absent")
    assert {k: v[:3] for k, v in mk.CASES.items()} == CASES
    det = mk.build_model(mk.import_reference_hed())
    for name in ("b2_16x24", "b1_17x31"):
        new = np.load(mk.mint(name, str(tmp_path), det))
        old = np.load(os.path.join(GOLDEN, f"hed_{name}.npz"))
        assert sorted(new.files) == sorted(old.files)
        for k in old.files:
            assert np.array_equal(new[k], old[k]), (name, k)


def test_reference_runs_at_16x16_and_raises_at_15x15():
    """car_hed refuses H or W below 16 because the reference does: four 2x2 max-pools turn 15 into 0 and max_pool2d raises."""
    mk = _minter()
    if not mk.reference_tree_present():
        pytest.skip("the reference tree is absent")
    det = mk.build_model(mk.import_reference_hed())
    with torch.no_grad():
        assert tuple(det(torch.zeros(1, 3, 16, 16, dtype=torch.uint8)).shape) == (1, 16, 16)
        for shape in ((15, 15), (15, 64), (64, 15)):
            with pytest.raises(RuntimeError):
                det(torch.zeros(1, 3, *shape, dtype=torch.uint8))
