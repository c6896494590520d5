"""CPU side of the DPT depth estimator (car_depth): the C ABI declares, exports and binds it, the committed fixtures meet the conditions that make them
worth grading against, the synthetic weights carry exactly the names and shapes of transformers' DPTForDepthEstimation (tiny configs and dpt_large),
and a fixture re-mints identically from the unmodified reference class."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = {"b2_32": ("tiny_dpt", 2, 32), "b1_64": ("tiny_dpt", 1, 64), "b1_96": ("tiny_dpt", 1, 96), "b1_128": ("tiny_dpt", 1, 128),
         "wide_b1_64": ("tiny_dpt_wide", 1, 64)}


def _minter():
    spec = importlib.util.spec_from_file_location("make_depth_golden", os.path.join(GOLDEN, "make_depth_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _need_transformers(mk):
    if not mk.transformers_present():
        pytest.skip("transformers is absent")


def test_header_declares_library_exports_and_binding_has_car_depth():
    from controlar_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "controlar_hip.h")).read()
    m = re.search(r"int\s+car_depth\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/controlar_hip.h does not declare car_depth"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 8 and args[0].startswith("car_ctx*") and args[1].startswith("const float*") and args[5].startswith("float*")
    assert args[6].startswith("void*") and args[7].startswith("void*")
    assert re.search(r"int\s+car_depth_configure\s*\(\s*car_ctx\*\s*\w+\s*,\s*const\s+car_dpt_config\*\s*\w+\s*\)\s*;", hdr)
    body = re.search(r"typedef struct car_dpt_config \{(.*?)\} car_dpt_config;", hdr, re.S).group(1)
    fields = re.findall(r"(int32_t|float)\s+(\w+)(?:\[(\d+)\])?;", body)
    assert [(t, n, int(k or 1)) for t, n, k in fields] == [
        ("int32_t", "hidden", 1), ("int32_t", "layers", 1), ("int32_t", "heads", 1), ("int32_t", "mlp", 1), ("int32_t", "pos_grid", 1),
        ("int32_t", "out_indices", 4), ("int32_t", "neck_hidden", 4), ("int32_t", "fusion_hidden", 1), ("float", "ln_eps", 1), ("int32_t", "reserved", 8)]
    assert [(n, getattr(t, "_length_", 1)) for n, t in L.CarDptConfig._fields_] == [(n, k) for _, n, k in [(t, n, int(k or 1)) for t, n, k in fields]]
    assert C.sizeof(L.CarDptConfig) == 4 * 23
    res, argtypes = L.SYMBOLS["car_depth"]
    assert res is C.c_int and len(argtypes) == 8 and argtypes[2:5] == [C.c_int32] * 3
    lib = L.load()
    assert hasattr(lib, "car_depth") and hasattr(lib, "car_depth_configure")
    assert lib.car_abi_version() == 2                      # additive: the ABI version stays


def test_configs_are_the_stated_ones_and_the_family_check_names_what_is_outside():
    from controlar_amd import config as Cfg
    big = Cfg.dpt_large()
    assert (big.hidden_size, big.num_hidden_layers, big.num_attention_heads, big.intermediate_size, big.pos_grid) == (1024, 24, 16, 4096, 24)
    assert tuple(big.backbone_out_indices) == (5, 11, 17, 23) and tuple(big.neck_hidden_sizes) == (256, 512, 1024, 1024)
    assert big.fusion_hidden_size == 256 and big.layer_norm_eps == 1e-12 and big.family_errors() == []
    t, w = Cfg.tiny_dpt(), Cfg.tiny_dpt_wide()
    assert (t.hidden_size, t.num_attention_heads, t.num_hidden_layers, t.intermediate_size, t.pos_grid, t.fusion_hidden_size) == (128, 2, 4, 512, 4, 64)
    assert tuple(t.neck_hidden_sizes) == (64, 64, 128, 128) and tuple(t.backbone_out_indices) == (0, 1, 2, 3)
    assert (w.hidden_size, w.num_attention_heads, w.num_hidden_layers, w.intermediate_size, w.pos_grid, w.fusion_hidden_size) == (256, 4, 4, 1024, 4, 128)
    assert tuple(w.neck_hidden_sizes) == (96, 192, 384, 384)
    for kw in (dict(is_hybrid=True), dict(readout_type="add"), dict(use_batch_norm_in_fusion_residual=True), dict(add_projection=True),
               dict(hidden_act="relu"), dict(reassemble_factors=(4, 2, 1, 1))):
        assert Cfg.DPTConfig(**kw).family_errors(), kw
    assert Cfg.DPTConfig.from_hf_dict(dict(big.to_hf_dict(), model_type="dpt", torch_dtype="float32")) == big


def test_synthetic_weights_are_deterministic_and_follow_the_recipe():
    from controlar_amd import config as Cfg, synth
    cfg = Cfg.tiny_dpt()
    sd = synth.dpt_state_dict(cfg, 13)
    assert all(v.dtype == torch.float32 for v in sd.values())
    assert sum(v.numel() * 4 for v in sd.values()) / 1e6 == pytest.approx(8.6, abs=0.1)          # 8.6 MB of weights
    again = synth.dpt_state_dict(cfg, 13)
    assert all(torch.equal(v, again[k]) for k, v in sd.items())
    assert not torch.equal(sd["neck.convs.1.weight"], synth.dpt_state_dict(cfg, 14)["neck.convs.1.weight"])
    assert float(sd["head.head.4.bias"]) == 1.0
    w = sd["neck.fusion_stage.layers.2.residual_layer1.convolution1.weight"]
    assert float(w.std()) == pytest.approx((64 * 9) ** -0.5, rel=0.05)                              # N(0, 1/fan_in)
    t = sd["neck.reassemble_stage.layers.0.resize.weight"]
    assert tuple(t.shape) == (64, 64, 4, 4) and float(t.std()) == pytest.approx(64 ** -0.5, rel=0.05)   # a k = stride transposed conv: fan-in Cin


@pytest.mark.parametrize("cfg_name", ["tiny_dpt", "tiny_dpt_wide"])
def test_synthetic_weights_have_the_names_and_shapes_of_the_hf_model(cfg_name):
    mk = _minter()
    _need_transformers(mk)
    from transformers import DPTForDepthEstimation
    from controlar_amd import config as Cfg, synth
    cfg = getattr(Cfg, cfg_name)()
    ref = DPTForDepthEstimation(mk.hf_config(cfg)).state_dict()
    sd = synth.dpt_state_dict(cfg, 13)
    assert sorted(ref) == sorted(sd)
    assert all(tuple(ref[k].shape) == tuple(sd[k].shape) for k in ref)


def test_dpt_large_names_and_shapes_equal_the_hf_model_on_the_meta_device():
    """Pins the name list car_finalize_weights expects to the real checkpoint's, without allocating its 1.4 GB."""
    mk = _minter()
    _need_transformers(mk)
    from transformers import DPTForDepthEstimation
    from controlar_amd import config as Cfg, synth
    cfg = Cfg.dpt_large()
    with torch.device("meta"):
        ref = {k: tuple(v.shape) for k, v in DPTForDepthEstimation(mk.hf_config(cfg)).state_dict().items()}
        mine = {k: tuple(v.shape) for k, v in synth.dpt_state_dict(cfg, 13).items()}
    assert sorted(ref) == sorted(mine) and all(ref[k] == mine[k] for k in ref)
    assert ref["dpt.embeddings.position_embeddings"] == (1, 577, 1024) and ref["neck.reassemble_stage.layers.0.resize.weight"] == (256, 256, 4, 4)
    assert ref["head.head.0.weight"] == (128, 256, 3, 3) and len(ref) == 462


@pytest.mark.parametrize("name", list(CASES))
def test_fixtures_meet_their_conditions(name):
    mk = _minter()
    z = np.load(os.path.join(GOLDEN, f"depth_{name}.npz"))
    cfg_name, B, S = CASES[name]
    assert mk.CASES[name][:3] == (cfg_name, B, S)
    assert z["x"].dtype == np.uint8 and z["x"].shape == (B, 3, S, S)
    assert z["ref"].dtype == np.float32 and z["ref"].shape == (B, S, S) and z["ref"].min() >= 0
    assert float(z["zero_share"]) == pytest.approx(float((z["ref"] == 0).mean()), abs=1e-6)
    mk.check_case(name, z)                                 # zero share <= 0.25, maximum >= 1, emulation <= 1.5 x native (max and mean)
    assert 0 < float(z["ref_f32_vs_f64_max"]) < 1e-4
    assert 0 < float(z["bf16_native_mean"]) < float(z["bf16_native_max"]) < 0.2
    assert os.path.getsize(os.path.join(GOLDEN, f"depth_{name}.npz")) < 150_000
    if B == 2:
        assert not np.array_equal(z["ref"][0], z["ref"][1])


def test_some_fixture_exercises_the_final_relu():
    mk = _minter()
    mk.check_all([np.load(os.path.join(GOLDEN, f"depth_{n}.npz")) for n in CASES])


def test_reminting_the_smallest_case_reproduces_the_committed_fixture(tmp_path):
    mk = _minter()
    _need_transformers(mk)
    new = np.load(mk.mint("b2_32", str(tmp_path)))
    old = np.load(os.path.join(GOLDEN, "depth_b2_32.npz"))
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert np.array_equal(new[k], old[k]), k


def test_reference_raises_on_a_non_square_image():
    """car_depth refuses a non-square image because the reference does: its reassemble stage takes sqrt of the token count."""
    mk = _minter()
    _need_transformers(mk)
    model = mk.build_model("tiny_dpt")
    with torch.no_grad(), pytest.raises(RuntimeError):
        model(pixel_values=torch.zeros(1, 3, 48, 80))


def test_depth_estimator_preprocess_is_the_processors_rescale_and_normalise():
    from controlar_amd.condition import DepthEstimator
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, "depth_b2_32.npz"))["x"])
    pv = DepthEstimator.preprocess(x)
    assert pv.dtype == torch.float32 and torch.equal(pv, (x.to(torch.float32) / 255 - 0.5) / 0.5)
    assert torch.equal(pv, _minter().pixel_values(x))
