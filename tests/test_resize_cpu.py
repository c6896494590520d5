"""CPU side of the Pillow-exact resampler (car_resize): the C ABI declares, exports and binds both symbols at ABI version 2; the host-side coefficient
tables (car_debug_resample_coeffs) reproduce the fixtures' tables exactly for all five filters and both axes; the fixtures, minted from Pillow by
tests/golden/make_resize_golden.py, meet their conditions and re-mint identically; the reference's helpers keep their call shapes.

Two fixture conditions cannot hold for two cases, by construction and not by choice of seed: with both passes skipped (copy_64x48) the five filters
all return the input, and a 1 x 1 source (one_1x1) makes every normalised tap sum the pixel itself, so their outputs cannot differ pairwise and no
tap sum can leave 0..255.  Those two cases are exempt from exactly those two conditions and from nothing else."""
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
FILTERS = {"lanczos": 1, "bilinear": 2, "bicubic": 3, "box": 4, "hamming": 5}
# name -> (input shape, (Ho, Wo), box)
CASES = {
    "down_53x37": ((53, 37, 3), (16, 16), None),
    "up_l_31x20": ((31, 20), (48, 64), None),
    "half_64x64": ((64, 64, 3), (32, 32), None),
    "vonly_70x50": ((70, 50, 3), (35, 50), None),
    "honly_70x50": ((70, 50, 3), (70, 25), None),
    "copy_64x48": ((64, 48, 3), (64, 48), (0, 0, 48, 64)),
    "box_60x48": ((60, 48, 3), (32, 32), (3.5, 2, 40.25, 30)),
    "box_96x96": ((96, 96, 3), (32, 32), (10.5, 7.25, 80, 91.5)),
    "deep_l_200x300": ((200, 300), (16, 24), None),
    "up_33x47": ((33, 47, 3), (144, 160), None),
    "tiny_2x3": ((2, 3, 3), (4, 5), None),
    "one_1x1": ((1, 1, 3), (8, 8), None),
    "sq_40x56": ((40, 56, 3), (64, 64), None),
}
DEGENERATE = ("copy_64x48", "one_1x1")          # see the module docstring


def _minter():
    spec = importlib.util.spec_from_file_location("make_resize_golden", os.path.join(GOLDEN, "make_resize_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _z(name):
    return np.load(os.path.join(GOLDEN, f"resize_{name}.npz"))


def test_header_declares_library_exports_and_binding_has_both_symbols():
    from controlar_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "controlar_hip.h")).read()
    m = re.search(r"int\s+car_resize\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/controlar_hip.h does not declare car_resize"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(args) == 15 and args[0].startswith("car_ctx*") and args[1].startswith("const uint8_t*") and args[9].startswith("const float*")
    assert args[10].startswith("uint8_t*") and args[11].startswith("void*") and args[12].startswith("float*") and args[14].startswith("void*")
    m = re.search(r"int\s+car_debug_resample_coeffs\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/controlar_hip.h does not declare car_debug_resample_coeffs"
    assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == 9
    for word in ("RGBA", "NEAREST", "reducing_gap", "Out of scope"):
        assert word in hdr, word                               # what the resampler leaves out is stated where the contract is
    res, argtypes = L.SYMBOLS["car_resize"]
    assert res is C.c_int and len(argtypes) == 15 and argtypes[2:9] == [C.c_int32] * 7
    res, argtypes = L.SYMBOLS["car_debug_resample_coeffs"]
    assert res is C.c_int and len(argtypes) == 9 and argtypes[1:3] == [C.c_double] * 2
    lib = L.load()
    assert hasattr(lib, "car_resize") and hasattr(lib, "car_debug_resample_coeffs")
    assert lib.car_abi_version() == 2 and L.CAR_ABI_VERSION == 2          # additive: the ABI version stays
    assert (L.CAR_FILTER_LANCZOS, L.CAR_FILTER_BILINEAR, L.CAR_FILTER_BICUBIC, L.CAR_FILTER_BOX, L.CAR_FILTER_HAMMING) == (1, 2, 3, 4, 5)


def _coeffs(lib, in_size, in0, in1, out_size, f, cap=1 << 16):
    kk = np.full(cap, -12345, np.int32)
    bounds = np.full(out_size * 2, -12345, np.int32)
    ks = C.c_int32(0)
    rc = lib.car_debug_resample_coeffs(in_size, float(in0), float(in1), out_size, f, C.byref(ks), C.c_void_p(kk.ctypes.data), C.c_void_p(bounds.ctypes.data), cap)
    assert rc == 0, (in_size, in0, in1, out_size, f)
    assert (kk[out_size * ks.value:] == -12345).all()                       # nothing written past the table
    return ks.value, kk[:out_size * ks.value].reshape(out_size, ks.value), bounds.reshape(out_size, 2)


@pytest.mark.parametrize("name", list(CASES))
def test_host_tables_reproduce_the_fixture_tables_exactly(name):
    from controlar_amd import _lib as L
    lib = L.load()
    z = _z(name)
    shape, (Ho, Wo), box = CASES[name]
    H, W = shape[:2]
    assert tuple(z["out_size"]) == (Ho, Wo) and bool(z["has_box"]) == (box is not None)
    b = box if box is not None else (0, 0, W, H)
    assert tuple(z["box"]) == tuple(float(v) for v in b)
    for fname, f in FILTERS.items():
        for axis, (n_in, e0, e1, n_out) in (("h", (W, b[0], b[2], Wo)), ("v", (H, b[1], b[3], Ho))):
            want_kk, want_b = z[f"kk{axis}_{fname}"], z[f"b{axis}_{fname}"]
            ks, kk, bounds = _coeffs(lib, n_in, e0, e1, n_out, f)
            assert ks == want_kk.shape[1], (fname, axis)
            assert np.array_equal(kk, want_kk) and np.array_equal(bounds, want_b), (fname, axis)
            assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all() and (bounds[:, 1] <= ks).all()
    if name == "deep_l_200x300":
        assert z["kkv_lanczos"].shape[1] == 77 and z["kkh_lanczos"].shape[1] == 77


def test_host_tables_refuse_what_car_resize_refuses():
    from controlar_amd import _lib as L
    lib = L.load()
    kk = np.zeros(4096, np.int32)
    bounds = np.zeros(64, np.int32)
    ks = C.c_int32(0)

    def call(in_size, in0, in1, out_size, f, cap=4096):
        return lib.car_debug_resample_coeffs(in_size, in0, in1, out_size, f, C.byref(ks), C.c_void_p(kk.ctypes.data), C.c_void_p(bounds.ctypes.data), cap)

    assert call(16, 0.0, 16.0, 8, 3) == 0 and ks.value == 9
    assert call(16, 0.0, 16.0, 8, 0) != 0 and call(16, 0.0, 16.0, 8, 6) != 0 and call(16, 0.0, 16.0, 8, -1) != 0      # NEAREST, unknown filters
    assert call(0, 0.0, 16.0, 8, 3) != 0 and call(16, 0.0, 16.0, 0, 3) != 0                                           # non-positive sizes
    assert call(16, 4.0, 4.0, 8, 3) != 0 and call(16, 5.0, 4.0, 8, 3) != 0                                            # empty box
    assert call(16, -0.5, 16.0, 8, 3) != 0 and call(16, 0.0, 16.5, 8, 3) != 0 and call(16, float("nan"), 16.0, 8, 3) != 0   # outside the image
    assert call(16, 0.0, 16.0, 8, 3, cap=8 * 9 - 1) != 0 and call(16, 0.0, 16.0, 8, 3, cap=8 * 9) == 0               # capacity of kk


@pytest.mark.parametrize("name", list(CASES))
def test_fixtures_meet_their_conditions(name):
    z = _z(name)
    shape, (Ho, Wo), _ = CASES[name]
    oshape = (Ho, Wo) + tuple(shape[2:])
    assert z["x_noise"].shape == shape and z["x_binary"].shape == shape and z["x_noise"].dtype == np.uint8
    assert set(np.unique(z["x_binary"])) <= {0, 255}
    for fname in FILTERS:
        assert z[f"noise_{fname}"].shape == oshape and z[f"binary_{fname}"].shape == oshape and z[f"noise_{fname}"].dtype == np.uint8
    for fname in ("bicubic", "lanczos"):                     # the binary input reaches both ends of the clamp
        out = z[f"binary_{fname}"]
        assert out.min() == 0 and out.max() == 255, fname
        if name not in DEGENERATE:                           # ... and tap sums really left 0..255 before it, on both sides
            assert z[f"over_{fname}"][0] > 0 and z[f"over_{fname}"][1] > 0, (fname, z[f"over_{fname}"])
    if name not in DEGENERATE:
        names = list(FILTERS)
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                assert not np.array_equal(z[f"noise_{a}"], z[f"noise_{b}"]), (a, b)
    else:
        assert all(np.array_equal(z[f"noise_{a}"], z["noise_box"]) for a in FILTERS)


def test_crop_fixture_is_the_box_then_bicubic_chain():
    z = _z("crop_150x210")
    assert z["x_noise"].shape == (150, 210, 3) and int(z["image_size"]) == 32 and tuple(z["resized_size"]) == (45, 32)
    assert z["resized_noise"].shape == (32, 45, 3) and z["crop_noise"].shape == (32, 32, 3)
    mk = _minter()
    steps, (cy, cx) = mk.center_crop_sizes(150, 210, 32)
    assert steps == [(105, 75, mk.BOX), (52, 37, mk.BOX), (45, 32, mk.BICUBIC)] and (cy, cx) == (0, 6)
    assert np.array_equal(z["crop_binary"], z["resized_binary"][:, 6:38])
    assert z["crop_binary"].min() == 0 and z["crop_binary"].max() == 255


def test_fixture_set_stays_within_one_committed_file_limit():
    files = [f for f in os.listdir(GOLDEN) if f.startswith("resize_") and f.endswith(".npz")]
    assert sorted(files) == sorted([f"resize_{n}.npz" for n in CASES] + ["resize_crop_150x210.npz"])
    assert sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in files) <= 1 << 20


def test_reminting_reproduces_the_committed_fixtures(tmp_path):
    pytest.importorskip("PIL")
    mk = _minter()
    assert {k: v[:3] for k, v in mk.CASES.items()} == CASES and mk.FILTERS == FILTERS
    for name in ("box_60x48", "tiny_2x3", "up_l_31x20", "crop_150x210"):
        new, old = np.load(mk.mint(name, str(tmp_path))), _z(name)
        assert sorted(new.files) == sorted(old.files)
        for k in old.files:
            assert np.array_equal(new[k], old[k]), (name, k)


def test_restatement_equals_the_fixtures_without_pillow():
    """The NumPy restatement in the minter is the specification: it reproduces Pillow's stored outputs with no Pillow in the loop."""
    mk = _minter()
    for name in ("down_53x37", "box_96x96", "deep_l_200x300", "one_1x1", "copy_64x48"):
        z = _z(name)
        _, (Ho, Wo), box = CASES[name]
        for fname, f in FILTERS.items():
            for kind in ("noise", "binary"):
                assert np.array_equal(mk.resize(z[f"x_{kind}"], (Wo, Ho), f, box), z[f"{kind}_{fname}"]), (name, fname, kind)


def test_helpers_keep_the_reference_call_shapes():
    from controlar_amd import condition as K
    from controlar_amd.demo import Model
    from controlar_amd.engine import Engine
    assert list(inspect.signature(K.center_crop_arr).parameters)[:2] == ["pil_image", "image_size"]
    p = inspect.signature(K.resize_image_to_16_multiple).parameters
    assert list(p)[:2] == ["image_path", "condition_type"] and p["condition_type"].default == "seg"
    assert list(inspect.signature(K.resize_image).parameters)[:2] == ["input_image", "resolution"]
    assert list(inspect.signature(K.HWC3).parameters) == ["x"]
    p = inspect.signature(K.Resizer.__call__).parameters
    assert list(p) == ["self", "img", "size", "resample", "box"] and p["resample"].default == K.BICUBIC == 3 and p["box"].default is None
    p = inspect.signature(Engine.resize).parameters
    assert list(p) == ["self", "img", "size", "resample", "box", "want_control", "want_float"]
    assert p["resample"].default == "bicubic" and p["box"].default is None and p["want_control"].default is False and p["want_float"].default is None
    p = inspect.signature(K.DepthEstimator.preprocess).parameters
    assert list(p) == ["images", "size"] and p["size"].default is None
    p = inspect.signature(Model.__init__).parameters
    assert list(p)[-3:] == ["hed", "lineart", "depth"] and all(p[k].default is None for k in ("hed", "lineart", "depth"))
    assert (K.LANCZOS, K.BILINEAR, K.BICUBIC, K.BOX, K.HAMMING) == (1, 2, 3, 4, 5)


def test_hwc3_is_the_reference_rule():
    """condition/utils.py:9-25: grey -> three equal channels, RGB untouched, RGBA blended over white in fp32 and truncated."""
    from controlar_amd.condition import HWC3
    rng = np.random.default_rng(5)
    g = rng.integers(0, 256, (5, 7), dtype=np.uint8)
    out = HWC3(g)
    assert isinstance(out, np.ndarray) and out.shape == (5, 7, 3) and all(np.array_equal(out[:, :, c], g) for c in range(3))
    assert np.array_equal(HWC3(g[:, :, None]), out)
    rgb = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    assert np.array_equal(HWC3(rgb), rgb)
    rgba = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    color, alpha = rgba[:, :, 0:3].astype(np.float32), rgba[:, :, 3:4].astype(np.float32) / 255.0
    want = (color * alpha + 255.0 * (1.0 - alpha)).clip(0, 255).astype(np.uint8)
    assert np.array_equal(HWC3(rgba), want)
    t = HWC3(torch.from_numpy(rgba))
    assert torch.is_tensor(t) and np.array_equal(t.numpy(), want)
    with pytest.raises(AssertionError):
        HWC3(rng.integers(0, 256, (5, 7, 2), dtype=np.uint8))


def test_demo_model_without_the_new_arguments_raises_as_before():
    from PIL import Image
    from controlar_amd.demo import Model
    img = Image.fromarray(np.zeros((8, 8, 3), np.uint8))
    for name in ("HED", "Lineart", "Depth"):
        with pytest.raises(RuntimeError, match="needs the preprocessor callable"):
            Model()._preprocess(name, img, detect_resolution=64)
    assert Model()._preprocess("No preprocess", img) is img
    seen = []
    m = Model(preprocessor=lambda name, image, **kw: seen.append((name, kw)) or image, hed=object())
    assert m._preprocess("HED", img, detect_resolution=64) is img and seen == [("HED", {"detect_resolution": 64})]     # an injected preprocessor wins
