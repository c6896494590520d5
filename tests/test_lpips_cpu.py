"""CPU side of the reconstruction judges (car_lpips, car_psnr, car_recon_to_u8): the C ABI declares, exports and binds them; the restatement in
tests/recon_ref.py is exact on identical inputs, symmetric, sensitive to every detail the issue names, and its trunk is the unmodified
``ControlNetHED_Apache2``'s; the quantiser and PSNR restatements equal the torch expression and the closed form; the loader's name map covers both
spellings of the trunk; the committed fixtures re-mint identically."""
import ctypes as C
import importlib.util
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import recon_ref as R      # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def mk():
    return _load("make_lpips_golden", os.path.join(GOLDEN, "make_lpips_golden.py"))


@pytest.fixture(scope="module")
def sd(mk):
    return mk.weights()


@pytest.fixture(scope="module")
def small(mk, sd):
    """the smallest fixture's inputs and its fp32 restatement, computed once"""
    torch.set_num_threads(1)
    a, b = mk.case_inputs("16x24")
    with torch.no_grad():
        val, layers = R.lpips(a, b, sd)
    return a, b, val, layers


def test_header_declares_library_exports_and_binding_has_the_new_entries():
    from controlar_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "controlar_hip.h")).read()
    nargs = {"car_lpips": 9, "car_psnr": 12, "car_recon_to_u8": 5, "car_debug_lpips_canonical_name": 3, "car_debug_lpips_chunk_pairs": 3}
    lib = L.load()
    for name, n in nargs.items():
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"include/controlar_hip.h does not declare {name}"
        assert len(m.group(1).split(",")) == n, name
        res, argtypes = L.SYMBOLS[name]
        assert res is C.c_int and len(argtypes) == n, name
        assert hasattr(lib, name)
    assert L.SYMBOLS["car_lpips"][1][3:6] == [C.c_int32] * 3 and L.SYMBOLS["car_psnr"][1][8] is C.c_int64 and L.SYMBOLS["car_psnr"][1][9] is C.c_double
    for k, v in (("CAR_PSNR_RAW", 0), ("CAR_PSNR_DIV255", 1), ("CAR_PSNR_HALF", 2)):
        assert getattr(L, k) == v and re.search(k + r"\s*=\s*%d" % v, hdr)
    assert lib.car_abi_version() == 2                      # additive: the ABI version stays


def test_loader_name_map_covers_both_trunk_spellings():
    from controlar_amd import _lib as L, synth
    lib = L.load()
    buf = C.create_string_buffer(128)

    def canon(name):
        return buf.value.decode() if lib.car_debug_lpips_canonical_name(name.encode(), buf, 128) == 0 else None

    ours, tv = synth.lpips_state_dict(17), synth.lpips_state_dict(17, spelling="torchvision")
    assert len(ours) == len(tv) == 26 + 5 + 2 and [tuple(v.shape) for v in ours.values()] == [tuple(v.shape) for v in tv.values()]
    assert all(torch.equal(x, y) for x, y in zip(ours.values(), tv.values()))
    assert sum(k.startswith("features.") for k in tv) == 26 and sum(k.startswith("net.slice") for k in ours) == 26
    assert len(synth.lpips_state_dict(17, scaling=False)) == 31
    for k_ours, k_tv in zip(ours, tv):                     # both spellings land on the LPIPS module's name
        assert canon("lpips." + k_ours) == "lpips." + k_ours, k_ours
        assert canon("lpips." + k_tv) == "lpips." + k_ours, k_tv
    stored = {canon("lpips." + k) for k in tv}
    assert len(stored) == 33
    idx = [n for s in R.SLICES for n in s]
    assert idx == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28] and synth.LPIPS_FEATURES == R.SLICES
    for bad in ("lpips.features.1.weight", "lpips.features.30.weight", "lpips.net.slice1.5.weight", "lpips.net.slice2.0.bias", "lpips.lin5.model.1.weight",
                "lpips.lin0.model.0.weight", "lpips.features.0.gamma", "hed.norm", "lpips.classifier.0.weight", "lpips.lin0.model.1.weightx"):
        assert canon(bad) is None, bad
    assert lib.car_debug_lpips_canonical_name(b"lpips.lin0.model.1.weight", buf, 8) != 0          # a short buffer is refused, not overrun


def test_chunk_rule_is_a_function_of_mode_and_size():
    from controlar_amd import _lib as L
    lib = L.load()
    f32, bf = lib.car_debug_lpips_chunk_pairs(L.CAR_F32, 16, 16), lib.car_debug_lpips_chunk_pairs(L.CAR_BF16, 16, 16)
    # per pair at 16 x 16: two images of (3 + 2 * 64) channels x 256 pixels in the element type, plus 256 bytes of partials; 1.5 GiB of workspace
    assert f32 == (1536 << 20) // (2 * (256 * 3 * 4 + 2 * 256 * 64 * 4) + 256) and bf == (1536 << 20) // (2 * (256 * 3 * 2 + 2 * 256 * 64 * 2) + 256)
    assert 5000 < f32 < bf < 32768
    assert lib.car_debug_lpips_chunk_pairs(L.CAR_F32, 4096, 4096) == 1                              # a chunk holds at least one whole pair
    assert lib.car_debug_lpips_chunk_pairs(L.CAR_F32, 15, 40) == -1 and lib.car_debug_lpips_chunk_pairs(7, 16, 16) == -1


def test_restatement_is_zero_on_identical_inputs_and_symmetric(small, sd):
    a, b, val, layers = small
    assert val.shape == (3,) and layers.shape == (3, 5)
    assert val[2] == 0 and (layers[2] == 0).all()                                                    # pair 2 is identical
    assert 0.05 < float(val[0]) < 2 and 0 < float(val[1]) < 1e-3 * float(val[0])                     # unrelated; a 1e-3 perturbation
    assert (layers > 0)[:2].all(), "every layer contributes: relu5_3 is not dead"
    with torch.no_grad():
        val_r, layers_r = R.lpips(b, a, sd)
    assert torch.equal(val_r, val) and torch.equal(layers_r, layers)
    assert torch.equal(layers.sum(dim=1), val) or torch.allclose(layers.sum(dim=1), val, rtol=1e-6, atol=0)


@pytest.mark.parametrize("mutation", [m for m in R.MUTATIONS if m != "eps_inside_root"])
def test_every_detail_of_the_restatement_moves_the_result(small, sd, mutation):
    """A misreading must move the unrelated pair's value by far more than the fp32 bound the GPU is held to (16 x the fixture's fp32-vs-fp64 deviation)."""
    a, b, val, _ = small
    bound = 16 * json.load(open(os.path.join(GOLDEN, "lpips_measured.json")))["16x24"]["f32_vs_f64_val"]
    with torch.no_grad():
        got, _ = R.lpips(a[:1], b[:1], sd, mutate=mutation)
    moved = abs(float(got[0]) - float(val[0]))
    print(f"LPIPS_MUTATION {mutation}: moved {moved:.3g}, bound {bound:.3g}")
    assert moved > 1000 * bound, (mutation, moved, bound)


def test_eps_placement_shows_on_faint_features_only(small, sd):
    """The eps inside the root, sqrt(sum x^2 + 1e-10), against lpips.py:159-160's sqrt(sum x^2) + 1e-10.  On the fixture inputs this misreading moves the
    value by 3.0e-8 (measured), which is BELOW the GPU's fp32 bound of 2.3e-7: the two forms differ by a relative 1e-10 / |x| - 0.5e-10 / |x|^2, and the taps
    of any image through a He-scaled (or the trained) trunk have norms of order 1.  No input with such norms can show it, so the criterion of the other three
    mutations cannot hold for this one; what can be held is checked here, on the fixture's own relu1_2 taps made faint (x 1e-6: norms around the eps):
    there the two forms differ by tens of percent, and the literal form is the one the restatement — and the kernel, which adds 1e-10f behind
    __fsqrt_rn — takes."""
    a, b, val, _ = small
    bound = 16 * json.load(open(os.path.join(GOLDEN, "lpips_measured.json")))["16x24"]["f32_vs_f64_val"]
    with torch.no_grad():
        got, _ = R.lpips(a[:1], b[:1], sd, mutate="eps_inside_root")
        tap = R.vgg16_taps(R.scaling_layer(a[:1], sd), sd)[0].double() * 1e-6
    moved = abs(float(got[0]) - float(val[0]))
    print(f"LPIPS_MUTATION eps_inside_root: moved {moved:.3g} on the fixture inputs, bound {bound:.3g}")
    assert moved < bound, "norms of order 1: the placement of the eps is invisible there (if this fails the fixture changed: use the common criterion)"
    lit, mut = R.normalize_tensor(tap), R.normalize_tensor(tap, mutate="eps_inside_root")
    n = tap.pow(2).sum(dim=1, keepdim=True).sqrt()
    assert 1e-7 < float(n.min()) and float(n.max()) < 1e-4
    assert torch.allclose(lit * (n + 1e-10), tap, rtol=1e-12, atol=0) and torch.allclose(mut * (n * n + 1e-10).sqrt(), tap, rtol=1e-12, atol=0)
    assert float(((lit - mut).abs().amax(dim=1) / lit.abs().amax(dim=1)).min()) > 0.1


def test_restated_trunk_is_the_reference_hed_trunk(sd):
    """vgg16.forward's thirteen convolutions, ReLUs and four pools are ControlNetHED_Apache2's: with norm = 0 the inputs of its five projections are the taps."""
    hed = _load("make_hed_golden", os.path.join(GOLDEN, "make_hed_golden.py"))
    if not hed.reference_tree_present():
        pytest.skip("the reference tree is absent")
    net = hed.import_reference_hed().ControlNetHED_Apache2().float().eval()
    own = net.state_dict()
    for s, idx in enumerate(R.SLICES, 1):
        for i, n in enumerate(idx):
            for p in ("weight", "bias"):
                own[f"block{s}.convs.{i}.{p}"] = sd[f"net.slice{s}.{n}.{p}"]
    own["norm"] = torch.zeros(1, 3, 1, 1)
    net.load_state_dict(own)
    seen = []
    for s in range(1, 6):
        getattr(net, f"block{s}").projection.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    torch.set_num_threads(1)
    x = torch.randn(1, 3, 35, 50, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        net(x)
        taps = R.vgg16_taps(x, sd)
    assert [tuple(t.shape) for t in seen] == [(1, 64, 35, 50), (1, 128, 17, 25), (1, 256, 8, 12), (1, 512, 4, 6), (1, 512, 2, 3)]
    for t, want in zip(taps, seen):
        assert torch.equal(t, want)
        assert 0.2 < float((want > 0).float().mean()) < 0.8, "neither dead nor saturated"


def test_quantiser_restatement_equals_the_torch_expression_on_a_dense_grid():
    """Every 2^-17 step of [-1.1, 1.1], the 256 bucket edges (x with 127.5 x + 128 = k) and their fp32 neighbours on both sides."""
    grid = torch.arange(-144180, 144181, dtype=torch.float64) / 131072.0
    edges = (torch.arange(0, 257, dtype=torch.float64) - 128.0) / 127.5
    e32 = edges.to(torch.float32)
    near = torch.cat([e32, torch.nextafter(e32, torch.tensor(2.0)), torch.nextafter(e32, torch.tensor(-2.0))])
    x = torch.cat([grid.to(torch.float32), near, torch.tensor([-1.1, 1.1, -1.0, 1.0, 0.0, -0.0, 1e-30, -1e-30])])
    want, got = R.recon_quantise_torch(x), R.recon_quantise(x)
    assert want.dtype == got.dtype == torch.uint8 and torch.equal(want, got)
    assert int(want.min()) == 0 and int(want.max()) == 255 and len(torch.unique(want)) == 256
    assert not torch.equal(want, (x.clamp(-1, 1).add(1).div(2).mul(255).add(0.5).clamp(0, 255)).to(torch.uint8)), "it is not save_image's rule"


def test_psnr_restatement_equals_the_closed_form_on_a_constant_offset():
    g = torch.Generator().manual_seed(3)
    a = torch.rand(2, 3, 8, 8, generator=g, dtype=torch.float64) * 0.5
    for delta, dr in ((0.125, 1.0), (0.25, 2.0), (2.0 ** -10, 1.0)):
        got = R.psnr(a, a + delta, data_range=dr)
        want = 20 * np.log10(dr / delta)                    # mse = delta^2 exactly: the offsets are powers of two
        assert torch.allclose(got, torch.full((2,), want, dtype=torch.float64), rtol=1e-14, atol=0), (delta, dr)
    assert torch.isinf(R.psnr(a, a)).all() and (R.psnr(a, a) > 0).all()
    u8 = torch.tensor([[0, 255, 128]], dtype=torch.uint8)
    rest, gt = R.restored_and_gt(u8, torch.tensor([[-1.0, 1.0, 0.0]]))
    assert rest.dtype == gt.dtype == torch.float32 and torch.equal(gt, torch.tensor([[0.0, 1.0, 0.5]])) and torch.equal(rest, u8.float() / 255.0)


def test_fixtures_hold_results_only_and_remint_identically(mk, sd, tmp_path):
    measured = json.load(open(os.path.join(GOLDEN, "lpips_measured.json")))
    assert sorted(measured) == sorted(mk.CASES)
    for name in mk.CASES:
        z = np.load(os.path.join(GOLDEN, f"lpips_{name}.npz"))
        assert sorted(z.files) == ["layers32", "layers64", "layers_bf", "psnr32", "psnr64", "val32", "val64", "val_bf"]
        assert os.path.getsize(os.path.join(GOLDEN, f"lpips_{name}.npz")) < 4096
        assert z["val64"].dtype == np.float64 and z["val64"][2] == 0 and z["val_bf"][2] == 0 and z["val32"][2] == 0
        m = measured[name]
        assert 0 < m["f32_vs_f64_val"] < 1e-6 and 0 < m["f32_vs_f64_layers"] < 1e-6 and m["f32_vs_f64_val"] < m["bf16_vs_f32_val"] < 1e-2
        assert 0 < m["psnr_f32_vs_f64"] < 1e-4
    torch.set_num_threads(1)
    path, rec = mk.mint("16x24", str(tmp_path), sd)
    new, old = np.load(path), np.load(os.path.join(GOLDEN, "lpips_16x24.npz"))
    for k in old.files:
        assert np.array_equal(new[k], old[k]), k
    assert rec == measured["16x24"]
