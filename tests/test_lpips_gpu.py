"""car_lpips, car_psnr and car_recon_to_u8 on the GPU (pytest -m gpu) against the fixtures minted on the CPU from tests/recon_ref.py
(tests/golden/make_lpips_golden.py: inputs and weights from seeds, expected values and the restatement's own deviations committed).

Tolerances come from tests/golden/lpips_measured.json, per fixture: exact mode |out - fp64| <= 16 x the restatement's own |fp32 - fp64|; fast mode
|out - fp32| <= 2 x the restatement's own |bf16-operand emulation - fp32|; the same for the per-layer terms.  Each case prints its measured figures as
one LPIPS_PARITY JSON line (pytest -s) before it asserts."""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import recon_ref as R      # noqa: E402

CASES = ["16x24", "17x31", "35x50", "72x104"]
PRECS = ["fp32", "bf16"]


def _minter():
    spec = importlib.util.spec_from_file_location("make_lpips_golden", os.path.join(GOLDEN, "make_lpips_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def mk():
    return _minter()


@pytest.fixture(scope="module")
def measured():
    return json.load(open(os.path.join(GOLDEN, "lpips_measured.json")))


@pytest.fixture(scope="module")
def inputs(mk):
    return {name: mk.case_inputs(name) for name in CASES}


@pytest.fixture(scope="module")
def engines(mk):
    """fp32: the LPIPS module's own names with its ScalingLayer buffers; bf16: torchvision's trunk names and no buffers (the constants): both against one golden"""
    from controlar_amd import config as Cfg, synth
    from controlar_amd.engine import Engine
    e = {"fp32": Engine(Cfg.tiny_t2i(), "fp32"), "bf16": Engine(Cfg.tiny_t2i(), "bf16")}
    e["fp32"].load_lpips(synth.lpips_state_dict(mk.WEIGHT_SEED))
    e["bf16"].load_lpips(synth.lpips_state_dict(mk.WEIGHT_SEED, spelling="torchvision", scaling=False))
    yield e
    for v in e.values():
        v.close()


@pytest.fixture(scope="module")
def outputs(engines, inputs):
    """every case once per mode, with the per-layer terms: shared by the tests below and left unchanged"""
    res = {}
    for prec, eng in engines.items():
        for name in CASES:
            a, b = inputs[name]
            val, lay = eng.lpips(a, b, want_layers=True)
            torch.cuda.synchronize()
            res[prec, name] = (val.cpu(), lay.cpu())
    return res


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("prec", PRECS)
def test_lpips_matches_the_restatement(outputs, measured, prec, name):
    z, m = np.load(os.path.join(GOLDEN, f"lpips_{name}.npz")), measured[name]
    val, lay = (t.numpy() for t in outputs[prec, name])
    assert val.shape == (3,) and lay.shape == (3, 5) and val.dtype == lay.dtype == np.float64
    ref_v, ref_l = (z["val64"], z["layers64"]) if prec == "fp32" else (z["val32"].astype(np.float64), z["layers32"].astype(np.float64))
    dv, dl = np.abs(val - ref_v), np.abs(lay - ref_l)
    bound_v, bound_l = (16 * m["f32_vs_f64_val"], 16 * m["f32_vs_f64_layers"]) if prec == "fp32" else (2 * m["bf16_vs_f32_val"], 2 * m["bf16_vs_f32_layers"])
    rec = dict(case=name, mode=prec, val=val.tolist(), max_abs_val=float(dv.max()), per_pair_val=dv.tolist(), bound_val=bound_v,
               max_abs_layers=float(dl.max()), bound_layers=bound_l)
    print("LPIPS_PARITY " + json.dumps(rec))
    assert np.isfinite(val).all() and (lay >= 0).all()
    assert (val[2] == 0.0) and (lay[2] == 0.0).all(), "an identical pair is exactly 0 in every layer"
    assert dv.max() <= bound_v and dl.max() <= bound_l, rec


@pytest.mark.parametrize("prec", PRECS)
def test_value_is_the_sum_of_the_layers_in_order_and_symmetric_in_its_arguments(outputs, engines, inputs, prec):
    for name in CASES:
        val, lay = outputs[prec, name]
        want = lay[:, 0].clone()
        for l in range(1, 5):
            want = want + lay[:, l]
        assert torch.equal(want, val), name
        a, b = inputs[name]
        rv, rl = engines[prec].lpips(b, a, want_layers=True)
        assert torch.equal(rv.cpu(), val) and torch.equal(rl.cpu(), lay), name


@pytest.mark.parametrize("prec", PRECS)
def test_second_call_other_stream_and_a_pair_alone_give_the_same_bits(outputs, engines, inputs, prec):
    eng = engines[prec]
    for name in ("72x104", "16x24"):
        a, b = (t.cuda() for t in inputs[name])
        val, lay = outputs[prec, name]
        assert torch.equal(eng.lpips(a, b).cpu(), val), name                       # a second call, without the layers
        for i in (2, 1, 0):                                                        # a pair alone = its slice of the batch of 3
            v1, l1 = eng.lpips(a[i:i + 1], b[i:i + 1], want_layers=True)
            assert torch.equal(v1.cpu(), val[i:i + 1]) and torch.equal(l1.cpu(), lay[i:i + 1]), (name, i)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            v2, l2 = eng.lpips(a, b, want_layers=True)
        s.synchronize()
        assert torch.equal(v2.cpu(), val) and torch.equal(l2.cpu(), lay), name


@pytest.mark.parametrize("prec", PRECS)
def test_a_batch_that_crosses_the_chunk_boundary_keeps_every_pair_its_bits(engines, prec):
    """16 x 16 pairs, three more than one chunk of the workspace rule holds: the pairs of the second chunk and those next to the boundary carry the bits
    they have alone."""
    from controlar_amd import _lib as L
    eng = engines[prec]
    chunk = eng.lib.car_debug_lpips_chunk_pairs(eng.mode, 16, 16)
    assert 5000 < chunk < 32768
    g = torch.Generator().manual_seed(77)
    pa, pb = torch.rand(3, 3, 16, 16, generator=g) * 2 - 1, torch.rand(3, 3, 16, 16, generator=g) * 2 - 1
    pb[2] = pa[2]
    alone = eng.lpips(pa, pb).cpu()
    assert alone[2] == 0 and alone[0] != alone[1] and alone[0] > 0
    B = chunk + 3
    idx = (torch.arange(B) % 3).cuda()
    got = eng.lpips(pa.cuda()[idx], pb.cuda()[idx])
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), alone[idx.cpu()])
    assert L.CAR_F32 == 0 and tuple(got.shape) == (B,)


@pytest.mark.parametrize("name", CASES)
def test_psnr_of_the_script_and_the_quantiser_in_front_of_it(engines, inputs, measured, name):
    z = np.load(os.path.join(GOLDEN, f"lpips_{name}.npz"))
    eng = engines["bf16"]
    a, b = inputs[name]
    u8 = eng.recon_to_u8(b)
    assert u8.dtype == torch.uint8 and torch.equal(u8.cpu(), R.recon_quantise_torch(b))
    got = eng.psnr(u8, a, data_range=1.0, a_map="div255", b_map="half").cpu().numpy()
    d = np.abs(got - z["psnr64"])
    rec = dict(case=name, psnr=got.tolist(), max_abs=float(d.max()), bound=16 * measured[name]["psnr_f32_vs_f64"])
    print("PSNR_PARITY " + json.dumps(rec))
    assert d.max() <= rec["bound"], rec
    rest, gt = R.restored_and_gt(u8.cpu(), a)                                      # the same number from tensors that are floats already
    assert torch.equal(eng.psnr(rest, gt).cpu(), torch.from_numpy(got))
    assert torch.equal(engines["fp32"].psnr(rest, gt).cpu(), torch.from_numpy(got))


def test_psnr_is_infinite_on_equal_images_and_follows_its_data_range(engines):
    eng = engines["fp32"]
    g = torch.Generator().manual_seed(5)
    x = torch.rand(3, 3, 40, 56, generator=g)
    inf = eng.psnr(x, x).cpu()
    assert torch.isinf(inf).all() and (inf > 0).all()
    u = torch.randint(0, 256, (2, 70000), generator=g).to(torch.uint8)             # more than one chunk of 8192 elements per image
    assert torch.isinf(eng.psnr(u, u)).all() and torch.isinf(eng.psnr(u, u.float() / 255.0, a_map="div255")).all()
    y = x + 0.125
    got = eng.psnr(x, y, data_range=2.0).cpu()
    want = R.psnr(x, y, data_range=2.0)
    assert torch.allclose(got, want, rtol=1e-12, atol=0)
    v = torch.randint(0, 256, (2, 70000), generator=g).to(torch.uint8)
    assert torch.allclose(eng.psnr(u, v, data_range=255.0, a_map="raw", b_map="raw").cpu(), R.psnr(u, v, data_range=255.0), rtol=1e-12, atol=0)
    with pytest.raises(RuntimeError, match="data_range"):
        eng.psnr(x, y, data_range=0.0)
    with pytest.raises(ValueError):
        eng.psnr(x, y[:, :, :-1])


def test_quantiser_is_bit_equal_to_torch_on_the_dense_grid(engines):
    grid = torch.arange(-144180, 144181, dtype=torch.float64) / 131072.0
    e32 = ((torch.arange(0, 257, dtype=torch.float64) - 128.0) / 127.5).to(torch.float32)
    near = torch.cat([e32, torch.nextafter(e32, torch.tensor(2.0)), torch.nextafter(e32, torch.tensor(-2.0))])
    x = torch.cat([grid.to(torch.float32), near, torch.tensor([-1.1, 1.1, -1.0, 1.0, 0.0, -0.0, 1e-30, -1e-30, 5.0, -5.0])])
    want = R.recon_quantise_torch(x)
    for eng in engines.values():
        got = eng.recon_to_u8(x)
        assert got.shape == x.shape and torch.equal(got.cpu(), want)
    x4 = x[:3 * 40 * 50].reshape(1, 3, 40, 50)
    assert torch.equal(engines["bf16"].recon_to_u8(x4).cpu(), want[:6000].reshape(1, 3, 40, 50))


def test_refusals_are_clean_errors(engines, mk):
    from controlar_amd import config as Cfg, synth
    from controlar_amd.engine import Engine
    eng = engines["bf16"]
    for shape in ((15, 40), (40, 15)):
        with pytest.raises(RuntimeError, match="at least 16 x 16"):
            eng.lpips(torch.zeros(1, 3, *shape), torch.zeros(1, 3, *shape))
    assert float(eng.lpips(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))[0]) == 0.0        # the boundary itself runs
    with pytest.raises(ValueError):
        eng.lpips(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 17))
    bare = Engine(Cfg.tiny_t2i(), "bf16")
    with pytest.raises(RuntimeError, match="no LPIPS weights"):
        bare.lpips(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))
    sd = synth.lpips_state_dict(mk.WEIGHT_SEED)
    for missing, stored in (("net.slice4.21.bias", "lpips.net.slice4.21.bias"), ("lin3.model.1.weight", "lpips.lin3.model.1.weight")):
        bare.close()
        bare = Engine(Cfg.tiny_t2i(), "bf16")                                                      # a fresh context: the tensor was never loaded
        with pytest.raises(RuntimeError, match=stored.replace(".", r"\.")):
            bare.load_lpips({k: v for k, v in sd.items() if k != missing})                         # finalize names the missing tensor
        with pytest.raises(RuntimeError, match="no LPIPS weights"):
            bare.lpips(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))                       # a partly loaded family does not run
    with pytest.raises(RuntimeError, match="lpips.features.1.weight: not a tensor of the LPIPS network"):
        bare.load_state_dict({"lpips.features.1.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match=r"expected \[1,128,1,1\]"):
        bare.load_state_dict({"lpips.lin1.model.1.weight": torch.zeros(1, 64, 1, 1)})
    bare.close()


def test_packed_cache_round_trip_reproduces_the_bits(engines, outputs, inputs, tmp_path):
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    path = str(tmp_path / "lpips.carpk").encode()
    for prec in PRECS:
        src = engines[prec]
        src._check(src.lib.car_export_packed(src._h, path), "car_export_packed")
        dst = Engine(Cfg.tiny_t2i(), prec)
        dst._check(dst.lib.car_import_packed(dst._h, path), "car_import_packed")
        val, lay = dst.lpips(*inputs["35x50"], want_layers=True)
        assert torch.equal(val.cpu(), outputs[prec, "35x50"][0]) and torch.equal(lay.cpu(), outputs[prec, "35x50"][1]), prec
        dst.close()


def test_reconstruction_quality_on_the_tiny_tokenizer(mk):
    """vq_encode -> vq_decode -> the script's quantiser -> PSNR against (x + 1) / 2 and LPIPS against x, all on the device; compare(p, p) is 0."""
    from controlar_amd import config as Cfg, synth
    from controlar_amd.engine import Engine
    from controlar_amd.metrics import LPIPS, PSNR, ReconstructionQuality
    cfg = Cfg.tiny_t2i()
    eng = Engine(cfg, "bf16")
    eng.load_state_dict(synth.vq_state_dict(cfg.vq, seed=2), finalize=True)
    rq = ReconstructionQuality(eng, synth.lpips_state_dict(mk.WEIGHT_SEED))
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).cuda()
    res = rq(x)
    assert all(t.is_cuda for t in res.values())
    assert res["tokens"].shape == (2, 16) and res["pixels"].shape == (2, 3, 64, 64) and res["u8"].dtype == torch.uint8
    assert torch.equal(res["tokens"], eng.vq_encode(x)) and torch.equal(res["pixels"], eng.vq_decode(res["tokens"], 4, 4))
    assert torch.equal(res["u8"], eng.recon_to_u8(res["pixels"]))
    # Engine.psnr of its own intermediate tensors, made as the script makes them: on the host, where / 255. is a true division (the device's element-wise
    # division by a constant multiplies by its reciprocal, which is not the script's rgb_restored)
    rest, gt = R.restored_and_gt(res["u8"].cpu(), x.cpu())
    assert torch.equal(res["psnr"], eng.psnr(rest, gt))
    assert torch.equal(res["lpips"], eng.lpips(x, res["pixels"]))
    assert res["psnr"].dtype == res["lpips"].dtype == torch.float64 and torch.isfinite(res["psnr"]).all() and (res["lpips"] > 0).all()
    same = rq.compare(res["pixels"], res["pixels"])
    assert (same["lpips"] == 0).all() and torch.isfinite(same["psnr"]).all()
    other = rq.compare(res["pixels"], x)
    assert torch.equal(other["lpips"], res["lpips"])                                               # lpips(a, b) == lpips(b, a)
    acc_l, acc_p = LPIPS(engine=eng), PSNR(engine=eng)
    assert torch.equal(acc_l.update(x, res["pixels"]), res["lpips"]) and acc_l.calculate() == float(res["lpips"].mean())
    assert torch.equal(acc_p.update(res["u8"], (x + 1.0) / 2.0), res["psnr"]) and acc_p.calculate() == float(res["psnr"].mean())
    eng.close()
