"""car_resize on the GPU (pytest -m gpu) against the fixtures minted from Pillow (tests/golden/make_resize_golden.py): the resampler is integer
arithmetic on host-computed tables, so every comparison of the uint8 result is np.array_equal, and the float epilogues (one fp32 expression with a
correctly rounded division, rounded once) are compared bit for bit as well; the torch side of those comparisons is evaluated on the CPU, where
x / 255 is a true division.

The vertical pass and the passes that write the caller's tensors directly have one form.  The horizontal pass into the intermediate has two that give
the same bits: LDS-staged (a block stages the source span of 64 output pixels for up to 16 rows, 48 KiB at most) and the byte gather it falls back
to when a tile's span does not fit.  Every fixture case with both passes takes the LDS-staged form, the 200 x 300 Lanczos case (ksize 77, span 300
pixels, 16 rows per block) and the small ones alike; vonly_70x50, honly_70x50 and copy_64x48 launch no intermediate pass at all.  The wide cases of
test_wide_rows_* are generated from a seed and graded against the minter's NumPy restatement (which test_resize_cpu.py pins to Pillow): 3 x 1500
and 3 x 6000 -> 2 x 64 stay LDS-staged with 10 and 2 rows per block, 3 x 17000 -> 2 x 64 (span 17000 pixels = 51 KB) takes the byte gather.
test_both_horizontal_forms_give_the_same_bits forces the byte gather in the development build and compares it with the shipped choice."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILTERS = {"lanczos": 1, "bilinear": 2, "bicubic": 3, "box": 4, "hamming": 5}
CASES = ["down_53x37", "up_l_31x20", "half_64x64", "vonly_70x50", "honly_70x50", "copy_64x48", "box_60x48", "box_96x96", "deep_l_200x300",
         "up_33x47", "tiny_2x3", "one_1x1", "sq_40x56"]
PRECS = ["fp32", "bf16"]


def _z(name):
    return np.load(os.path.join(GOLDEN, f"resize_{name}.npz"))


def _geom(z):
    Ho, Wo = (int(v) for v in z["out_size"])
    return Ho, Wo, (tuple(float(v) for v in z["box"]) if bool(z["has_box"]) else None)


def _stream():
    return C.c_void_p(int(torch.cuda.current_stream().cuda_stream))


def _raw(eng, x, Ho, Wo, f, box=None, out=True, control=False, fl=None, C_=None, B_=None):
    """car_resize through the C ABI on x uint8 [B,H,W,C] (cuda): (rc, out, control, float) with None where not asked for."""
    B, H, W, ch = x.shape
    o = torch.full((B, Ho, Wo, ch), 77, dtype=torch.uint8, device="cuda") if out and Ho > 0 and Wo > 0 else None
    c = torch.empty(B, 3, Ho, Wo, dtype=eng.dtype, device="cuda") if control else None
    f32 = torch.empty(B, ch, Ho, Wo, dtype=torch.float32, device="cuda") if fl is not None else None
    cbox = None if box is None else (C.c_float * 4)(*box)
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    rc = eng.lib.car_resize(eng._h, p(x), B if B_ is None else B_, H, W, ch if C_ is None else C_, Ho, Wo, f, cbox, p(o), p(c), p(f32), fl or 0, _stream())
    return rc, o, c, f32


@pytest.fixture(scope="module")
def engines():
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    e = {prec: Engine(Cfg.tiny_t2i(), prec) for prec in PRECS}
    yield e
    for v in e.values():
        v.close()


def _img(z, kind):
    x = torch.from_numpy(z[f"x_{kind}"])
    return (x[:, :, None] if x.dim() == 2 else x)[None].contiguous()          # [1,H,W,C]


@pytest.fixture(scope="module")
def outputs(engines):
    """every case, filter and input once per mode, with both epilogue tensors (norm = 1): shared by the tests below and left unchanged"""
    res = {}
    for prec in PRECS:
        for name in CASES:
            z = _z(name)
            Ho, Wo, box = _geom(z)
            for kind in ("noise", "binary"):
                x = _img(z, kind).cuda()
                for fname, f in FILTERS.items():
                    rc, o, c, fl = _raw(engines[prec], x, Ho, Wo, f, box, control=True, fl=1)
                    assert rc == 0, engines[prec].lib.car_last_error(engines[prec]._h)
                    res[prec, name, kind, fname] = (o, c, fl)
    torch.cuda.synchronize()
    return {k: tuple(t.cpu() for t in v) for k, v in res.items()}


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("prec", PRECS)
def test_output_is_pillows_bit_for_bit(outputs, prec, name):
    z = _z(name)
    for kind in ("noise", "binary"):
        for fname in FILTERS:
            want = z[f"{kind}_{fname}"]
            got = outputs[prec, name, kind, fname][0].numpy()[0]
            got = got[:, :, 0] if want.ndim == 2 else got
            assert got.shape == want.shape and np.array_equal(got, want), (kind, fname, int((got != want).sum()))


@pytest.mark.parametrize("prec", PRECS)
def test_control_and_float_outputs_are_the_stated_expressions(outputs, engines, prec):
    from controlar_amd.condition import DepthEstimator
    dt = engines[prec].dtype
    for name in CASES:
        for fname in ("bicubic", "box"):
            o, c, fl = outputs[prec, name, "noise", fname]
            nchw = o.permute(0, 3, 1, 2).contiguous()                                  # uint8 [1,C,Ho,Wo]
            want = (2 * (nchw.float() / 255 - 0.5)).to(dt)
            assert c.dtype == dt and tuple(c.shape) == (1, 3) + tuple(nchw.shape[2:])
            for ch in range(3):
                assert torch.equal(c[:, ch], want[:, ch if nchw.shape[1] == 3 else 0]), (name, fname, ch)      # C = 1 is replicated
            assert fl.dtype == torch.float32 and torch.equal(fl, DepthEstimator.preprocess(nchw)), (name, fname)     # norm = 1
    eng = engines[prec]
    for name in ("down_53x37", "up_l_31x20", "copy_64x48"):                              # norm = 0: the raw value
        z = _z(name)
        Ho, Wo, box = _geom(z)
        rc, o, _, fl = _raw(eng, _img(z, "noise").cuda(), Ho, Wo, 3, box, fl=0)
        assert rc == 0 and torch.equal(fl.cpu(), o.cpu().permute(0, 3, 1, 2).float())


@pytest.mark.parametrize("prec", PRECS)
def test_a_batch_equals_its_single_image_calls(outputs, engines, prec):
    eng = engines[prec]
    for name in ("down_53x37", "up_l_31x20", "box_60x48", "vonly_70x50", "honly_70x50", "copy_64x48"):
        z = _z(name)
        Ho, Wo, box = _geom(z)
        a, b = _img(z, "noise"), _img(z, "binary")
        batch = torch.cat([a, b, a.flip(1)]).contiguous().cuda()
        for fname in ("lanczos", "bicubic"):
            rc, o, c, fl = _raw(eng, batch, Ho, Wo, FILTERS[fname], box, control=True, fl=1)
            assert rc == 0
            for i, kind in ((0, "noise"), (1, "binary")):
                so, sc, sf = outputs[prec, name, kind, fname]
                assert torch.equal(o[i].cpu(), so[0]) and torch.equal(c[i].cpu(), sc[0]) and torch.equal(fl[i].cpu(), sf[0]), (name, fname, i)
            rc, o2, _, _ = _raw(eng, batch[2:3].contiguous(), Ho, Wo, FILTERS[fname], box)
            assert rc == 0 and torch.equal(o2[0], o[2]), (name, fname)


@pytest.mark.parametrize("prec", PRECS)
def test_second_call_and_epilogue_only_call_give_the_same_bits(outputs, engines, prec):
    eng = engines[prec]
    for name in ("box_96x96", "deep_l_200x300", "honly_70x50", "copy_64x48"):
        z = _z(name)
        Ho, Wo, box = _geom(z)
        x = _img(z, "noise").cuda()
        for fname in ("lanczos", "hamming"):
            want = outputs[prec, name, "noise", fname]
            for _ in range(2):                                                            # the second of these reuses the cached tables
                rc, o, c, fl = _raw(eng, x, Ho, Wo, FILTERS[fname], box, control=True, fl=1)
                assert rc == 0 and all(torch.equal(t.cpu(), w) for t, w in zip((o, c, fl), want)), (name, fname)
            rc, o, c, fl = _raw(eng, x, Ho, Wo, FILTERS[fname], box, out=False, control=True, fl=1)      # out_hwc = NULL
            assert rc == 0 and o is None and torch.equal(c.cpu(), want[1]) and torch.equal(fl.cpu(), want[2]), (name, fname)


def _minter():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_resize_golden", os.path.join(GOLDEN, "make_resize_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("W", [1500, 6000, 17000])
def test_wide_rows_on_both_sides_of_the_lds_limit(engines, W):
    """3 x W x 3 -> 2 x 64: the source span of the one 64-pixel tile is the whole row.  1500 and 6000 pixels fit in LDS (10 and 2 rows per block),
    17000 do not (51 KB): that call takes the byte-gather form of the horizontal pass."""
    mk = _minter()
    x = np.random.default_rng(W).integers(0, 256, (3, W, 3), dtype=np.uint8)
    xg = torch.from_numpy(x)[None].cuda()
    for fname in ("box", "lanczos"):
        want = mk.resize(x, (64, 2), FILTERS[fname])
        for prec in PRECS:
            rc, o, _, _ = _raw(engines[prec], xg, 2, 64, FILTERS[fname])
            assert rc == 0 and np.array_equal(o.cpu().numpy()[0], want), (fname, prec)


def test_both_horizontal_forms_give_the_same_bits(outputs, monkeypatch):
    """The development build reads CAR_RESIZE_NO_LDS per call: with it the intermediate comes from the byte-gather form for every case."""
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    eng = Engine(Cfg.tiny_t2i(), "bf16", dev=True)
    for forced in (True, False):
        if forced:
            monkeypatch.setenv("CAR_RESIZE_NO_LDS", "1")
        else:
            monkeypatch.delenv("CAR_RESIZE_NO_LDS")
        for name in CASES:
            z = _z(name)
            Ho, Wo, box = _geom(z)
            for kind in ("noise", "binary"):
                x = _img(z, kind).cuda()
                for fname in ("lanczos", "bicubic", "box"):
                    rc, o, _, _ = _raw(eng, x, Ho, Wo, FILTERS[fname], box)
                    assert rc == 0 and torch.equal(o.cpu(), outputs["bf16", name, kind, fname][0]), (forced, name, kind, fname)
    eng.close()


def test_engine_resize_and_the_resizer_return_in_kind(outputs, engines):
    from PIL import Image
    from controlar_amd.condition import BICUBIC, LANCZOS, Resizer
    eng = engines["bf16"]
    z = _z("box_60x48")
    Ho, Wo, box = _geom(z)
    x = torch.from_numpy(z["x_noise"])
    out, ctrl, fl = eng.resize(x, (Wo, Ho), "lanczos", box=box, want_control=True, want_float="norm")
    assert out.is_cuda and tuple(out.shape) == (Ho, Wo, 3) and np.array_equal(out.cpu().numpy(), z["noise_lanczos"])
    assert torch.equal(ctrl.cpu(), outputs["bf16", "box_60x48", "noise", "lanczos"][1]) and torch.equal(fl.cpu(), outputs["bf16", "box_60x48", "noise", "lanczos"][2])
    assert np.array_equal(eng.resize(x[None], (Wo, Ho), 3, box=box).cpu().numpy()[0], z["noise_bicubic"])
    zl = _z("up_l_31x20")
    g = eng.resize(torch.from_numpy(zl["x_noise"]), (64, 48))                              # [H,W] in, [Ho,Wo] out, BICUBIC by default
    assert tuple(g.shape) == (48, 64) and np.array_equal(g.cpu().numpy(), zl["noise_bicubic"])
    with pytest.raises(ValueError, match="unknown resample filter"):
        eng.resize(x, (8, 8), "cubic")
    with pytest.raises(TypeError, match="8-bit"):
        eng.resize(x.float(), (8, 8))
    r = Resizer()
    pil = r(Image.fromarray(z["x_noise"]), (Wo, Ho), LANCZOS, box)
    assert isinstance(pil, Image.Image) and pil.mode == "RGB" and np.array_equal(np.asarray(pil), z["noise_lanczos"])
    pl = r(Image.fromarray(zl["x_binary"]), (64, 48))
    assert pl.mode == "L" and np.array_equal(np.asarray(pl), zl["binary_bicubic"])
    arr = r(z["x_binary"], (Wo, Ho), BICUBIC, box)
    assert isinstance(arr, np.ndarray) and np.array_equal(arr, z["binary_bicubic"])
    t = r(x, (Wo, Ho), resample=BICUBIC, box=box)
    assert torch.is_tensor(t) and not t.is_cuda and np.array_equal(t.numpy(), z["noise_bicubic"])
    with pytest.raises(RuntimeError, match="HWC3"):
        r(np.zeros((4, 4, 4), np.uint8), (2, 2))
    r._eng.close()


def test_reference_helpers_run_on_the_gpu(tmp_path):
    from PIL import Image
    from controlar_amd import condition as K
    z = _z("crop_150x210")
    for kind in ("noise", "binary"):
        pil = K.center_crop_arr(Image.fromarray(z[f"x_{kind}"]), 32)
        assert isinstance(pil, Image.Image) and np.array_equal(np.asarray(pil), z[f"crop_{kind}"])
    assert np.array_equal(K.center_crop_arr(z["x_noise"], 32), z["crop_noise"])
    assert np.array_equal(K.center_crop_arr(torch.from_numpy(z["x_noise"]), 32).numpy(), z["crop_noise"])
    # resize_image_to_16_multiple: both branches, from a path as the reference takes it and from a loaded image
    zs = _z("down_53x37")
    path = str(tmp_path / "photo.png")
    Image.fromarray(zs["x_noise"]).save(path)                                            # 53 x 37 (H x W)
    a = K.resize_image_to_16_multiple(path, "canny")
    assert isinstance(a, Image.Image) and a.size == (48, 64)
    assert np.array_equal(np.asarray(a), np.asarray(Image.open(path).resize((48, 64))))
    d = K.resize_image_to_16_multiple(zs["x_noise"], condition_type="depth")
    assert isinstance(d, np.ndarray) and d.shape == (64, 64, 3) and np.array_equal(d, np.asarray(Image.fromarray(zs["x_noise"]).resize((64, 64))))
    same = K.resize_image_to_16_multiple(_z("half_64x64")["x_noise"])
    assert np.array_equal(same, _z("half_64x64")["x_noise"])                              # already a multiple of 16: a copy
    # resize_image: LANCZOS when enlarging (k > 1), BOX when shrinking
    zq = _z("sq_40x56")
    assert np.array_equal(K.resize_image(zq["x_noise"], 64), zq["noise_lanczos"])          # k = 1.6: 64 x 64
    zb = _z("box_96x96")
    down = K.resize_image(zb["x_noise"], 64)                                              # k = 2/3: 64 x 64
    assert np.array_equal(down, np.asarray(Image.fromarray(zb["x_noise"]).resize((64, 64), Image.BOX)))
    assert not np.array_equal(down, np.asarray(Image.fromarray(zb["x_noise"]).resize((64, 64), Image.LANCZOS)))


def test_depth_preprocess_with_size_feeds_the_model_what_pil_would():
    from controlar_amd import config as Cfg, synth
    from controlar_amd.condition import DepthEstimator
    cfg = Cfg.tiny_dpt()
    model = DepthEstimator(cfg, synth.dpt_state_dict(cfg, 13))
    z = _z("sq_40x56")
    x = torch.from_numpy(z["x_noise"]).permute(2, 0, 1)[None].contiguous()               # uint8 [1,3,40,56]
    pv = DepthEstimator.preprocess(x, size=(64, 64))
    resized = torch.from_numpy(z["noise_bicubic"]).permute(2, 0, 1)[None].contiguous()    # what PIL's bicubic resize makes of it
    want = DepthEstimator.preprocess(resized)
    assert pv.is_cuda and pv.dtype == torch.float32 and torch.equal(pv.cpu(), want)
    assert torch.equal(model(pixel_values=pv).predicted_depth.cpu(), model(pixel_values=want).predicted_depth)
    from PIL import Image
    assert torch.equal(DepthEstimator.preprocess(Image.fromarray(z["x_noise"]), size=(64, 64)).cpu(), want)
    model._eng.close()


def test_demo_model_runs_the_librarys_own_extractors():
    from PIL import Image
    from controlar_amd import config as Cfg, synth
    from controlar_amd.condition import DepthEstimator, HEDdetector, LineArt
    from controlar_amd.demo import Model
    hed = HEDdetector().load_state_dict(synth.hed_state_dict(11))
    la = LineArt().load_state_dict(synth.lineart_state_dict(11))
    cfg = Cfg.tiny_dpt()
    dpt = DepthEstimator(cfg, synth.dpt_state_dict(cfg, 13))
    z = _z("sq_40x56")
    photo = Image.fromarray(z["x_noise"])
    m = Model(hed=hed, lineart=la, depth=dpt)
    for name in ("HED", "Lineart", "Depth"):
        out = m._preprocess(name, photo, image_resolution=64, detect_resolution=64)
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == (64, 64), name
    # HED at detect resolution 64: resize_image makes 64 x 64 with LANCZOS (k = 1.6), then the detector
    resized = torch.from_numpy(z["noise_lanczos"]).permute(2, 0, 1)[None].contiguous()
    want = hed(resized.cuda())[0].clamp(0, 255).to(torch.uint8).cpu().numpy()
    assert np.array_equal(m._preprocess("HED", photo, detect_resolution=64), want)
    # the Canny branch resizes on the GPU now: the same bits as PIL in front of car_canny
    edges = m._preprocess("Canny", photo, detect_resolution=64)
    assert np.array_equal(edges, m._canny(z["noise_lanczos"]))
    # without the new arguments everything raises as before
    for name in ("HED", "Lineart", "Depth"):
        with pytest.raises(RuntimeError, match="needs the preprocessor callable"):
            Model()._preprocess(name, photo, detect_resolution=64)
    with pytest.raises(RuntimeError, match="needs the preprocessor callable"):
        Model(hed=hed)._preprocess("Depth", photo, detect_resolution=64)
    for e in (hed, la, dpt, m._canny):
        e._eng.close()


def test_refusals_are_clean_and_leave_the_context_usable(outputs, engines):
    eng = engines["bf16"]
    z = _z("down_53x37")
    Ho, Wo, _ = _geom(z)
    x = _img(z, "noise").cuda()
    err = lambda: eng.lib.car_last_error(eng._h).decode()

    def still_fine():
        rc, o, _, _ = _raw(eng, x, Ho, Wo, 3)
        assert rc == 0 and torch.equal(o.cpu(), outputs["bf16", "down_53x37", "noise", "bicubic"][0])

    rc = _raw(eng, x, Ho, Wo, 3, out=False)[0]
    assert rc != 0 and "all NULL" in err()
    still_fine()
    x4 = torch.zeros(1, 8, 8, 4, dtype=torch.uint8, device="cuda")
    rc = _raw(eng, x4, 4, 4, 3)[0]
    assert rc != 0 and "HWC3" in err()
    x2 = torch.zeros(1, 8, 8, 2, dtype=torch.uint8, device="cuda")
    rc = _raw(eng, x2, 4, 4, 3)[0]
    assert rc != 0 and "C must be 1 (L) or 3 (RGB)" in err()
    still_fine()
    for Ho_, Wo_ in ((0, 16), (16, 0), (-1, 16)):
        rc = _raw(eng, x, Ho_, Wo_, 3, out=False, control=False)[0]
        assert rc != 0 and "sizes must be positive" in err()
    rc = _raw(eng, x, Ho, Wo, 3, B_=0)[0]
    assert rc != 0 and "sizes must be positive" in err()
    still_fine()
    rc = _raw(eng, x, Ho, Wo, 0)[0]
    assert rc != 0 and "NEAREST" in err()
    for f in (6, -3, 99):
        rc = _raw(eng, x, Ho, Wo, f)[0]
        assert rc != 0 and "unknown filter" in err()
    still_fine()
    for box in ((5.0, 0.0, 5.0, 53.0), (9.0, 0.0, 4.0, 53.0), (0.0, 20.0, 37.0, 20.0)):
        rc = _raw(eng, x, Ho, Wo, 3, box)[0]
        assert rc != 0 and "box is empty" in err(), box
    for box in ((-1.0, 0.0, 37.0, 53.0), (0.0, 0.0, 37.5, 53.0), (0.0, 0.0, 37.0, 54.0), (0.0, -0.25, 37.0, 53.0), (float("nan"), 0.0, 37.0, 53.0)):
        rc = _raw(eng, x, Ho, Wo, 3, box)[0]
        assert rc != 0 and ("outside the image" in err() or "box is empty" in err()), box
    still_fine()
    with pytest.raises(RuntimeError, match="NEAREST"):
        eng.resize(x, (Wo, Ho), "nearest")
    still_fine()
