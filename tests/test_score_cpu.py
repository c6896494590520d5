"""CPU side of car_score: both built libraries export the two new symbols, controlar_amd._lib binds them with the header's argument lists, the fp64
reference of the tests agrees with torch's cross_entropy, and generate.score_loss is the reference's `valid` reduction (gpt_t2i.py:476-481)."""
import ctypes as C
import os
import re

import numpy as np
import torch

from controlar_amd import _lib as L
from tests.score_ref import nll_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_both_libraries_export_score_entries():
    for path in (L.LIB_PATH, L.DEV_LIB_PATH):
        lib = C.CDLL(path)
        for name in ("car_score", "car_debug_score_rows"):
            assert hasattr(lib, name), (path, name)
    assert L.load().car_abi_version() == 2 and L.CAR_ABI_VERSION == 2          # additive: the ABI version stays


def _header_args(name):
    hdr = open(os.path.join(ROOT, "include", "controlar_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, name
    args = [re.sub(r"/\*.*?\*/", "", a, flags=re.S).strip() for a in m.group(1).split(",")]

    def ctype(a):
        if "car_sampling" in a:
            return C.POINTER(L.CarSampling)
        if "*" in a:
            return C.c_void_p
        assert a.startswith("int32_t"), a
        return C.c_int32
    return [ctype(a) for a in args]


def test_lib_binds_the_headers_argument_lists():
    for name, n in (("car_score", 12), ("car_debug_score_rows", 12)):
        want = _header_args(name)
        res, got = L.SYMBOLS[name]
        assert res is C.c_int and len(want) == n
        assert got == want, (name, got, want)


def test_score_ref_matches_torch_cross_entropy():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "tiny_canny_cfg1.npz"))
    logits, tokens = torch.from_numpy(gold["logits"]).double(), torch.from_numpy(gold["tokens"]).long()
    want = torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), tokens.reshape(-1), reduction="none").reshape(tokens.shape)
    got = nll_ref(gold["logits"], gold["tokens"])
    assert got.dtype == np.float64 and got.shape == tuple(tokens.shape)
    np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=1e-12)


def test_score_loss_is_the_references_valid_reduction():
    from controlar_amd.generate import score_loss
    g = torch.Generator().manual_seed(3)
    B, N, V = 5, 7, 11
    logits = torch.randn(B, N, V, generator=g, dtype=torch.float64) * 3
    targets = torch.randint(0, V, (B, N), generator=g)
    loss_all = torch.nn.functional.cross_entropy(logits.view(-1, V), targets.view(-1), reduction="none")          # gpt_t2i.py:477
    nll = loss_all.view(B, N)
    for valid in (torch.tensor([1, 0, 1, 1, 0]), torch.ones(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int64)):
        valid_all = valid[:, None].repeat(1, targets.shape[1]).view(-1)                                           # gpt_t2i.py:478
        want = (loss_all * valid_all).sum() / max(valid_all.sum(), 1)                                             # gpt_t2i.py:479
        got = score_loss(nll, valid)
        assert got.dim() == 0 and got.dtype == torch.float64
        np.testing.assert_allclose(float(got), float(want), rtol=1e-14, atol=0)
    assert float(score_loss(nll, torch.zeros(B))) == 0.0
    np.testing.assert_allclose(float(score_loss(nll.float())), float(torch.nn.functional.cross_entropy(logits.view(-1, V), targets.view(-1))), rtol=1e-6)
