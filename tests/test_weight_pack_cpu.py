"""The host-side weight layouts (controlar_amd/csrc/weight_pack.h) against the PyTorch definition of each tensor, on the CPU: tests/weight_pack_check.cpp
is built with the host compiler, packs w[i] = i for the smallest case of every branch, and every line it prints is compared with numpy."""
import os
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("weight_pack") / "weight_pack_check")
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "weight_pack_check.cpp"), "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return {ln.split()[0]: np.array(ln.split()[1:], dtype=np.float32) for ln in out.splitlines()}


def iota(*shape, first=0):
    return np.arange(first, first + int(np.prod(shape)), dtype=np.float32).reshape(shape)


@pytest.mark.parametrize("Co,Ci,k,Kp", [(2, 3, 7, 160), (2, 3, 3, 32), (3, 32, 3, 288), (1, 4, 7, 224)])
def test_pack_conv(packed, Co, Ci, k, Kp):
    w = iota(Co, Ci, k, k)                                          # Conv2d weight, OIHW
    want = w.reshape(Co, Ci, k * k).transpose(0, 2, 1).reshape(Co, -1)
    want = np.pad(want, ((0, 0), (0, Kp - k * k * Ci)))
    assert np.array_equal(packed[f"conv_{Co}_{Ci}_{k}_{Kp}"], want.reshape(-1))


def test_pack_convT_phases(packed):
    Ci, Co = 4, 2
    w = iota(Ci, Co, 3, 3)                                          # ConvTranspose2d weight [Cin, Cout, 3, 3]
    # ConvTranspose2d(3, stride 2, padding 1): input i and kernel index k land on output 2*i - 1 + k.  Output 2*g + p therefore takes, at input offset d,
    # the kernel index k with 2*d - 1 + k == p.
    taps1 = {p: [(d, k) for d in (0, 1) for k in range(3) if 2 * d - 1 + k == p] for p in (0, 1)}
    assert taps1 == {0: [(0, 1)], 1: [(0, 2), (1, 0)]}
    img, off = packed["convT_phases_4_2"], 0
    assert img.size == 9 * Ci * Co
    x = torch.from_numpy(np.random.default_rng(0).integers(-3, 4, (1, Ci, 3, 5)).astype(np.float32))
    want = torch.nn.functional.conv_transpose2d(x, torch.from_numpy(w), stride=2, padding=1, output_padding=1)[0].numpy()
    xp = np.pad(x[0].numpy(), ((0, 0), (0, 1), (0, 1)))             # zero beyond the edge
    got = np.zeros_like(want)
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        taps = [(dy, dx, ky, kx) for dy, ky in taps1[py] for dx, kx in taps1[px]]
        line = packed[f"convT_phase_taps_{ph}"]
        assert line[0] == len(taps) == (1, 2, 2, 4)[ph] and line[1:].reshape(-1, 4).tolist() == [list(t) for t in taps]
        want_img = np.stack([w[:, :, ky, kx].T for _, _, ky, kx in taps], axis=1).reshape(Co, len(taps) * Ci)       # [Co][tap*Ci + ci]
        ph_img = img[off:off + want_img.size].reshape(Co, -1)
        off += want_img.size
        assert np.array_equal(ph_img, want_img)
        # and the four implicit GEMMs over the packed images are the transposed conv itself
        for gy in range(3):
            for gx in range(5):
                a = np.concatenate([xp[:, gy + dy, gx + dx] for dy, dx, _, _ in taps])
                got[:, 2 * gy + py, 2 * gx + px] = ph_img @ a
    assert off == img.size and np.array_equal(got, want)


@pytest.mark.parametrize("k", [2, 4])
def test_pack_convT_taps(packed, k):
    Ci, Co = 3, 2
    w = iota(Ci, Co, k, k)                                          # ConvTranspose2d(k, stride k) weight [Cin, Cout, k, k]
    want = w.reshape(Ci, Co, k * k).transpose(2, 1, 0).reshape(k * k * Co, Ci)
    assert np.array_equal(packed[f"convT_taps_{k}"], want.reshape(-1))
    assert np.array_equal(packed[f"convT_taps_bias_{k}"], np.tile(iota(Co), k * k))
    x = torch.from_numpy(np.random.default_rng(k).integers(-3, 4, (1, Ci, 2, 3)).astype(np.float32))
    ref = torch.nn.functional.conv_transpose2d(x, torch.from_numpy(w), stride=k)[0].numpy()
    y = (want @ x[0].numpy().reshape(Ci, -1)).reshape(k, k, Co, 2, 3)                      # [ky, kx, co, gy, gx] -> pixel (gy*k + ky, gx*k + kx)
    assert np.array_equal(y.transpose(2, 3, 0, 4, 1).reshape(Co, 2 * k, 3 * k), ref)


@pytest.mark.parametrize("rows", [16, 48])
def test_interleave16(packed, rows):
    cols = 5
    a, b = iota(rows, cols), iota(rows, cols, first=rows * cols)
    want = np.stack([a.reshape(-1, 16, cols), b.reshape(-1, 16, cols)], axis=1)             # [block][a | b][16][cols]
    assert np.array_equal(packed[f"interleave16_{rows}"], want.reshape(-1))


def test_pad_rows(packed):
    want = np.pad(iota(3, 27), ((0, 0), (0, 5)))
    assert np.array_equal(packed["pad_rows_3_27_32"], want.reshape(-1))
