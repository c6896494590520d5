"""Functional restatement of the reference's reconstruction judges, torch only: LPIPS in inference (tokenizer/tokenizer_image/lpips.py:83-164) and the
PSNR and pixel quantiser of its tokenizer evaluation (tokenizer/tokenizer_image/reconstruction_vq_ddp.py:136-152).  The reference module itself is never
imported: it needs torchvision and its constructor fetches a checkpoint.  Every line cites the line it restates; tests/test_lpips_cpu.py holds the trunk
to the unmodified ``ControlNetHED_Apache2`` (the same thirteen convolutions), so the restatement is not one reading alone.

Weights: a dict with the keys of ``LPIPS().state_dict()`` (``controlar_amd.synth.lpips_state_dict``).  Runs in the dtype of its inputs (fp32 / fp64).
``bf16=True`` rounds every convolution's input and weight, and therefore every tap, to bf16: the emulation the GPU's bf16 mode is graded against.
``mutate`` names one deliberate misreading, for the tests that show each detail matters."""
import numpy as np
import torch
import torch.nn.functional as F

SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))       # lpips.py:128-137: features[0:4], [4:9], [9:16], [16:23], [23:30]
SHIFT = (-.030, -.088, -.188)                                             # lpips.py:102
SCALE = (.458, .448, .450)                                                # lpips.py:103
MUTATIONS = ("eps_inside_root", "norm_over_hw", "scale_before_shift", "tap_one_layer_early")


def _bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def scaling_layer(x, sd, mutate=None):
    shift = sd["scaling_layer.shift"] if "scaling_layer.shift" in sd else torch.tensor(SHIFT).view(1, 3, 1, 1)      # lpips.py:102
    scale = sd["scaling_layer.scale"] if "scaling_layer.scale" in sd else torch.tensor(SCALE).view(1, 3, 1, 1)      # lpips.py:103
    shift, scale = shift.to(x.dtype), scale.to(x.dtype)
    if mutate == "scale_before_shift":
        return x / scale - shift
    return (x - shift) / scale                                            # lpips.py:106


def vgg16_taps(x, sd, bf16=False, mutate=None, prefix="net."):
    """vgg16.forward (lpips.py:142-155): relu1_2, relu2_2, relu3_3, relu4_3, relu5_3."""
    taps, h = [], x
    for s, idx in enumerate(SLICES, 1):
        if s > 1:
            h = F.max_pool2d(h, kernel_size=2, stride=2)                  # features[4], [9], [16], [23]: MaxPool2d(2, 2), the first module of slice2..5
        early = None
        for n in idx:
            w, b = sd[f"{prefix}slice{s}.{n}.weight"].to(x.dtype), sd[f"{prefix}slice{s}.{n}.bias"].to(x.dtype)
            if bf16:
                h, w = _bf(h), _bf(w)
            early = h
            h = F.relu(F.conv2d(h, w, b, stride=1, padding=1))            # features[n], features[n + 1]: Conv2d(3x3, padding 1), ReLU
        tap = _bf(h) if bf16 else h                                       # the stored tap of the bf16 mode
        taps.append(early if mutate == "tap_one_layer_early" else tap)    # lpips.py:143-152
    return taps


def normalize_tensor(x, eps=1e-10, mutate=None):
    if mutate == "eps_inside_root":
        return x / torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True) + eps)
    if mutate == "norm_over_hw":
        return x / (torch.sqrt(torch.sum(x ** 2, dim=(2, 3), keepdim=True)) + eps)
    norm_factor = torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True))      # lpips.py:159
    return x / (norm_factor + eps)                                        # lpips.py:160


def lpips(a, b, sd, bf16=False, mutate=None):
    """LPIPS.forward (lpips.py:83-96) in .eval(): Dropout is the identity.  Returns (val [B], layers [B,5])."""
    in0, in1 = scaling_layer(a, sd, mutate), scaling_layer(b, sd, mutate)             # lpips.py:84
    outs0, outs1 = vgg16_taps(in0, sd, bf16, mutate), vgg16_taps(in1, sd, bf16, mutate)      # lpips.py:85
    if bf16:                                                              # the head of the bf16 mode computes in fp32 from the bf16 taps
        outs0, outs1 = [t.float() for t in outs0], [t.float() for t in outs1]
    res = []
    for kk in range(5):
        f0, f1 = normalize_tensor(outs0[kk], mutate=mutate), normalize_tensor(outs1[kk], mutate=mutate)      # lpips.py:89
        diff = (f0 - f1) ** 2                                             # lpips.py:90
        lin = sd[f"lin{kk}.model.1.weight"].to(diff.dtype)
        res.append(F.conv2d(diff, lin).mean([2, 3], keepdim=True))        # lpips.py:92, :114 (1x1, no bias), :163-164
    val = res[0].clone()
    for l in range(1, 5):
        val += res[l]                                                     # lpips.py:93-95
    return val.flatten(), torch.cat(res, dim=1).flatten(1)


def recon_quantise(x):
    """torch.clamp(127.5 * x + 128.0, 0, 255).to(uint8) (reconstruction_vq_ddp.py:144) step by step in numpy fp32: a product, a sum, a clamp, a truncation."""
    v = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32)
    v = (np.float32(127.5) * v).astype(np.float32)
    v = (v + np.float32(128.0)).astype(np.float32)
    return torch.from_numpy(np.trunc(np.clip(v, np.float32(0), np.float32(255))).astype(np.uint8))


def recon_quantise_torch(x):
    return torch.clamp(127.5 * x + 128.0, 0, 255).to(torch.uint8)         # reconstruction_vq_ddp.py:144, val_ddp.py:138


def restored_and_gt(u8, x):
    """rgb_restored = sample.astype(np.float32) / 255. (:151) and rgb_gt = (x + 1.0) / 2.0 (:136), both fp32."""
    return u8.to(torch.float32) / 255.0, (x.to(torch.float32) + 1.0) / 2.0


def psnr(a, b, data_range=1.0, dtype=torch.float64):
    """skimage.metrics.peak_signal_noise_ratio per image (reconstruction_vq_ddp.py:152): 10 log10(data_range^2 / mean((a - b)^2)); skimage computes it in
    fp64, ``dtype=torch.float32`` gives the yardstick for the deviation."""
    a, b = a.to(dtype).flatten(1), b.to(dtype).flatten(1)
    mse = ((a - b) ** 2).mean(dim=1)
    return 10 * torch.log10(torch.tensor(data_range, dtype=dtype) ** 2 / mse)
