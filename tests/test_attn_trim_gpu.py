"""The edge-block trim of the bf16 decode attention (decode2.hip dec_attn2_kernel: the first and the last 32-position block of a sequence load only the lanes
that hold an attended row) must not change a bit: at kernel level against the untrimmed load form, a poisoned cache and an fp64 softmax
(experiments/attn_edge_check.hip), and end to end against CAR_ATTN_NO_TRIM on the development library."""
import os
import shutil
import subprocess

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "controlar_amd", "csrc")


def _build(name, extra=()):      # as tests/test_kernels_gpu.py builds its harnesses: one hipcc line, rebuilt when a source is newer
    src = os.path.join(ROOT, "experiments", name + ".hip")
    exe = os.path.join(ROOT, "experiments", name)
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, *extra, src, "-o", exe], check=True, capture_output=True, timeout=900)
    return exe


def test_edge_blocks_kernel_level():
    """experiments/attn_edge_check.hip: H = 2, SA = 160, T = 40; 40 left-padded sequences (jmin 0..39) and the same without a mask; pos = 40..103;
    2 / 4 / 16 waves, both register-set forms, nsplit 1 and 4 + combine.  (a) trimmed == no_trim bit for bit; (b) rows outside [jmin, pos] zero vs
    +-3.0e38: equal bits, for both load forms; (c) within 2e-2 of an fp64 softmax."""
    exe = _build("attn_edge_check")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout[-3000:] + out.stderr[-1000:]
    assert "FAIL" not in out.stdout


def test_two_chains_tokens_and_logits_equal_with_and_without_the_trim(monkeypatch):
    """GPT-B, 384 images = two chains of 192 (dec_attn2_kernel<4, 0, 0>, the headline's attention form), 47 free-running decode steps over left-padded
    captions: positions 120..166 cross a block boundary at both edges for most sequences.  Tokens and the last step's logits with CAR_ATTN_NO_TRIM
    (edge blocks load every lane, the kernel as it was) must equal the default's bit for bit."""
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    cfg = C.b_t2i(256, adapter_size="small", condition_type="canny")
    gsd, _ = synth.path_state_dicts(cfg, seed=0)
    B, n_new = 384, 48
    img = synth.canny_like_control(B, 256, 256); emb, mask = synth.text_embeddings(B, cfg.gpt.cls_token_num, cfg.gpt.caption_dim)
    eng = Engine(cfg, "bf16", dev=True); eng.load_state_dict(gsd); eng.finalize()      # the switch exists only in the development build of the library
    eng.encode_control(img.cuda())
    monkeypatch.setenv("CAR_ATTN_NO_TRIM", "1")
    want, want_l = eng.generate(emb.cuda(), n_new, mask.cuda(), cfg_scale=1.0, return_logits=True)
    st = eng.stats()
    assert st["graph_used"] and st["dev_knobs_active"] >= 1, st
    want, want_l = want.cpu(), want_l[:, -1].cpu()      # [B, V]: the last step's logits
    monkeypatch.delenv("CAR_ATTN_NO_TRIM")
    got, got_l = eng.generate(emb.cuda(), n_new, mask.cuda(), cfg_scale=1.0, return_logits=True)
    assert eng.stats()["graph_used"]
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got_l[:, -1].cpu(), want_l)
    eng.close()
