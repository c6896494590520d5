"""Mints the CLIP-score fixtures: tests/golden/clip_{tiny,small,b32}.npz and clip_measured.json.  CPU only.

The arithmetic oracle is HF transformers' CLIPModel (given the same weights it computes what OpenAI's clip.load computes); the pixel oracle is
PIL + torch (controlar_amd.clip.preprocess_reference restates CLIP's preprocessor with them).  The files hold INPUTS AND OUTPUTS ONLY: the weights
are regenerated from controlar_amd.synth.clip_state_dict.  Per fixture:

  ids                  int64 [4, 77]: caption lengths 2 (start + end-of-text), 9, 40, 77
  pool_index           int64 [4]: the first position of the end-of-text id (what the tower pools)
  img0..img3           uint8 [H, W, 3] sources of different shapes
  pixel_values         fp32 [4, 3, n, n] (clip_tiny only: at 224 px four of them exceed the size limit of a committed file; the restatement that
  pixel_values_requant     produced them is pinned bit for bit against the tiny fixture by tests/test_clip_cpu.py) — without / with the script's
                           ToTensor / Normalize(0.5) / tensor2pil round trip in front
  img_emb, txt_emb, cos        HF fp32
  img_emb_bf16, txt_emb_bf16, cos_bf16    HF bf16 (model and pixel_values cast to bfloat16), widened to fp32

clip_measured.json: per fixture the largest |fp32 - fp64| of each output (the summation-order noise the fp32 GPU test multiplies by 16) and the mean
and largest |bf16 - fp32| (the reference's own bf16 round-off the bf16 GPU test is graded against).

    python tests/golden/make_clip_golden.py
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from controlar_amd import config as C, synth                              # noqa: E402
from controlar_amd.clip import preprocess_reference, requant_table        # noqa: E402

LENGTHS = [2, 9, 40, 77]
FIXTURES = {
    # name: (config, source sizes (H, W), seeds)
    "clip_tiny": (C.tiny_clip, [(40, 64), (64, 40), (37, 53), (48, 48)]),
    "clip_small": (C.small_clip, [(96, 128), (150, 113), (120, 120), (224, 224)]),
    "clip_b32": (C.clip_vit_b32, [(96, 128), (150, 113), (120, 120), (224, 224)]),
}


def hf_model(cfg, sd):
    from transformers import CLIPConfig, CLIPModel
    hc = CLIPConfig(
        text_config=dict(vocab_size=cfg.vocab_size, hidden_size=cfg.text_width, intermediate_size=cfg.text_mlp, num_hidden_layers=cfg.text_layers,
                         num_attention_heads=cfg.text_heads, max_position_embeddings=cfg.context_length, hidden_act="quick_gelu",
                         layer_norm_eps=cfg.ln_eps, projection_dim=cfg.proj_dim, eos_token_id=2, bos_token_id=0, pad_token_id=1),   # eos 2: pool at ids.argmax
        vision_config=dict(hidden_size=cfg.vision_width, intermediate_size=cfg.vision_mlp, num_hidden_layers=cfg.vision_layers,
                           num_attention_heads=cfg.vision_heads, image_size=cfg.image_size, patch_size=cfg.patch, hidden_act="quick_gelu",
                           layer_norm_eps=cfg.ln_eps, projection_dim=cfg.proj_dim),
        projection_dim=cfg.proj_dim)
    m = CLIPModel(hc).eval()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    return m


@torch.no_grad()
def run(model, dtype, pv, ids):
    m = model.to(dtype)
    img = m.get_image_features(pixel_values=pv.to(dtype)).pooler_output.to(torch.float32 if dtype != torch.float64 else torch.float64)
    txt = m.get_text_features(input_ids=ids).pooler_output.to(img.dtype)
    return img, txt, F.cosine_similarity(img, txt, dim=1)


def main():
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    tab = requant_table()
    measured = {}
    for name, (mk, sizes) in FIXTURES.items():
        cfg = mk()
        sd = synth.clip_state_dict(cfg)
        imgs = synth.clip_images(sizes)
        ids = synth.clip_tokens(len(LENGTHS), cfg, lengths=LENGTHS)
        pv = torch.stack([preprocess_reference(im, cfg.image_size) for im in imgs])
        pv_rq = torch.stack([preprocess_reference(tab[im.long()], cfg.image_size) for im in imgs])
        model = hf_model(cfg, sd)
        i64, t64, c64 = run(model, torch.float64, pv, ids)
        model = hf_model(cfg, sd)
        i32, t32, c32 = run(model, torch.float32, pv, ids)
        ib, tb, cb = run(model, torch.bfloat16, pv, ids)
        out = {"ids": ids.numpy(), "pool_index": (ids == cfg.eot_id).int().argmax(dim=-1).numpy().astype(np.int64),
               "img_emb": i32.numpy(), "txt_emb": t32.numpy(), "cos": c32.numpy(),
               "img_emb_bf16": ib.numpy(), "txt_emb_bf16": tb.numpy(), "cos_bf16": cb.numpy()}
        for i, im in enumerate(imgs):
            out[f"img{i}"] = im.numpy()
        if name == "clip_tiny":
            out["pixel_values"], out["pixel_values_requant"] = pv.numpy(), pv_rq.numpy()
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        d = lambda a, b: (a.double() - b.double()).abs()
        measured[name] = {
            "fp32_vs_fp64_max": {"img_emb": float(d(i32, i64).max()), "txt_emb": float(d(t32, t64).max()), "cos": float(d(c32, c64).max())},
            "bf16_vs_fp32_mean": {"img_emb": float(d(ib, i32).mean()), "txt_emb": float(d(tb, t32).mean()), "cos": float(d(cb, c32).mean())},
            "bf16_vs_fp32_max": {"img_emb": float(d(ib, i32).max()), "txt_emb": float(d(tb, t32).max()), "cos": float(d(cb, c32).max())},
            "scale": {"img_emb": float(i32.abs().mean()), "txt_emb": float(t32.abs().mean()), "cos": float(c32.abs().mean())},
        }
        print(name, os.path.getsize(path), json.dumps(measured[name]))
    with open(os.path.join(HERE, "clip_measured.json"), "w") as fh:
        json.dump(measured, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
