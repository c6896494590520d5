"""GPU timing of CLIPScorer.score (pixels in [-1,1] to cosines: quantiser, crop + LANCZOS, requant, CLIP preprocess, both towers, cosine) at full-size
ViT-B/32 with synthetic weights, next to HF transformers' CLIPModel forward on the same GPU where `transformers` imports.  Reported, not gated.  Not a test.

The HF side is timed WITHOUT preprocessing: it receives ready pixel_values [B,3,224,224] and ids on the device and runs get_image_features,
get_text_features and F.cosine_similarity in bf16; the script's PIL preprocessing (CPU, per image) is left out of its time, which favours it.  The HIP
side is timed with everything.  `--stages` adds the HIP path's own split (preprocess+image tower, text tower) timed the same way.

One process: both forms are warmed (2 calls each), then they alternate, `--repeats` rounds, each call timed on its own with device events on the
caller's stream; median, min and max per form.  Appends one line per form to <out-dir>/clip_time.jsonl.
usage: clip_time.py [--B 64] [--side 512] [--precision bf16|fp32] [--repeats 5] [--out-dir profiles]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-hf", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from controlar_amd import config as Cfg, synth
    from controlar_amd.clip import CLIPScorer
    cfg = Cfg.clip_vit_b32()
    sd = synth.clip_state_dict(cfg)
    s = CLIPScorer(cfg, sd, precision=a.precision, device="cuda")
    gen = torch.Generator().manual_seed(1)
    pixels = (torch.rand(a.B, 3, a.side, a.side, generator=gen) * 2 - 1).cuda()
    ids = synth.clip_tokens(a.B, cfg, seed=2).cuda()
    u8 = s.eval_image(pixels)
    forms = {"hip_score": lambda: s.score(pixels, ids),
             "hip_image_tower_with_preprocess": lambda: s.encode_image(u8, requant=True),
             "hip_text_tower": lambda: s.encode_text(ids)}
    hf_note = None
    if not a.no_hf:
        try:
            from transformers import CLIPConfig, CLIPModel
            hc = CLIPConfig(text_config=dict(eos_token_id=2), vision_config=dict(), projection_dim=cfg.proj_dim)       # the defaults are ViT-B/32
            dt = torch.bfloat16 if a.precision == "bf16" else torch.float32
            hf = CLIPModel(hc).eval()
            hf.load_state_dict(sd, strict=False)
            hf = hf.to(device="cuda", dtype=dt)
            pv = s.engine.clip_encode_image(u8, requant=True, want_pixel_values=True, want_embedding=False).to(dt)

            @torch.no_grad()
            def hf_forward():
                i = hf.get_image_features(pixel_values=pv).pooler_output
                t = hf.get_text_features(input_ids=ids).pooler_output
                return F.cosine_similarity(i.float(), t.float(), dim=1)
            forms["hf_forward_no_preprocess"] = hf_forward
        except Exception as exc:                                   # reported, not hidden: the HIP numbers stand alone then
            hf_note = f"{type(exc).__name__}: {exc}"
    for fn in forms.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    s.engine.check_errors()
    med = {k: statistics.median(v) for k, v in ms.items()}
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "clip_time.jsonl"), "a") as f:
        for k, v in ms.items():
            rec = dict(form=k, model="vit_b32_synthetic", precision=a.precision, B=a.B, side=a.side, ms=round(med[k], 3), ms_min=round(min(v), 3),
                       ms_max=round(max(v), 3), repeats=a.repeats, images_per_s=round(a.B / med[k] * 1e3, 1))
            if k == "hip_score" and "hf_forward_no_preprocess" in med:
                rec["ratio_hf_over_hip"] = round(med["hf_forward_no_preprocess"] / med[k], 3)
            if k == "hip_score" and hf_note:
                rec["hf_unavailable"] = hf_note
            line = json.dumps(rec)
            f.write(line + "\n")
            print("CLIP_TIME " + line, flush=True)
    s.engine.close()


if __name__ == "__main__":
    main()
