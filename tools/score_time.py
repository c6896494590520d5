"""GPU timing of Engine.score (car_score, one parallel pass) next to Engine.generate(forced_tokens=..., return_logits=True), the token loop that was the
only way to get teacher-forced logits before: the same prompts, control and tokens.  Reported, not gated.  Not a test.

One process per configuration: both forms are warmed (2 calls each; the token loop's warm-up also captures its graph), then they alternate, `--repeats`
rounds, each call timed on its own with device events on the caller's stream; median, min and max per form.  The pass's arithmetic is counted as
2 * rows * (the layers' linear parameters) + the causal attention + 2 * B * N * mult * V * D for the fused projection; `mfma_fraction` is that count over the
median time and the dense matrix peak of the mode (--peak-tflops, default 2500 for bf16 and 157 for fp32 on one MI355X).
Writes <out-dir>/score_time.jsonl (appends one line per form).
usage: score_time.py --model b|xl [--precision bf16|fp32] [--B 8] [--cfg-scale 4.0] [--repeats 5] [--out-dir profiles]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pass_flops(g, B, N, mult, Tv):
    Ts = Tv + N - 1
    rows = B * mult * Ts
    lin = g.n_layer * (4.0 * g.dim * g.dim + 3.0 * g.dim * g.ffn_hidden)
    attn = g.n_layer * B * mult * 2.0 * 2.0 * g.dim * Ts * Ts / 2.0          # QK^T and PV, causal half
    return 2.0 * rows * lin + attn + 2.0 * B * N * mult * g.vocab_size * g.dim


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("b", "xl"), default="b")
    ap.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--cfg-scale", type=float, default=4.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--peak-tflops", type=float, default=0.0)
    ap.add_argument("--score-only", action="store_true", help="skip the token loop (kernel traces of the pass alone); nothing is written")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    from controlar_amd import config as Cfg, synth
    from controlar_amd.engine import Engine, first_valid_position
    cfg = Cfg.b_t2i(256, "small", "canny") if a.model == "b" else Cfg.xl_t2i(1024, "small", "canny")
    g = cfg.gpt
    N = g.block_size; side = int(N ** 0.5) * 16
    gsd, _ = synth.path_state_dicts(cfg, seed=0)
    eng = Engine(cfg, a.precision); eng.load_state_dict(gsd); eng.finalize()
    img = synth.canny_like_control(a.B, side, side).cuda()
    emb, mask = synth.text_embeddings(a.B, g.cls_token_num, g.caption_dim)
    fv = first_valid_position(mask)
    emb, mask = emb.cuda(), mask.cuda()
    tokens = torch.randint(0, g.vocab_size, (a.B, N), generator=torch.Generator().manual_seed(1), dtype=torch.int32).cuda()
    eng.encode_control(img)
    kw = dict(emb_masks=mask, cfg_scale=a.cfg_scale, first_valid=fv)
    forms = {"score": lambda: eng.score(emb, tokens, **kw),
             "token_loop": lambda: eng.generate(emb, N, forced_tokens=tokens, return_logits=True, **kw)}
    if a.score_only:
        del forms["token_loop"]
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
    eng.check_errors(); eng.close()
    if a.score_only:
        print(f"score {statistics.median(ms['score']):.3f} ms", flush=True)
        return
    mult = 2 if a.cfg_scale > 1 else 1
    t0 = (fv // 32) * 32
    fl = pass_flops(g, a.B, N, mult, g.cls_token_num - t0)
    peak = a.peak_tflops or (2500.0 if a.precision == "bf16" else 157.0)
    med = {k: statistics.median(v) for k, v in ms.items()}
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "score_time.jsonl"), "a") as f:
        for k, v in ms.items():
            rec = dict(form=k, model=a.model, precision=a.precision, B=a.B, N=N, cfg_scale=a.cfg_scale, window_rows=g.cls_token_num - t0,
                       ms=round(med[k], 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3), repeats=a.repeats)
            if k == "score":
                rec.update(pass_tflop=round(fl / 1e12, 3), tflops=round(fl / med[k] / 1e9, 1), peak_tflops=peak, mfma_fraction=round(fl / med[k] / 1e9 / peak, 4),
                           ratio_token_loop_over_score=round(med["token_loop"] / med["score"], 2))
            line = json.dumps(rec)
            f.write(line + "\n")
            print("SCORE_TIME " + line, flush=True)


if __name__ == "__main__":
    main()
