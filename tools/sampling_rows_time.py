"""GPU timing of row mode (car_generate_rows: one car_sampling_row per image) next to the plain call, at the shapes of bench.py: the headline (LlamaGen-XL
t2i, 512 x 512 = 1024 tokens, bf16, 768 images, stochastic top_k = 2000, no CFG) and config 2 (one image, cfg 4).  Reported, not gated.  Not a test.

Three forms: `parent_uniform` — the plain call on ANOTHER build of the library (--parent-lib: the .so of the parent commit), `uniform` — the plain call on
this tree, `rows` — the row call with one distinct row per image (own seed, temperature, top_k; rng_stream 0).  The two builds cannot hold their KV caches
side by side at 768 images, so the parent build runs first in the same process (1 warm-up + --repeats calls) and is closed; `uniform` and `rows` are then
warmed and ALTERNATE, --repeats rounds.  Every call is timed on its own with device events on the caller's stream; median, min and max per form.
With --strength (a CFG configuration) a fourth form `rows_strength` gives every row control_strength 0.5, so that the pre-scale kernel runs: its cost is the
difference of the two row forms' prefill_ms (car_stats: control MLPs + pre-scale + prefill) — three small launches, expect it inside the noise.
Appends one line per form to <out-dir>/sampling_rows_time.jsonl.
usage: sampling_rows_time.py --config headline|2 [--parent-lib PATH] [--repeats 3] [--tokens 1024] [--strength] [--out-dir profiles]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("headline", "2"), default="2")
    ap.add_argument("--parent-lib", default=None, help="libcontrolar_hip.so of the parent commit (plain calls only)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=0, help="override the configuration's batch")
    ap.add_argument("--strength", action="store_true")
    ap.add_argument("--rows-only", action="store_true", help="two row calls and nothing else (kernel traces); nothing is written")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    from controlar_amd import _lib as L, config as Cfg, synth
    from controlar_amd.engine import Engine, first_valid_position
    cfg = Cfg.xl_t2i(1024, "small", "canny")
    g = cfg.gpt
    B = a.batch or (768 if a.config == "headline" else 1)
    cfg_scale = 1.0 if a.config == "headline" else 4.0
    stochastic = a.config == "headline"
    gsd, _ = synth.path_state_dicts(cfg, seed=0)
    nu = min(B, 16)                                                   # distinct inputs, repeated: the timing does not depend on their content
    rep = (B + nu - 1) // nu
    img = synth.canny_like_control(nu, 512, 512).repeat(rep, 1, 1, 1)[:B].cuda()
    emb, mask = synth.text_embeddings(nu, g.cls_token_num, g.caption_dim)
    emb, mask = emb.repeat(rep, 1, 1)[:B], mask.repeat(rep, 1)[:B]
    fv = first_valid_position(mask)
    emb, mask = emb.to(torch.bfloat16).cuda(), mask.cuda()
    uni = dict(emb_masks=mask, cfg_scale=cfg_scale, first_valid=fv, sample_logits=stochastic, top_k=2000 if stochastic else 0, seed=1)
    row = dict(uni, seed=list(range(100, 100 + B)), temperature=[0.8 + 0.4 * i / max(B - 1, 1) for i in range(B)] if stochastic else 1.0,
               top_k=[1500 + (i * 37) % 1000 for i in range(B)] if stochastic else 0, rng_stream=0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        print(f"call {e0.elapsed_time(e1):.1f} ms", flush=True)
        return e0.elapsed_time(e1)

    def engine(lib):
        L._lib = lib                                                  # Engine takes the library _lib.load() returns: the cached one
        eng = Engine(cfg, "bf16"); eng.load_state_dict(gsd); eng.finalize()
        eng.encode_control(img)
        return eng
    ms, prefill = {}, {}
    if a.parent_lib and not a.rows_only:
        lib = C.CDLL(a.parent_lib)
        for name, (res, args) in L.SYMBOLS.items():
            if hasattr(lib, name):
                fn = getattr(lib, name); fn.restype, fn.argtypes = res, args
        eng = engine(lib)
        call = lambda: eng.generate(emb, a.tokens, **uni)
        call()
        ms["parent_uniform"] = [timed(call) for _ in range(a.repeats)]
        eng.check_errors(); eng.close(); del eng
        torch.cuda.synchronize()
    eng = engine(None)
    forms = {"uniform": lambda: eng.generate(emb, a.tokens, **uni), "rows": lambda: eng.generate(emb, a.tokens, **row)}
    if a.strength:
        forms["rows_strength"] = lambda: eng.generate(emb, a.tokens, **dict(row, control_strength=[0.5] * B))
    if a.rows_only:
        fn = forms["rows_strength" if a.strength else "rows"]
        fn(); fn(); torch.cuda.synchronize(); eng.close()
        return
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    for k in forms:
        ms[k], prefill[k] = [], []
    for _ in range(a.repeats):
        for k, fn in forms.items():
            ms[k].append(timed(fn)); prefill[k].append(eng.stats()["prefill_ms"])
    graph = eng.stats()["graph_used"]
    eng.check_errors(); eng.close()
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "sampling_rows_time.jsonl"), "a") as f:
        for k, v in ms.items():
            rec = dict(form=k, config=a.config, model="xl", precision="bf16", B=B, tokens=a.tokens, cfg_scale=cfg_scale, stochastic=stochastic,
                       ms=round(statistics.median(v), 2), ms_min=round(min(v), 2), ms_max=round(max(v), 2), repeats=a.repeats, graph_used=bool(graph))
            if k in prefill:
                rec["prefill_ms"] = round(statistics.median(prefill[k]), 3)
            line = json.dumps(rec)
            f.write(line + "\n")
            print("ROWS_TIME " + line, flush=True)


if __name__ == "__main__":
    main()
