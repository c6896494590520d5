"""GPU timing of the DPT depth estimator (car_depth) with dpt_large and synthetic weights, at 384 x 384 and 512 x 512, B = 1 and 8, in both arithmetic
modes, next to transformers' DPTForDepthEstimation on the same device in the same dtype where transformers imports.  Reported, not gated.  Not a test.

Every (stage, mode) runs in a child process of its own under its own time limit and walks the four (size, B) points:
  depth      car_depth of the shipped library, map and control tensor
  backbone   the development build with CAR_DEPTH_BACKBONE_ONLY=1: patchify, embeddings and the ViT layers up to the last tap, no readout, neck or head;
             neck + head = depth - backbone
  upfirst    the development build with CAR_DEPTH_UP_FIRST=1: the fusion layers up-sample first and project afterwards (the reference's order) — the A/B
             behind the choice to commute the two
  torch      DPTForDepthEstimation(pixel_values).predicted_depth through torch (HF eager modules, MIOpen / hipBLASLt)
Per point: 2 warm-up calls, then `--repeats` calls timed one by one with device events on the caller's stream; median, min and max.  FLOPs are the
algorithm's (depth_flops).  The parent stops at the first child that fails and writes what it has to <out-dir>/depth_time.jsonl.
usage: depth_time.py [--repeats 7] [--timeout 400] [--out-dir profiles] [--sizes 384 512] [--batches 1 8]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def depth_flops(cfg, S):
    """(backbone, neck + head) FLOPs of one image: 2 x multiply-adds of every GEMM and convolution car_depth runs (projection before up-sampling)."""
    D, I, F, g = cfg.hidden_size, cfg.intermediate_size, cfg.fusion_hidden_size, S // 16
    n, T = g * g, g * g + 1
    layers = cfg.backbone_out_indices[-1] + 1
    bb = n * 768 * D + layers * (T * (4 * D * D + 2 * D * I) + 2 * T * T * D)
    nk = 0
    side = (4 * g, 2 * g, g, g // 2)
    for i, c in enumerate(cfg.neck_hidden_sizes):
        nk += n * D * D + D * D + n * D * c                               # readout (tokens + cls), 1x1 projection
        if i < 2:
            nk += n * c * c * (16 if i == 0 else 4)                       # transposed conv as a GEMM
        elif i == 3:
            nk += side[3] ** 2 * 9 * c * c
        nk += side[i] ** 2 * 9 * c * F                                    # neck.convs[i]
    for j in range(4):
        s = side[3 - j]
        nk += s * s * 9 * F * F * (2 if j == 0 else 4) + s * s * F * F    # residual units, projection at the low resolution
    nk += (8 * g) ** 2 * 9 * F * (F // 2) + S * S * (9 * (F // 2) * 32 + 32)
    return 2.0 * bb, 2.0 * nk


def _timed(fn, repeats):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def child(a):
    import torch
    from controlar_amd import config as C, synth
    cfg = C.dpt_large()
    sd = synth.dpt_state_dict(cfg, 13)
    prec = a.mode
    dtype = torch.bfloat16 if prec == "bf16" else torch.float32
    run = None
    if a.child == "torch":
        spec_dir = os.path.join(ROOT, "tests", "golden")
        sys.path.insert(0, spec_dir)
        import make_depth_golden as mk
        if not mk.transformers_present():
            print("DEPTH_NOTE " + json.dumps(dict(stage="torch", note="transformers is absent: no baseline")), flush=True)
            return
        from transformers import DPTForDepthEstimation
        model = DPTForDepthEstimation(mk.hf_config(cfg)).eval()
        model.load_state_dict(sd, strict=True)
        model = model.to(dtype).cuda()
        run = lambda x: model(pixel_values=x.to(dtype)).predicted_depth
    else:
        from controlar_amd.engine import Engine
        eng = Engine(C.tiny_t2i(), prec, dev=a.child != "depth")
        eng.load_depth(sd, cfg)
        run = lambda x: eng.depth(x, want_control=True)
    del sd
    for S in a.sizes:
        fb, fn_ = depth_flops(cfg, S)
        for B in a.batches:
            g = torch.Generator().manual_seed(5)
            x = (torch.randint(0, 256, (B, 3, S, S), generator=g).float() / 255 - 0.5) / 0.5
            x = x.cuda()
            reps = a.repeats if prec == "bf16" else max(3, a.repeats // 2)
            with torch.no_grad():
                med, lo, hi = _timed(lambda: run(x), reps)
            fl = fb if a.child == "backbone" else fb + fn_
            print("DEPTH_TIME " + json.dumps(dict(stage=a.child, mode=prec, B=B, S=S, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                                                  ms_per_image=round(med / B, 3), gflop_per_image=round(fl / 1e9, 1), tflops=round(fl * B / med / 1e9, 1))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--sizes", type=int, nargs="+", default=[384, 512])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--child", default=None, choices=["depth", "backbone", "upfirst", "torch"])
    ap.add_argument("--mode", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--stages", nargs="+", default=["depth", "backbone", "upfirst", "torch"])
    a = ap.parse_args()
    if a.child:
        child(a)
        sys.exit(0)
    lines = []
    rc = 0
    for stage in a.stages:
        for mode in ("bf16", "fp32"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", stage, "--mode", mode, "--repeats", str(a.repeats),
                   "--sizes"] + [str(s) for s in a.sizes] + ["--batches"] + [str(b) for b in a.batches]
            env = dict(os.environ)
            env.pop("CAR_DEPTH_BACKBONE_ONLY", None); env.pop("CAR_DEPTH_UP_FIRST", None)
            if stage == "backbone":
                env["CAR_DEPTH_BACKBONE_ONLY"] = "1"
            if stage == "upfirst":
                env["CAR_DEPTH_UP_FIRST"] = "1"
            try:
                r = subprocess.run(cmd, timeout=a.timeout, stdout=subprocess.PIPE, text=True, env=env)
            except subprocess.TimeoutExpired:
                print(f"{stage} {mode}: no result within {a.timeout} s; stopping", flush=True)
                rc = 124
                break
            sys.stdout.write(r.stdout); sys.stdout.flush()
            lines += [ln[len("DEPTH_TIME "):] for ln in r.stdout.splitlines() if ln.startswith("DEPTH_TIME ")]
            if r.returncode != 0:                        # a failed child may have faulted the device: nothing more runs on it
                print(f"{stage} {mode}: exit status {r.returncode}; stopping", flush=True)
                rc = r.returncode if r.returncode > 0 else 1
                break
        if rc:
            break
    recs = [json.loads(l) for l in lines]
    t = {(r["stage"], r["mode"], r["S"], r["B"]): r["ms"] for r in recs}
    for (stage, mode, S, B), ms in sorted(t.items()):
        if stage == "depth" and ("backbone", mode, S, B) in t:
            bb = t["backbone", mode, S, B]
            recs.append(dict(stage="split", mode=mode, B=B, S=S, ms=ms, backbone_ms=bb, neck_head_ms=round(ms - bb, 3),
                             torch_ms=t.get(("torch", mode, S, B)), upfirst_ms=t.get(("upfirst", mode, S, B))))
            print("DEPTH_SPLIT " + json.dumps(recs[-1]), flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    if recs:
        with open(os.path.join(a.out_dir, "depth_time.jsonl"), "w") as f:
            f.write("\n".join(json.dumps(r) for r in recs) + "\n")
    sys.exit(rc)
