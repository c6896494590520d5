"""GPU timing of the LPIPS distance (car_lpips) at 8 pairs of 512 x 512, in both arithmetic modes, next to the same network written with
torch.nn.functional on the same device in the same dtype (MIOpen convolutions; head in fp32, as car_lpips has it).  Reported, not gated.  Not a test.

Every measurement runs in a child process of its own under its own time limit: `lpips` / `torch` x `bf16` / `fp32`, and `parity` (every fixture of
tests/golden/lpips_*.npz in both modes, the figures tests/test_lpips_gpu.py asserts on).  Per timing: 3 warm-up calls, then `--repeats` calls timed one
by one with device events on the caller's stream; median, min and max.  FLOPs are the trunk's (two images per pair).  The parent stops at the first
child that fails, and writes what it has to <out-dir>/lpips_time.jsonl and <out-dir>/lpips_parity_measured.jsonl.
usage: lpips_time.py [--B 8] [--size 512] [--repeats 9] [--timeout 240] [--out-dir profiles]"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCKS = ((3, 64, 2), (64, 128, 2), (128, 256, 3), (256, 512, 3), (512, 512, 3))
FEATURES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
WEIGHT_SEED = 17


def trunk_flops(H: int, W: int) -> float:
    mac = 0
    for l, (ci, co, n) in enumerate(BLOCKS):
        mac += (H >> l) * (W >> l) * 9 * (ci * co + (n - 1) * co * co)
    return 2.0 * mac


def _timed(fn, repeats):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def _torch_lpips(sd, dtype):
    """tokenizer/tokenizer_image/lpips.py:83-164 restated with torch.nn.functional: trunk weights and activations in `dtype`, both images of a pair in one
    batch, the head in fp32 and the spatial mean in fp64, as car_lpips has them"""
    import torch
    import torch.nn.functional as F
    w = {k: v.cuda().to(dtype if k.startswith("net.") else torch.float32) for k, v in sd.items()}

    def run(a, b):
        B = a.shape[0]
        h = ((torch.cat([a, b]) - w["scaling_layer.shift"]) / w["scaling_layer.scale"]).to(dtype)
        val = None
        for s, idx in enumerate(FEATURES, 1):
            if s > 1:
                h = F.max_pool2d(h, 2, 2)
            for n in idx:
                h = F.relu(F.conv2d(h, w[f"net.slice{s}.{n}.weight"], w[f"net.slice{s}.{n}.bias"], padding=1))
            t = h.float()
            f = t / (t.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
            d = F.conv2d((f[:B] - f[B:]) ** 2, w[f"lin{s - 1}.model.1.weight"]).double().mean(dim=(1, 2, 3))
            val = d if val is None else val + d
        return val
    return run


def child(a):
    import numpy as np
    import torch
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    sd = synth.lpips_state_dict(WEIGHT_SEED)
    if a.child == "parity":
        spec = importlib.util.spec_from_file_location("make_lpips_golden", os.path.join(ROOT, "tests", "golden", "make_lpips_golden.py"))
        mk = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mk)
        measured = json.load(open(os.path.join(ROOT, "tests", "golden", "lpips_measured.json")))
        for prec in ("fp32", "bf16"):
            eng = Engine(C.tiny_t2i(), prec)
            eng.load_lpips(sd)
            for name in mk.CASES:
                z, m = np.load(os.path.join(ROOT, "tests", "golden", f"lpips_{name}.npz")), measured[name]
                x, y = mk.case_inputs(name)
                val, lay = (t.cpu().numpy() for t in eng.lpips(x, y, want_layers=True))
                rv, rl = (z["val64"], z["layers64"]) if prec == "fp32" else (z["val32"].astype(np.float64), z["layers32"].astype(np.float64))
                bv, bl = (16 * m["f32_vs_f64_val"], 16 * m["f32_vs_f64_layers"]) if prec == "fp32" else (2 * m["bf16_vs_f32_val"], 2 * m["bf16_vs_f32_layers"])
                print("LPIPS_PARITY " + json.dumps(dict(case=name, mode=prec, val=val.tolist(), max_abs_val=float(np.abs(val - rv).max()), bound_val=bv,
                                                        max_abs_layers=float(np.abs(lay - rl).max()), bound_layers=bl)), flush=True)
            eng.close()
        return
    B, S, prec = a.B, a.size, a.mode
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()
    y = (x + 0.05 * torch.randn(B, 3, S, S, generator=g).cuda()).clamp(-1, 1)
    fl = 2 * trunk_flops(S, S)
    reps = a.repeats if prec == "bf16" else max(3, a.repeats // 3)
    if a.child == "lpips":
        eng = Engine(C.tiny_t2i(), prec)
        eng.load_lpips(sd)
        med, lo, hi = _timed(lambda: eng.lpips(x, y, want_layers=True), reps)
        val = eng.lpips(x, y)
        eng.close()
    else:
        run = _torch_lpips(sd, torch.bfloat16 if prec == "bf16" else torch.float32)
        with torch.no_grad():
            med, lo, hi = _timed(lambda: run(x, y), reps)
            val = run(x, y)
    print("LPIPS_TIME " + json.dumps(dict(stage=a.child, mode=prec, pairs=B, H=S, W=S, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                                          ms_per_pair=round(med / B, 3), gflop_per_pair=round(fl / 1e9, 1), tflops=round(fl * B / med / 1e9, 1),
                                          mean_lpips=float(val.mean()))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--child", default=None, choices=["lpips", "torch", "parity"])
    ap.add_argument("--mode", default="bf16", choices=["bf16", "fp32"])
    a = ap.parse_args()
    if a.child:
        child(a)
        sys.exit(0)
    lines = {"LPIPS_TIME": [], "LPIPS_PARITY": []}
    rc = 0
    for stage, mode in (("parity", "bf16"), ("lpips", "bf16"), ("lpips", "fp32"), ("torch", "bf16"), ("torch", "fp32")):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", stage, "--mode", mode, "--B", str(a.B), "--size", str(a.size), "--repeats", str(a.repeats)]
        try:
            r = subprocess.run(cmd, timeout=a.timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print(f"{stage} {mode}: no result within {a.timeout} s; stopping", flush=True)
            rc = 124
            break
        sys.stdout.write(r.stdout); sys.stdout.flush()
        for ln in r.stdout.splitlines():
            for tag in lines:
                if ln.startswith(tag + " "):
                    lines[tag].append(ln[len(tag) + 1:])
        if r.returncode != 0:                        # a failed child may have faulted the device: nothing more runs on it
            print(f"{stage} {mode}: exit status {r.returncode}; stopping", flush=True)
            rc = r.returncode if r.returncode > 0 else 1
            break
    os.makedirs(a.out_dir, exist_ok=True)
    for tag, fn in (("LPIPS_TIME", "lpips_time.jsonl"), ("LPIPS_PARITY", "lpips_parity_measured.jsonl")):
        if lines[tag]:
            with open(os.path.join(a.out_dir, fn), "w") as f:
                f.write("\n".join(lines[tag]) + "\n")
    t = {(json.loads(l)["stage"], json.loads(l)["mode"]): json.loads(l)["ms"] for l in lines["LPIPS_TIME"]}
    for mode in ("bf16", "fp32"):
        if ("lpips", mode) in t and ("torch", mode) in t:
            print(f"{mode}: car_lpips {t['lpips', mode]} ms, torch.nn.functional {t['torch', mode]} ms, ratio torch / car_lpips {t['torch', mode] / t['lpips', mode]:.2f}", flush=True)
    sys.exit(rc)
