"""GPU timing of the HED extractor (car_hed) at 512 x 512, B = 8, in both arithmetic modes, next to the same network written with torch.nn.functional
on the same device in the same dtype (MIOpen convolutions) — the only baseline there is.  Reported, not gated.  Not a test.

Every measurement runs in a child process of its own under its own time limit: `hed` / `torch` x `bf16` / `fp32`, and `parity` (every fixture of
tests/golden/hed_*.npz in both modes, the figures tests/test_hed_gpu.py asserts on).  Per timing: 3 warm-up calls, then `--repeats` calls timed one by
one with device events on the caller's stream; median, min and max.  FLOPs are the algorithm's (hed_flops).  The parent stops at the first child that
fails, and writes what it has to <out-dir>/hed_time.jsonl and <out-dir>/hed_parity_measured.jsonl.
usage: hed_time.py [--B 8] [--size 512] [--repeats 9] [--timeout 240] [--out-dir profiles]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCKS = ((3, 64, 2), (64, 128, 2), (128, 256, 3), (256, 512, 3), (512, 512, 3))


def hed_flops(H: int, W: int) -> float:
    mac = 0
    for l, (ci, co, n) in enumerate(BLOCKS):
        p = (H >> l) * (W >> l)
        mac += p * 9 * (ci * co + (n - 1) * co * co) + p * co
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


def _torch_hed(sd, dtype):
    """condition/hed.py:17-81 restated with torch.nn.functional, weights and activations in `dtype`; the fusion tail in fp32 as car_hed has it"""
    import torch
    import torch.nn.functional as F
    w = {k: v.cuda().to(dtype if k != "norm" else torch.float32) for k, v in sd.items()}

    def run(x):
        B, _, H, W = x.shape
        h = (x - w["norm"]).to(dtype)
        sides = []
        for b, (_, _, n) in enumerate(BLOCKS, 1):
            if b > 1:
                h = F.max_pool2d(h, 2, 2)
            for i in range(n):
                h = F.relu(F.conv2d(h, w[f"block{b}.convs.{i}.weight"], w[f"block{b}.convs.{i}.bias"], padding=1))
            s = F.conv2d(h, w[f"block{b}.projection.weight"], w[f"block{b}.projection.bias"]).float()
            sides.append(F.interpolate(s, size=(H, W), mode="bilinear", align_corners=False).squeeze(1))
        edge = (torch.sigmoid(torch.stack(sides, 1).mean(1)) * 255.0).clamp(0, 255)
        return edge, (2 * (edge / 255 - 0.5)).to(dtype).unsqueeze(1).expand(B, 3, H, W).contiguous()
    return run


def child(a):
    import numpy as np
    import torch
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    sd = synth.hed_state_dict(11)
    if a.child == "parity":
        for prec in ("fp32", "bf16"):
            eng = Engine(C.tiny_t2i(), prec)
            eng.load_hed(sd)
            for name in ("b2_16x24", "b1_17x31", "b1_35x50", "b1_72x104"):
                z = np.load(os.path.join(ROOT, "tests", "golden", f"hed_{name}.npz"))
                d = np.abs(eng.hed(torch.from_numpy(z["x"])).cpu().numpy().astype(np.float64) - z["ref"])
                print("HED_PARITY " + json.dumps(dict(case=name, mode=prec, max_abs=float(d.max()), mean_abs=float(d.mean()),
                                                      ref_f32_vs_f64_max=float(z["ref_f32_vs_f64_max"]), bf16_emul_max=float(z["bf16_emul_max"]),
                                                      bf16_emul_mean=float(z["bf16_emul_mean"]))), flush=True)
            eng.close()
        return
    B, S, prec = a.B, a.size, a.mode
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 256, (B, 3, S, S), generator=g).float().cuda()
    fl = hed_flops(S, S)
    reps = a.repeats if prec == "bf16" else max(3, a.repeats // 3)
    if a.child == "hed":
        eng = Engine(C.tiny_t2i(), prec)
        eng.load_hed(sd)
        med, lo, hi = _timed(lambda: eng.hed(x, want_control=True), reps)
        eng.close()
    else:
        run = _torch_hed(sd, torch.bfloat16 if prec == "bf16" else torch.float32)
        with torch.no_grad():
            med, lo, hi = _timed(lambda: run(x), reps)
    print("HED_TIME " + json.dumps(dict(stage=a.child, mode=prec, B=B, H=S, W=S, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                                        ms_per_image=round(med / B, 3), gflop_per_image=round(fl / 1e9, 1), tflops=round(fl * B / med / 1e9, 1))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--child", default=None, choices=["hed", "torch", "parity"])
    ap.add_argument("--mode", default="bf16", choices=["bf16", "fp32"])
    a = ap.parse_args()
    if a.child:
        child(a)
        sys.exit(0)
    lines = {"HED_TIME": [], "HED_PARITY": []}
    rc = 0
    for stage, mode in (("parity", "bf16"), ("hed", "bf16"), ("hed", "fp32"), ("torch", "bf16"), ("torch", "fp32")):
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
    for tag, fn in (("HED_TIME", "hed_time.jsonl"), ("HED_PARITY", "hed_parity_measured.jsonl")):
        if lines[tag]:
            with open(os.path.join(a.out_dir, fn), "w") as f:
                f.write("\n".join(lines[tag]) + "\n")
    t = {(json.loads(l)["stage"], json.loads(l)["mode"]): json.loads(l)["ms"] for l in lines["HED_TIME"]}
    for mode in ("bf16", "fp32"):
        if ("hed", mode) in t and ("torch", mode) in t:
            print(f"{mode}: car_hed {t['hed', mode]} ms, torch.nn.functional {t['torch', mode]} ms, ratio torch / car_hed {t['torch', mode] / t['hed', mode]:.2f}", flush=True)
    sys.exit(rc)
