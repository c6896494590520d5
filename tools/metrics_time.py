"""GPU timing of Engine.ms_ssim (car_ms_ssim) at the evaluation scripts' batch, B = 16 of 1 x 512 x 512, fp32 pred against a uint8 target, next to the
fp32 torch restatement of the same definition (tests/metrics_ref.py: reflect pad, grouped 11 x 11 conv2d of five maps, crop, avg_pool2d) on the same
device — the only baseline there is.  Reported, not gated.  Not a test.

One process: both forms are warmed (3 calls each), then they alternate, `--repeats` rounds, each call timed on its own with device events on the
caller's stream; median, min and max per form.  The kernel's launch count is by construction (one launch per scale and one fold).  Bytes are the
algorithm's: both images read once per scale, the pooled images written once.  Writes <out-dir>/metrics_time.jsonl.
usage: metrics_time.py [--B 16] [--C 1] [--size 512] [--repeats 15] [--out-dir profiles]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAUNCHES = 5 + 1


def algo_bytes(B, C, H, W):
    n, total = B * C, 0
    for s in range(5):
        h, w = H >> s, W >> s
        total += n * h * w * ((1 + 4) if s == 0 else 8)          # scale 1 reads uint8 + fp32, the others two fp32 images
        if s < 4:
            total += n * (h // 2) * (w // 2) * 8                 # the pooled pair
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--C", type=int, default=1)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    from controlar_amd import config as Cfg
    from controlar_amd.engine import Engine
    from tests import metrics_ref as R
    t, p = R.soft_edge_maps(a.B, a.C, a.size, a.size, seed=104)
    p, t = (p * 255).cuda(), (t * 255).round().to(torch.uint8).cuda()
    sc = (1.0 / 255.0, 1.0 / 255.0)
    eng = Engine(Cfg.tiny_t2i(), "bf16")
    forms = {"car_ms_ssim": lambda: eng.ms_ssim(p, t, scale=sc), "torch_fp32": lambda: R.ms_ssim(p, t, sc, dtype=torch.float32)[0]}
    with torch.no_grad():
        for fn in forms.values():
            for _ in range(3):
                out = fn()
        torch.cuda.synchronize()
        dev = float((forms["car_ms_ssim"]().cpu() - forms["torch_fp32"]().double().cpu()).abs().max())
        ms = {k: [] for k in forms}
        for _ in range(a.repeats):
            for k, fn in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record(); e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
    eng.close()
    by = algo_bytes(a.B, a.C, a.size, a.size)
    lines = []
    for k, v in ms.items():
        med = statistics.median(v)
        rec = dict(form=k, B=a.B, C=a.C, H=a.size, W=a.size, ms=round(med, 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), repeats=a.repeats,
                   algo_mb=round(by / 1e6, 1), algo_gb_per_s=round(by / med / 1e6, 1), max_abs_diff_between_forms=dev)
        if k == "car_ms_ssim":
            rec["launches"] = LAUNCHES
        lines.append(json.dumps(rec))
        print("METRICS_TIME " + lines[-1], flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "metrics_time.jsonl"), "w") as f:
        f.write("\n".join(lines) + "\n")
    m = {k: statistics.median(v) for k, v in ms.items()}
    print(f"car_ms_ssim {m['car_ms_ssim']:.3f} ms, torch fp32 {m['torch_fp32']:.3f} ms, ratio torch / car_ms_ssim {m['torch_fp32'] / m['car_ms_ssim']:.2f}", flush=True)


if __name__ == "__main__":
    main()
