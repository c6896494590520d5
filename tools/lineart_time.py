"""GPU timing of the LineArt extractor (car_lineart) at 512 x 512, B = 8, in both arithmetic modes, next to the VQ decoder's rate from the same
session.  Reported, not gated: there is no parent or reference number.  Not a test.

The measurement runs in a child process under a time limit of its own.  Per mode: 3 warm-up calls, then `--repeats` calls timed one by one with
device events on the caller's stream; the figure is the median.  FLOPs are the algorithm's, computed from the shapes below (transposed convolutions
counted as their four parity phases, 9 taps per INPUT pixel).
usage: lineart_time.py [--B 8] [--size 512] [--repeats 9] [--timeout 300]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lineart_flops(H: int, W: int) -> float:
    h1, w1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    h2, w2 = (h1 - 1) // 2 + 1, (w1 - 1) // 2 + 1
    mac = H * W * 64 * 147 + h1 * w1 * 128 * 576 + h2 * w2 * 256 * 1152 + 6 * h2 * w2 * 256 * 2304
    mac += h2 * w2 * 9 * 256 * 128 + (2 * h2) * (2 * w2) * 9 * 128 * 64 + (4 * h2) * (4 * w2) * 3136
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


def child(a):
    import torch
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    B, S = a.B, a.size
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 256, (B, 3, S, S), generator=g).float().cuda()
    sd = synth.lineart_state_dict(11)
    fl = lineart_flops(S, S)
    for prec in ("bf16", "fp32"):
        eng = Engine(C.tiny_t2i(), prec)
        eng.load_lineart(sd)
        med, lo, hi = _timed(lambda: eng.lineart(x, want_control=True), a.repeats if prec == "bf16" else max(3, a.repeats // 3))
        print(json.dumps(dict(stage="lineart", mode=prec, B=B, H=S, W=S, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                              ms_per_image=round(med / B, 3), gflop_per_image=round(fl / 1e9, 1), tflops=round(fl * B / med / 1e9, 1))), flush=True)
        eng.close()
    # the project's own 3x3 conv path in the same session: the VQ-16 decoder (32 x 32 tokens -> 512 x 512, 1.017 TFLOP per image, almost all of it 3x3 convs)
    cfg = C.xl_t2i(1024)
    _, vsd = synth.path_state_dicts(cfg, 0)
    vq = Engine(cfg, "bf16"); vq.load_state_dict(vsd, finalize=True)
    toks = torch.randint(0, 16384, (B, 1024), dtype=torch.int32).cuda()
    med, lo, hi = _timed(lambda: vq.vq_decode(toks, 32, 32), a.repeats)
    print(json.dumps(dict(stage="vq_decode", mode="bf16", B=B, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3), ms_per_image=round(med / B, 3),
                          tflops=round(1.017 * B / med * 1e3, 1))), flush=True)
    vq.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a)
    else:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--B", str(a.B), "--size", str(a.size), "--repeats", str(a.repeats)],
                           timeout=a.timeout)
        sys.exit(r.returncode)
