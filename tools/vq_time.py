"""GPU timing of the VQ decoder (Engine.vq_decode) at 32 x 32 tokens (512 x 512 pixels), B = 16, for the three arithmetics: `bf16`, `fp32` (exact) and
`fp32+vq_split` (car_config.vq_split_bf16: fp32 operands as two bf16 numbers, three bf16 MFMAs per product), with the deviation of each from the
reference's pixels (tests/golden/vq16_real_32x32.npz).  Reported, not gated.  Not a test.

Every measurement runs in a child process of its own under its own time limit; the parent stops at the first child that fails.  Per timing: 3 warm-up
calls, then `--repeats` calls timed one by one with device events on the caller's stream; median, min and max.  At most 16 CPU threads; no device or
host setting is touched.  `--modes bf16,fp32` runs on a commit that has no vq_split; `--label` names the commit in the output.  Lines are appended to
<out-dir>/vq_time.jsonl, each with the library's build id, so the lines of two commits sit side by side.
usage: vq_time.py [--modes bf16,fp32,fp32+vq_split] [--label this] [--B 16] [--repeats 9] [--timeout 300] [--out-dir profiles]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = ("bf16", "fp32", "fp32+vq_split")


def child(a):
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    prec, _, opt = a.child.partition("+")
    cfg = C.tiny_t2i(64, "canny"); cfg.vq = C.VQConfig()
    eng = Engine(cfg, prec, **({"vq_split": True} if opt == "vq_split" else {}))
    eng.load_state_dict(synth.vq_state_dict(cfg.vq, seed=2), finalize=True)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "vq16_real_32x32.npz"))
    g = torch.Generator().manual_seed(21)
    toks = torch.randint(0, cfg.vq.codebook_size, (a.B, 1024), generator=g, dtype=torch.int32)
    toks[0] = torch.from_numpy(gold["tokens"][0]); toks[a.B - 1] = torch.from_numpy(gold["tokens"][1])
    toks = toks.cuda()
    px = eng.vq_decode(toks, 32, 32)
    dmax, dsum, dn = 0.0, 0.0, 0
    for row, gi in ((0, 0), (a.B - 1, 1)):
        p = px[row].cpu().numpy()
        for name, got in (("lattice", p[:, ::8, ::8]), ("corner", p[:, :24, :24]), ("centre", p[:, 244:268, 244:268])):
            d = np.abs(got.astype(np.float64) - gold[name][gi])
            dmax = max(dmax, float(d.max())); dsum += float(d.sum()); dn += d.size
    for _ in range(2):
        eng.vq_decode(toks, 32, 32)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(); eng.vq_decode(toks, 32, 32); t1.record(); t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    med = statistics.median(ms)
    print("VQ_TIME " + json.dumps(dict(label=a.label, mode=a.child, build_id=eng.lib.car_build_id().decode(), B=a.B, tokens="32x32", repeats=a.repeats,
                                       ms=round(med, 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), ms_per_image=round(med / a.B, 3),
                                       max_abs_diff=dmax, mean_abs_diff=dsum / dn)), flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--label", default="this")
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--child", default=None, choices=MODES)
    a = ap.parse_args()
    if a.child:
        child(a)
        sys.exit(0)
    modes = [m for m in a.modes.split(",") if m]
    for m in modes:
        if m not in MODES:
            ap.error(f"unknown mode {m!r} (choose from {', '.join(MODES)})")
    lines, rc = [], 0
    for m in modes:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", m, "--label", a.label, "--B", str(a.B), "--repeats", str(a.repeats)]
        try:
            r = subprocess.run(cmd, timeout=a.timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print(f"{m}: no result within {a.timeout} s; stopping", flush=True)
            rc = 124
            break
        sys.stdout.write(r.stdout); sys.stdout.flush()
        lines += [ln[len("VQ_TIME "):] for ln in r.stdout.splitlines() if ln.startswith("VQ_TIME ")]
        if r.returncode != 0:                        # a failed child may have faulted the device: nothing more runs on it
            print(f"{m}: exit status {r.returncode}; stopping", flush=True)
            rc = r.returncode if r.returncode > 0 else 1
            break
    if lines:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "vq_time.jsonl"), "a") as f:
            f.write("\n".join(lines) + "\n")
    t = {json.loads(l)["mode"]: json.loads(l)["ms_per_image"] for l in lines}
    if "fp32" in t and "fp32+vq_split" in t:
        print(f"per image: fp32 {t['fp32']} ms, fp32+vq_split {t['fp32+vq_split']} ms, ratio {t['fp32'] / t['fp32+vq_split']:.2f}", flush=True)
    sys.exit(rc)
