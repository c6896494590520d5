"""GPU timing of the evaluator's statistics (car_manifold_radii, car_manifold_pr, car_fid_accumulate + car_fid_finalize, car_inception_score) at the
size of evaluations/c2i/evaluator.py, N = 50 000 activations of D = 2048 (and N = 10 000, D = 2023 for the sFID moments), next to a plain torch
restatement on the same GPU: cdist-style 10 000 x 10 000 blocks in fp16 plus kthvalue / comparisons, torch.cov in fp64, softmax and the KL in fp64.
Reported, not gated.  Not a test.

Every stage runs in a child process of its own under its own time limit.  Per stage: both forms warmed once, then `--repeats` rounds that time one
call of each, alternating, with device events; median, min and max.  `parity` runs tests/test_fid_gpu.py and keeps the figures it prints.  The parent
stops at the first child that fails and writes <out-dir>/fid_time.jsonl and <out-dir>/fid_parity_measured.jsonl.
usage: fid_time.py [--N 50000] [--D 2048] [--repeats 5] [--timeout 280] [--out-dir profiles] [--stages parity,radii,pr,moments,smoments,is]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP16_DENSE_PEAK_TFLOPS = 2500.0          # MI355X, dense fp16 on the matrix cores


def _alternate(fns, repeats):
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def _torch_dist(u, v):
    """_batch_pairwise_distances on fp16 casts, as DistanceBlock builds it (no fallback: the timed inputs stay finite)"""
    a, b = u.half(), v.half()
    return ((a * a).sum(1)[:, None] - 2 * (a @ b.T) + (b * b).sum(1)[None, :]).clamp_min(0)


def _torch_radii(f, k, blk):
    import torch
    out = torch.empty(len(f), device=f.device)
    for r0 in range(0, len(f), blk):
        row = torch.cat([_torch_dist(f[r0:r0 + blk], f[c0:c0 + blk]) for c0 in range(0, len(f), blk)], dim=1)
        out[r0:r0 + blk] = row.float().kthvalue(k + 1, dim=1).values
    return out


def _torch_pr(f1, r1, f2, r2, blk):
    import torch
    s1, s2 = torch.zeros(len(f1), dtype=torch.bool, device=f1.device), torch.zeros(len(f2), dtype=torch.bool, device=f1.device)
    for a0 in range(0, len(f1), blk):
        for b0 in range(0, len(f2), blk):
            d = _torch_dist(f1[a0:a0 + blk], f2[b0:b0 + blk]).float()
            s1[a0:a0 + blk] |= (d <= r2[None, b0:b0 + blk]).any(1)
            s2[b0:b0 + blk] |= (d <= r1[a0:a0 + blk, None]).any(0)
    return s2.double().mean(), s1.double().mean()


def _torch_is(acts, w, split):
    import torch
    p = torch.softmax(acts @ w, dim=1).double()
    vals = []
    for i in range(0, len(p), split):
        part = p[i:i + split]
        vals.append(torch.exp((part * (part.log() - part.mean(0, keepdim=True).log())).sum(1).mean()))
    return torch.stack(vals).mean()


def child(a):
    import torch
    from controlar_amd import config as C
    from controlar_amd.engine import Engine
    if a.child == "parity":
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_fid_gpu.py"), "-q", "-s", "-p", "no:cacheprovider"],
                           stdout=subprocess.PIPE, text=True, cwd=ROOT)
        for ln in r.stdout.splitlines():
            i = ln.find("FID_PARITY ")
            if i >= 0:
                print(ln[i:], flush=True)
        sys.exit(r.returncode)
    eng = Engine(C.tiny_t2i(), "bf16")
    g = torch.Generator(device="cuda").manual_seed(11)
    N, D, blk = a.N, a.D, 10000
    rec = dict(stage=a.child, N=N, D=D)
    if a.child in ("radii", "pr"):
        f1 = torch.randn(N, D, device="cuda", generator=g).clamp_min(0) * 0.4
        f2 = torch.randn(N, D, device="cuda", generator=g).clamp_min(0) * 0.4
        if a.child == "radii":
            t = _alternate({"hip": lambda: eng.manifold_radii(f1, 3, blk, blk), "torch": lambda: _torch_radii(f1, 3, blk)}, a.repeats)
            flop = 2.0 * N * N * D
            same = float((eng.manifold_radii(f1, 3, blk, blk) == _torch_radii(f1, 3, blk)).double().mean())
            rec.update(fraction_of_radii_equal_to_torch=same)
        else:
            r1, r2 = eng.manifold_radii(f1, 3, blk, blk), eng.manifold_radii(f2, 3, blk, blk)
            t = _alternate({"hip": lambda: eng.manifold_pr(f1, r1, f2, r2, blk, blk), "torch": lambda: _torch_pr(f1, r1, f2, r2, blk)}, a.repeats)
            flop = 2.0 * N * N * D
            pr, tp = eng.manifold_pr(f1, r1, f2, r2, blk, blk)[2].cpu(), _torch_pr(f1, r1, f2, r2, blk)
            rec.update(precision=float(pr[0]), recall=float(pr[1]), torch_precision=float(tp[0]), torch_recall=float(tp[1]))
        rec.update(tflops=round(flop / t["hip"][0] / 1e9, 1), fraction_of_fp16_peak=round(flop / t["hip"][0] / 1e9 / FP16_DENSE_PEAK_TFLOPS, 3),
                   torch_tflops=round(flop / t["torch"][0] / 1e9, 1))
    elif a.child in ("moments", "smoments"):
        if a.child == "smoments":
            N, D = 10000, 2023
            rec.update(N=N, D=D)
        x = torch.randn(N, D, device="cuda", generator=g).clamp_min(0) * 0.4 + 1.0
        st = eng.fid_state(D)

        def hip():
            st.zero_()
            for i in range(0, N, 10000):
                eng.fid_accumulate(st, x[i:i + 10000])
            return eng.fid_finalize(st, D)
        t = _alternate({"hip": hip, "torch": lambda: (x.double().mean(0), torch.cov(x.double().T))}, a.repeats)
        flop = 2.0 * N * D * D
        rec.update(tflops_fp64=round(flop / t["hip"][0] / 1e9, 1), torch_tflops_fp64=round(flop / t["torch"][0] / 1e9, 1),
                   max_abs_sigma_diff=float((hip()[1] - torch.cov(x.double().T)).abs().max()))
    else:
        Cn = 1008
        acts = torch.randn(N, D, device="cuda", generator=g).clamp_min(0) * 0.4
        w = torch.randn(D, Cn, device="cuda", generator=g) * 0.05
        t = _alternate({"hip": lambda: eng.inception_score(acts, w, 5000), "torch": lambda: _torch_is(acts, w, 5000)}, a.repeats)
        rec.update(C=Cn, score=float(eng.inception_score(acts, w, 5000)[0]), torch_score=float(_torch_is(acts, w, 5000)))
    for k, (med, lo, hi) in t.items():
        pre = "" if k == "hip" else "torch_"
        rec.update({pre + "ms": round(med, 3), pre + "ms_min": round(lo, 3), pre + "ms_max": round(hi, 3)})
    eng.close()
    print("FID_TIME " + json.dumps(rec), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=50000)
    ap.add_argument("--D", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=280)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--stages", default="parity,radii,pr,moments,smoments,is")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a)
        sys.exit(0)
    lines = {"FID_TIME": [], "FID_PARITY": []}
    rc = 0
    for stage in a.stages.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", stage, "--N", str(a.N), "--D", str(a.D), "--repeats", str(a.repeats)]
        try:
            r = subprocess.run(cmd, timeout=a.timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print(f"{stage}: no result within {a.timeout} s; stopping", flush=True)
            rc = 124
            break
        sys.stdout.write(r.stdout); sys.stdout.flush()
        for ln in r.stdout.splitlines():
            for tag in lines:
                if ln.startswith(tag + " "):
                    lines[tag].append(ln[len(tag) + 1:])
        if r.returncode != 0:                        # a failed child may have faulted the device: nothing more runs on it
            print(f"{stage}: exit status {r.returncode}; stopping", flush=True)
            rc = r.returncode if r.returncode > 0 else 1
            break
    os.makedirs(a.out_dir, exist_ok=True)
    for tag, fn in (("FID_TIME", "fid_time.jsonl"), ("FID_PARITY", "fid_parity_measured.jsonl")):
        if lines[tag]:
            with open(os.path.join(a.out_dir, fn), "w") as f:
                f.write("\n".join(lines[tag]) + "\n")
    sys.exit(rc)
