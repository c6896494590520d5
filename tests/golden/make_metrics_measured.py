"""Writes tests/golden/metrics_measured.json: how far the fp32 CPU restatements of tests/metrics_ref.py deviate from the fp64 ones over exactly the
inputs test_metrics_gpu.py uses, and the bounds that follow (16 x: fp32 tile partials and another summation order).  The bounds come from the reference's
own error, never from what the kernels give; the "gpu_reached" entries are a record of a run on an MI355X and are kept when the file is rewritten
(test_metrics_gpu.py prints them as METRICS_MEASURED lines).  Usage: python tests/golden/make_metrics_measured.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import metrics_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "metrics_measured.json")


def main():
    old = json.load(open(OUT)) if os.path.exists(OUT) else {}
    dev_val, dev_tab, per_case = 0.0, 0.0, {}
    for name, *_ in R.MS_CASES:
        for form in R.MS_FORMS[name]:
            p, t, sc = R.ms_inputs(name, form)
            v64, t64 = R.ms_ssim(p, t, sc, dtype=torch.float64)
            v32, t32 = R.ms_ssim(p, t, sc, dtype=torch.float32)
            dv, dt = float((v32.double() - v64).abs().max()), float((t32.double() - t64).abs().max())
            per_case[f"{name}/{form}"] = {"result": dv, "scale_mean": dt}
            dev_val, dev_tab = max(dev_val, dv), max(dev_tab, dt)
    dev_rmse, per_rmse = 0.0, {}
    for H, W, smax in R.RMSE_CASES:
        pred, label = R.rmse_inputs(H, W, smax)
        d = float((R.rmse(pred, label, smax, torch.float32).double() - R.rmse(pred, label, smax, torch.float64)).abs().max())
        per_rmse[f"{H}x{W}/{'max' if smax else 'plain'}"] = d
        dev_rmse = max(dev_rmse, d)
    rec = {
        "ms_ssim": {"fp32_vs_fp64_result": dev_val, "fp32_vs_fp64_scale_mean": dev_tab, "bound_result": 16 * dev_val, "bound_scale_mean": 16 * dev_tab,
                    "fp32_vs_fp64_per_case": per_case, "gpu_reached": old.get("ms_ssim", {}).get("gpu_reached")},
        "rmse": {"fp32_vs_fp64": dev_rmse, "bound": 16 * dev_rmse, "fp32_vs_fp64_per_case": per_rmse, "gpu_reached": old.get("rmse", {}).get("gpu_reached")},
    }
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
