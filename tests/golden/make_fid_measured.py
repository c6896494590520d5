"""Writes tests/golden/fid_measured.json: the largest deviation of the Inception Score in the script's literal fp32 arithmetic from the fp64 restatement
(tests/fid_ref.py) on exactly the inputs of the GPU test.  The GPU test allows 16 x that deviation (the rule of DESIGN.md §6f: a tolerance comes from the
reference's own error, never from the code under test).  Run from the repository root: python tests/golden/make_fid_measured.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fid_ref as R  # noqa: E402


def main():
    acts, w = R.is_inputs()
    s64, p64 = R.inception_score(acts, w, R.IS_SPLIT, np.float64)
    s32, p32 = R.inception_score(acts, w, R.IS_SPLIT, np.float32)
    dev = float(max(abs(s32 - s64), np.max(np.abs(p32 - p64))))
    out = {"inception_score": {"N": R.IS_N, "split": R.IS_SPLIT, "D": R.IS_D, "C": R.IS_C, "score_fp64": s64, "splits_fp64": [float(v) for v in p64],
                               "fp32_vs_fp64_max_abs": dev, "tolerance_factor": 16}}
    with open(os.path.join(HERE, "fid_measured.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
