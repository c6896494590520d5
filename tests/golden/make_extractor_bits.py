"""Bit-level pin of the three control extractors: the SHA-256 of every output of Engine.hed / Engine.depth / Engine.lineart on the inputs of the
committed fixtures (hed_*.npz, depth_*.npz, lineart_*.npz) with the synthetic weights their tests use, in both arithmetic modes, map and control tensor.
A change that is meant to keep the bits (a refactor of the kernels, a new build flag) must reproduce tests/golden/extractor_bits.json
(tests/test_extractor_bits_gpu.py); a change that is meant to move them re-mints the file and says so.  Needs a GPU.
usage: python tests/golden/make_extractor_bits.py [--out tests/golden/extractor_bits.json]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(GOLDEN)))

HED_CASES = ["b2_16x24", "b1_17x31", "b1_35x50", "b1_72x104"]
LINEART_CASES = ["b2_16x24", "b1_30x44", "b1_8x8", "b1_72x104"]
DEPTH_CASES = {"b2_32": "tiny_dpt", "b1_64": "tiny_dpt", "b1_96": "tiny_dpt", "b1_128": "tiny_dpt", "wide_b1_64": "tiny_dpt_wide"}
HED_SEED, LINEART_SEED, DEPTH_SEED = 11, 11, 13          # the weight seeds of tests/test_{hed,lineart,depth}_gpu.py


def _x(kind, name):
    return torch.from_numpy(np.load(os.path.join(GOLDEN, f"{kind}_{name}.npz"))["x"])


def _sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def digests():
    """{"<extractor>/<mode>/<case>/<map|control>": sha256 of the tensor's bytes}"""
    from controlar_amd import config as Cfg, synth
    from controlar_amd.engine import Engine
    res = {}

    def put(kind, prec, name, out, ctrl):
        torch.cuda.synchronize()
        res[f"{kind}/{prec}/{name}/map"] = _sha(out)
        res[f"{kind}/{prec}/{name}/control"] = _sha(ctrl)

    for prec in ("fp32", "bf16"):
        eng = Engine(Cfg.tiny_t2i(), prec)
        eng.load_hed(synth.hed_state_dict(HED_SEED))
        for name in HED_CASES:
            put("hed", prec, name, *eng.hed(_x("hed", name), want_control=True))
        eng.close()
        eng = Engine(Cfg.tiny_t2i(), prec)
        eng.load_lineart(synth.lineart_state_dict(LINEART_SEED))
        for name in LINEART_CASES:
            put("lineart", prec, name, *eng.lineart(_x("lineart", name), want_control=True))
        eng.close()
        for cn in ("tiny_dpt", "tiny_dpt_wide"):
            cfg = getattr(Cfg, cn)()
            eng = Engine(Cfg.tiny_t2i(), prec)
            eng.load_depth(synth.dpt_state_dict(cfg, DEPTH_SEED), cfg)
            for name in [n for n, c in DEPTH_CASES.items() if c == cn]:
                pv = (_x("depth", name).to(torch.float32) / 255 - 0.5) / 0.5
                put("depth", prec, name, *eng.depth(pv, want_control=True))
            eng.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(GOLDEN, "extractor_bits.json"))
    a = ap.parse_args()
    d = digests()
    with open(a.out, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(d)} digests -> {a.out}")
