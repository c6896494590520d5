"""Bit-level pin of the packed weight images: every entry that car_export_packed writes (the device images of car_ctx::w and the host tables of
car_ctx::host_keep), by name, with its kind, shape, numel, byte count and the first 16 hex characters of the SHA-256 of its payload, for three
contexts: fp32 and bf16 holding every model family (tiny_t2i GPT + ViT, VQ with the encoder, tiny_t5, LineArt, HED, tiny_dpt) and bf16 with
decode_weight_fp8 holding the GPT alone.  The state dicts have the shapes of synth.*_state_dict; every tensor is refilled with
((arange(n) * 2654435761 + crc32(name)) % 251 - 125) / 64: no RNG, and every value is exact in bf16.
A change to car_load_tensor / car_finalize_weights that is meant to keep the layouts must reproduce tests/golden/packed_digests.json
(tests/test_packed_layout_gpu.py).  The file is minted on the build of the commit named in its "parent" field, never on the tree under test.  Needs a GPU.
usage: python tests/golden/make_packed_digests.py --parent <commit hash> [--out tests/golden/packed_digests.json] [--verbose]"""
import argparse
import ctypes
import hashlib
import json
import os
import struct
import sys
import tempfile
import zlib

import torch

GOLDEN = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(GOLDEN)))

CONTEXTS = {"fp32": ("fp32", False, True), "bf16": ("bf16", False, True), "bf16_fp8": ("bf16", True, False)}     # precision, weights_fp8, every family


def refill(sd, prefix=""):
    """The same names and shapes, every value a function of the tensor's full name and the element index."""
    out = {}
    for k, v in sd.items():
        name = prefix + k
        i = torch.arange(v.numel(), dtype=torch.int64)
        out[name] = (((i * 2654435761 + zlib.crc32(name.encode())) % 251 - 125).to(torch.float32) / 64).reshape(v.shape)
    return out


def parse_packed(path):
    """{entry name: [kind, shape, numel, bytes, sha256[:16]]} of a car_export_packed file (layout: the comment above kPackMagic in engine_weights.hip)."""
    from controlar_amd import _lib as L
    res = {}
    with open(path, "rb") as f:
        magic = f.read(8)
        assert magic[:5] == b"CARPK", magic
        f.read(48)                                      # build id: differs between any two builds
        f.read(ctypes.sizeof(L.CarConfig))
        (n,) = struct.unpack("<Q", f.read(8))
        for _ in range(n):
            kind, nl = struct.unpack("<II", f.read(8))
            name = f.read(nl).decode()
            (nd,) = struct.unpack("<I", f.read(4))
            shape = list(struct.unpack(f"<{nd}q", f.read(8 * nd)))
            numel, nbytes = struct.unpack("<qQ", f.read(16))
            payload = f.read(nbytes)
            assert len(payload) == nbytes and name not in res, name
            res[name] = [kind, shape, numel, nbytes, hashlib.sha256(payload).hexdigest()[:16]]
        assert f.read(1) == b""
    return res


def digests():
    """{context: {entry name: [kind, shape, numel, bytes, sha256[:16]]}}"""
    from controlar_amd import config as Cfg, synth
    from controlar_amd.engine import Engine
    cfg = Cfg.tiny_t2i(64, "canny")
    gsd, vsd = synth.path_state_dicts(cfg, seed=0)
    gsd, vsd = refill(gsd), refill(vsd)
    t5c, dc = Cfg.tiny_t5(), Cfg.tiny_dpt()
    t5, la, hed = refill(synth.t5_state_dict(t5c), "t5."), refill(synth.lineart_state_dict(), "lineart."), refill(synth.hed_state_dict(), "hed.")
    dpt = refill(synth.dpt_state_dict(dc), "depth.")
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for ctx, (prec, fp8, every) in CONTEXTS.items():
            eng = Engine(cfg, prec, weights_fp8=fp8)
            eng.load_state_dict(gsd)
            if every:
                eng.load_state_dict(vsd)
                eng.t5_configure(t5c)
                eng.depth_configure(dc)
                for sd in (t5, la, hed, dpt):
                    eng.load_state_dict(sd)
            eng.finalize()
            path = os.path.join(tmp, ctx + ".pack")
            eng._check(eng.lib.car_export_packed(eng._h, path.encode()), "car_export_packed")
            eng.close()
            res[ctx] = parse_packed(path)
            os.remove(path)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(GOLDEN, "packed_digests.json"))
    ap.add_argument("--parent", required=True, help="hash of the commit whose build mints the file")
    ap.add_argument("--verbose", action="store_true", help="print every entry")
    a = ap.parse_args()
    d = digests()
    if a.verbose:
        for ctx in d:
            for name in sorted(d[ctx]):
                print(ctx, name, *d[ctx][name])
    with open(a.out, "w") as f:                          # one entry per line
        ctxs = [f' {json.dumps(c)}: {{\n' + ",\n".join(f"  {json.dumps(n)}: {json.dumps(d[c][n], separators=(',', ':'))}" for n in sorted(d[c])) + "\n }"
                for c in sorted(d)]
        f.write(f'{{"parent": {json.dumps(a.parent)}, "contexts": {{\n' + ",\n".join(ctxs) + "\n}}\n")
    print(f"{ {c: len(v) for c, v in d.items()} } entries -> {a.out}")
