"""Bit-level pin of the entries that run the batched multi-head attention on the host side: the SHA-256 of every output of Engine.encode_control,
t5_encode, clip_encode_image, clip_encode_text, score and generate on synthetic weights (controlar_amd.synth) and the inputs of tests/cases.py, in both
arithmetic modes.  The cases take every attention form the host code builds: planes and the packed wqkv layout, no mask / causal + pad mask / T5 bias +
key mask, the fused kernel (bf16, 64-wide heads) and the GEMM / softmax / GEMM form (fp32; tiny_t5's 32-wide heads in both modes), a prefill window that
starts past column 0, more than one chunk.  A change that is meant to keep the bits (moving host code, a new build flag) must reproduce
tests/golden/encoder_bits.json (tests/test_encoder_bits_gpu.py); a change that is meant to move them re-mints the file and says so.  Needs a GPU.
(car_depth runs the same attention: tests/golden/extractor_bits.json pins it.)
usage: python tests/golden/make_encoder_bits.py [--out tests/golden/encoder_bits.json] [--modes fp32,bf16]"""
import argparse
import hashlib
import json
import os
import sys

import torch

GOLDEN = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(GOLDEN)))

MODES = ("fp32", "bf16")
ENCODE_CASES = ("tiny_t2i", "tiny_c2i", "tiny_t2i_base")      # DINOv2 form, 2 heads, LayerScale | ViT form | 3 heads; 3 images of 48 x 32: 7 rows padded to 32
T5_CASES = {"tiny_t5/b3": ("tiny_t5", 3), "small_t5/b3": ("small_t5", 3), "tiny_t5/b65": ("tiny_t5", 65)}     # d_kv 32: unfused in both modes | 8 x 64: fused in bf16 | two chunks
T5_LENGTHS = [1, 120, 40]
CLIP_CASES = {"tiny_clip": (3, (40, 56)), "small_clip": (2, (96, 72))}      # 5 and 50 vision rows
CLIP_TEXT_LENGTHS = [2, 30, 77]                                              # three captions per configuration
GPT_CASES = ("tiny_depth_cfg4", "tiny_mask_edges", "tiny_t2i_window")       # CFG pair | lengths 1, 120, 40 | first valid position 80: the window starts past column 0
WINDOW_LENGTHS = [1, 40, 17]
N_KEYS = len(MODES) * (len(ENCODE_CASES) + len(T5_CASES) + 2 * len(CLIP_CASES) + 2 * len(GPT_CASES) + 2 * (len(GPT_CASES) + 1))


def _sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def _gpt_case(name):
    """cfg, GPT weights, control image, text embeddings, mask and the sampling arguments of one t2i case"""
    from controlar_amd import config as Cfg, synth
    from tests.cases import load_case
    if name != "tiny_t2i_window":
        cs = load_case(name)
        return cs["cfg"], cs["gsd"], cs["img"], cs["emb"], cs["mask"], dict(cfg_scale=cs["cfg_scale"], cfg_interval=cs["cfg_interval"],
                                                                            control_strength=cs["control_strength"]), cs["n_new"]
    cfg = Cfg.tiny_t2i(64, "canny")
    emb, mask = synth.text_embeddings_with_lengths(WINDOW_LENGTHS, cfg.gpt.cls_token_num, cfg.gpt.caption_dim)
    return cfg, synth.path_state_dicts(cfg, seed=0)[0], synth.canny_like_control(3, 128, 128), emb, mask, dict(cfg_scale=2.0), 64


def _tokens(B, n_new, V, seed=11):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, V, (B, n_new), generator=g, dtype=torch.int32)
    t[:, 0] = 0; t[:, 1] = V - 1; t[0, -1] = V - 1; t[-1, -1] = 0
    return t


def digests(modes=MODES):
    """{"<entry>/<mode>/<case>/<output>": sha256 of the tensor's bytes}"""
    from controlar_amd import config as Cfg, synth
    from controlar_amd.engine import Engine
    res = {}

    def put(key, t):
        torch.cuda.synchronize()
        res[key] = _sha(t)

    for prec in modes:
        for cn in ENCODE_CASES:
            cfg = getattr(Cfg, cn)()
            eng = Engine(cfg, prec)
            eng.load_state_dict(synth.path_state_dicts(cfg, seed=0)[0]); eng.finalize()
            img = synth.smooth_control(3, 48, 32) if cn == "tiny_t2i_base" else synth.canny_like_control(3, 48, 32)
            put(f"encode_control/{prec}/{cn}/control", eng.encode_control(img.cuda(), want_output=True))
            eng.close()
        for cn in ("tiny_t5", "small_t5"):
            cfg = getattr(Cfg, cn)()
            eng = Engine(Cfg.tiny_t2i(), prec)
            eng.t5_configure(cfg)
            eng.load_t5_state_dict(synth.t5_state_dict(cfg))
            for name, (c, B) in T5_CASES.items():
                if c == cn:
                    ids, mask = synth.t5_tokens(B, cfg, lengths=T5_LENGTHS if B == 3 else None)
                    put(f"t5_encode/{prec}/{name}/out", eng.t5_encode(ids.cuda(), mask.cuda()))
            eng.close()
        for cn, (B, size) in CLIP_CASES.items():
            cfg = getattr(Cfg, cn)()
            eng = Engine(Cfg.tiny_t2i(), prec)
            eng.clip_configure(cfg)
            eng.load_clip_state_dict(synth.clip_state_dict(cfg))
            put(f"clip_encode_image/{prec}/{cn}/emb", eng.clip_encode_image(torch.stack(synth.clip_images([size] * B)).cuda()))
            put(f"clip_encode_text/{prec}/{cn}/emb", eng.clip_encode_text(synth.clip_tokens(3, cfg, lengths=CLIP_TEXT_LENGTHS).cuda()))
            eng.close()
        for name in GPT_CASES:
            cfg, gsd, img, emb, mask, kw, n_new = _gpt_case(name)
            toks = _tokens(emb.shape[0], n_new, cfg.gpt.vocab_size)
            eng = Engine(cfg, prec)
            eng.load_state_dict(gsd); eng.finalize()
            eng.encode_control(img.cuda())
            nll, logits = eng.score(emb.cuda(), toks.cuda(), emb_masks=mask.cuda(), return_logits=True, **kw)
            put(f"score/{prec}/{name}/nll", nll)
            put(f"score/{prec}/{name}/logits", logits)
            out, logits = eng.generate(emb.cuda(), n_new, mask.cuda(), forced_tokens=toks, return_logits=True, **kw)
            put(f"generate/{prec}/{name}/logits", logits)
            put(f"generate/{prec}/{name}/tokens", out)
            eng.close()
        cfg = Cfg.tiny_c2i(64)                                   # no mask, one prefix row
        eng = Engine(cfg, prec)
        eng.load_state_dict(synth.path_state_dicts(cfg, seed=0)[0]); eng.finalize()
        eng.encode_control(synth.canny_like_control(3, 128, 128).cuda())
        out, logits = eng.generate(torch.tensor([1, cfg.gpt.num_classes - 1, 0]).cuda(), 64, None, cfg_scale=1.0,
                                   forced_tokens=_tokens(3, 64, cfg.gpt.vocab_size), return_logits=True)
        put(f"generate/{prec}/tiny_c2i/logits", logits)
        put(f"generate/{prec}/tiny_c2i/tokens", out)
        eng.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(GOLDEN, "encoder_bits.json"))
    ap.add_argument("--modes", default=",".join(MODES), help="comma-separated subset of the modes (a kernel trace of one mode)")
    a = ap.parse_args()
    d = digests(tuple(a.modes.split(",")))
    with open(a.out, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(d)} digests -> {a.out}")
