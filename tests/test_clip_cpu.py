"""CPU: the host-side pieces of the CLIP score (controlar_amd/clip.py, synth.clip_*, the requant table of libcontrolar_hip.so) against torch, PIL and the
goldens of tests/golden/make_clip_golden.py.  No GPU."""
import ctypes as C
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_requant_table_is_the_torch_round_trip_and_not_the_identity():
    from controlar_amd import _lib as L
    from controlar_amd.clip import requant_table
    u = torch.arange(256, dtype=torch.float32)
    want = (((u / 255.0 - 0.5) / 0.5 + 1.0) * 127.5).clamp(0.0, 255.0).to(torch.uint8)      # ToTensor, Normalize(0.5, 0.5), tensor2pil
    got = np.zeros(256, dtype=np.uint8)
    assert L.load().car_debug_clip_requant_table(C.c_void_p(got.ctypes.data)) == 0
    assert np.array_equal(got, want.numpy())
    assert torch.equal(requant_table(), want)
    changed = int((want != torch.arange(256, dtype=torch.uint8)).sum())
    assert changed == 63, changed
    assert int(want[1]) == 0 and int(want[0]) == 0 and int(want[255]) == 255


def test_photo_depicts_ids_hand_written_cases():
    from controlar_amd.clip import photo_depicts_ids
    S, E, P = 900, 901, [11, 12, 13]
    T = 77

    def row(body):                       # start, caption ids, end of text, zeros
        r = [S] + body + [E]
        return r + [0] * (T - len(r))

    short = row([5, 6])                                          # 4 tokens
    fits = row(list(range(100, 172)))                            # 74 tokens: 77 after the shift, the end-of-text id lands in the last column
    full = row(list(range(100, 175)))                            # 77 tokens: the shift pushes the end-of-text id out, the last column is forced
    zero_last = row(list(range(100, 171)))                       # 73 tokens: the last column is still 0 after the shift
    ids = torch.tensor([short, fits, full, zero_last], dtype=torch.int64)
    assert ids.shape == (4, T) and ids[2, 76] == E and ids[1, 73] == E and ids[1, 74] == 0
    out = photo_depicts_ids(ids, P, E)
    assert out.shape == (4, T) and out.dtype == torch.int64
    assert out[0].tolist() == [S, 11, 12, 13, 5, 6, E] + [0] * (T - 7)
    assert out[1].tolist() == [S, 11, 12, 13] + list(range(100, 172)) + [E]
    assert out[2].tolist() == [S, 11, 12, 13] + list(range(100, 172)) + [E]          # ids 172..174 and the old end-of-text id fell off
    assert out[3].tolist() == [S, 11, 12, 13] + list(range(100, 171)) + [E, 0] and out[3, 76] == 0
    assert ids[2, 76] == E and ids[0, 1] == 5                                       # the input is not modified
    # a last column that is occupied by a caption id (not the end-of-text id) is overwritten
    assert full[76] == E and photo_depicts_ids(ids, P, 777)[2, 76] == 777


def _openai_names(hf, cfg):
    """The inverse mapping, written out independently: what clip.load(...).state_dict() would call these tensors."""
    o = {}
    for tower, src in (("visual.transformer.resblocks.", "vision_model."), ("transformer.resblocks.", "text_model.")):
        n_layers = cfg.vision_layers if src == "vision_model." else cfg.text_layers
        for i in range(n_layers):
            p, q = f"{src}encoder.layers.{i}.", f"{tower}{i}."
            for kind in ("weight", "bias"):
                o[q + f"attn.in_proj_{kind}"] = torch.cat([hf[p + f"self_attn.{n}_proj.{kind}"] for n in "qkv"], dim=0)
                o[q + f"attn.out_proj.{kind}"] = hf[p + f"self_attn.out_proj.{kind}"]
                o[q + f"ln_1.{kind}"], o[q + f"ln_2.{kind}"] = hf[p + f"layer_norm1.{kind}"], hf[p + f"layer_norm2.{kind}"]
                o[q + f"mlp.c_fc.{kind}"], o[q + f"mlp.c_proj.{kind}"] = hf[p + f"mlp.fc1.{kind}"], hf[p + f"mlp.fc2.{kind}"]
    o["visual.conv1.weight"] = hf["vision_model.embeddings.patch_embedding.weight"]
    o["visual.class_embedding"] = hf["vision_model.embeddings.class_embedding"]
    o["visual.positional_embedding"] = hf["vision_model.embeddings.position_embedding.weight"]
    o["visual.ln_pre.weight"], o["visual.ln_pre.bias"] = hf["vision_model.pre_layrnorm.weight"], hf["vision_model.pre_layrnorm.bias"]
    o["visual.ln_post.weight"], o["visual.ln_post.bias"] = hf["vision_model.post_layernorm.weight"], hf["vision_model.post_layernorm.bias"]
    o["visual.proj"] = hf["visual_projection.weight"].t().contiguous()
    o["token_embedding.weight"] = hf["text_model.embeddings.token_embedding.weight"]
    o["positional_embedding"] = hf["text_model.embeddings.position_embedding.weight"]
    o["ln_final.weight"], o["ln_final.bias"] = hf["text_model.final_layer_norm.weight"], hf["text_model.final_layer_norm.bias"]
    o["text_projection"] = hf["text_projection.weight"].t().contiguous()
    o["logit_scale"] = hf["logit_scale"]
    o["input_resolution"], o["context_length"], o["vocab_size"] = torch.tensor(cfg.image_size), torch.tensor(cfg.context_length), torch.tensor(cfg.vocab_size)
    return o


def test_from_openai_state_dict_round_trips_to_the_hf_key_set():
    from controlar_amd import config as Cfg, synth
    from controlar_amd.clip import from_openai_state_dict, is_openai_state_dict
    cfg = Cfg.tiny_clip()
    hf = synth.clip_state_dict(cfg)
    oa = _openai_names(hf, cfg)
    assert is_openai_state_dict(oa) and not is_openai_state_dict(hf)
    back = from_openai_state_dict(oa)
    assert set(back) == set(hf), set(back) ^ set(hf)
    for k in hf:
        assert back[k].shape == hf[k].shape and torch.equal(back[k], hf[k]), k


def test_synthetic_tokens_and_weights_are_seeded_and_shaped():
    from controlar_amd import config as Cfg, synth
    cfg = Cfg.tiny_clip()
    ids = synth.clip_tokens(4, cfg, lengths=[2, 9, 40, 77])
    assert ids.shape == (4, 77) and ids.dtype == torch.int64 and torch.equal(ids, synth.clip_tokens(4, cfg, lengths=[2, 9, 40, 77]))
    for b, L in enumerate([2, 9, 40, 77]):
        assert ids[b, L - 1] == cfg.eot_id and (ids[b, :L - 1] < cfg.eot_id).all() and (ids[b, :L - 1] > 0).all() and (ids[b, L:] == 0).all()
    a, b = synth.clip_state_dict(cfg, seed=3), synth.clip_state_dict(cfg, seed=3)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert a["vision_model.embeddings.position_embedding.weight"].shape == (cfg.grid ** 2 + 1, cfg.vision_width)
    full = Cfg.clip_vit_b32()
    assert (full.vision_width, full.vision_layers, full.vision_heads, full.vision_mlp, full.patch, full.image_size) == (768, 12, 12, 3072, 32, 224)
    assert (full.text_width, full.text_layers, full.text_heads, full.text_mlp, full.vocab_size, full.context_length, full.proj_dim) == (512, 12, 8, 2048, 49408, 77, 512)
    assert full.eot_id == 49407


def test_preprocess_restatement_equals_golden_pixel_values_bit_for_bit():
    """landscape 40x64, portrait 64x40, odd 37x53 (the resized long side is 45: the crop offset 6.5 rounds to even), square 48x48; with and without the
    requant table in front.  The restatement here is written with PIL and torch alone."""
    from PIL import Image
    from controlar_amd.clip import center_crop_offset, clip_resized_size, preprocess_reference, requant_table
    g = np.load(os.path.join(GOLD, "clip_tiny.npz"))
    n = g["pixel_values"].shape[-1]
    assert n == 32
    mean = torch.tensor([0.48145466, 0.4578275, 0.40821073])[:, None, None]
    std = torch.tensor([0.26862954, 0.26130258, 0.27577711])[:, None, None]
    shapes = set()
    assert clip_resized_size(37, 53, 32) == (32, 45) and center_crop_offset(45, 32) == 6 and center_crop_offset(51, 32) == 10 and center_crop_offset(33, 32) == 0
    for i in range(4):
        src = g[f"img{i}"]
        H, W, _ = src.shape
        shapes.add("square" if H == W else "landscape" if W > H else "portrait")
        for key, a in (("pixel_values", src), ("pixel_values_requant", requant_table().numpy()[src])):
            short, long_ = min(H, W), max(H, W)
            new_long = int(n * long_ / short)
            Wr, Hr = (new_long, n) if W >= H else (n, new_long)
            im = Image.fromarray(a, "RGB").resize((Wr, Hr), Image.BICUBIC)
            top, left = int(round((Hr - n) / 2.0)), int(round((Wr - n) / 2.0))
            im = im.crop((left, top, left + n, top + n))
            x = torch.from_numpy(np.array(im)).permute(2, 0, 1).float().div(255)
            want = ((x - mean) / std).numpy()
            assert np.array_equal(want, g[key][i]), (i, key)
            assert np.array_equal(preprocess_reference(torch.from_numpy(a), n).numpy(), g[key][i]), (i, key)
    assert shapes == {"square", "landscape", "portrait"}
    assert not np.array_equal(g["pixel_values"], g["pixel_values_requant"])


def test_golden_text_pooling_is_the_first_end_of_text_position():
    from controlar_amd import config as Cfg
    for name, cfg in (("clip_tiny", Cfg.tiny_clip()), ("clip_small", Cfg.small_clip()), ("clip_b32", Cfg.clip_vit_b32())):
        g = np.load(os.path.join(GOLD, name + ".npz"))
        ids = torch.from_numpy(g["ids"])
        assert ids.shape == (4, 77)
        assert torch.equal(ids.argmax(dim=-1), torch.from_numpy(g["pool_index"]))
        assert g["pool_index"].tolist() == [1, 8, 39, 76]
        assert (ids.max(dim=-1).values == cfg.eot_id).all()


def test_clip_score_accumulator_cuts_at_how_many():
    """CLIPScore needs no GPU of its own: a stand-in scorer returns known cosines."""
    from controlar_amd.metrics import CLIPScore

    class Fake:
        device = torch.device("cpu")

        def score(self, pixels, ids, eval_res=256):
            return pixels.reshape(pixels.shape[0], -1)[:, 0].float()

    m = CLIPScore(Fake(), how_many=5)
    m.update(torch.tensor([0.1, 0.2, 0.3])[:, None], None)
    m.update(torch.tensor([0.4, 0.5, 0.6])[:, None], None)
    assert m.per_image.shape == (6,)
    assert abs(m.calculate() - float(torch.tensor([0.1, 0.2, 0.3, 0.4, 0.5], dtype=torch.float32).double().mean())) < 1e-15
