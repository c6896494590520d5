"""GPU parity tests (pytest -m gpu): the HIP path, called through the C ABI, against
(a) golden vectors minted from the unmodified reference and (b) the CPU oracle on the same inputs.

Contract:
  * exact mode (fp32): greedy VQ token indices bit-identical to the fp32 CPU reference; logits,
    control tokens and pixels within fp32 round-off (tolerances below).
  * fast mode (bf16): graded teacher-forced (reference bf16 is itself not thread-stable):
    per-step logits max|d| <= 0.6*k and mean|d| <= 0.08*k vs the fp32 reference (k = 1, or sqrt(s^2+(s-1)^2)
    under CFG scale s, because the mix u+(c-u)*s amplifies single-pass error); arg-max equal wherever the
    reference top-2 margin > 0.25*k; pixels max|d| <= 0.32 / mean|d| <= 0.024 on the random-init decoder (2 x measured: ADVICE r5).
"""
import numpy as np
import pytest
import torch

from tests.cases import record_measured, CASES, load_case

pytestmark = pytest.mark.gpu


def _mask(cs):
    return cs["mask"].cuda() if cs["mask"] is not None else None


def _engine(cs, prec, dev=None):
    from controlar_amd.engine import Engine
    eng = Engine(cs["cfg"], prec, dev=dev)
    eng.load_state_dict(cs["gsd"]); eng.load_state_dict(cs["vsd"]); eng.finalize()
    return eng


@pytest.mark.parametrize("name", list(CASES))
def test_exact_mode_tokens_bit_identical(name):
    from oracle import controlar_oracle as O
    cs = load_case(name); gold = cs["gold"]
    eng = _engine(cs, "fp32")
    a = eng.encode_control(cs["img"].cuda(), want_output=True).cpu()
    toks, logits = eng.generate(cs["emb"].cuda(), cs["n_new"], _mask(cs), cfg_scale=cs["cfg_scale"],
                                cfg_interval=cs["cfg_interval"], control_strength=cs["control_strength"], return_logits=True)
    np.testing.assert_allclose(a.numpy()[:, ::7, ::5], gold["adapter_mlp_out"], atol=5e-5, rtol=1e-4)
    assert np.array_equal(toks.cpu().numpy(), gold["tokens"])
    np.testing.assert_allclose(logits.cpu().numpy(), gold["logits"], atol=5e-4, rtol=1e-4)
    # full-tensor check of the cached control tokens against the oracle
    _, st = O.generate(cs["gsd"], cs["cfg"], cs["emb"], 1, cs["mask"], cfg_scale=cs["cfg_scale"], condition=cs["img"],
                       control_strength=cs["control_strength"], return_stages=True)
    b = 2 * cs["B"] if cs["cfg_scale"] > 1 else cs["B"]
    for k in range(3):
        c = eng.control_tokens(k, b, cs["n_new"])
        np.testing.assert_allclose(c[: cs["B"]].numpy(), st["ctrl"][k][: cs["B"]].numpy(), atol=5e-5, rtol=1e-4)
        if b > cs["B"]:
            assert float(c[cs["B"]:].abs().max()) == 0.0          # uncond half is exactly zero (generate.py:161-162)
    if "pixels" in gold:
        px = eng.vq_decode(toks, cs["H"] // 16, cs["W"] // 16).cpu().numpy()
        np.testing.assert_allclose(px, gold["pixels"], atol=5e-4, rtol=1e-4)
    assert eng.stats()["graph_used"]
    eng.close()


@pytest.mark.parametrize("name", ["tiny_canny_cfg1", "tiny_depth_cfg4", "tiny_mr_192x128"])
def test_fast_mode_teacher_forced(name):
    cs = load_case(name); gold = cs["gold"]
    eng = _engine(cs, "bf16")
    eng.encode_control(cs["img"].cuda())
    forced = torch.from_numpy(gold["tokens"])
    toks, logits = eng.generate(cs["emb"].cuda(), cs["n_new"], _mask(cs), cfg_scale=cs["cfg_scale"],
                                cfg_interval=cs["cfg_interval"], control_strength=cs["control_strength"],
                                forced_tokens=forced, return_logits=True)
    d = np.abs(logits.cpu().numpy() - gold["logits"])
    # CFG mixes u + (c-u)*s: single-pass logit errors enter with weights s and (s-1)
    s_ = cs["cfg_scale"]
    k = 1.0 if s_ <= 1 else float(np.sqrt(s_ ** 2 + (s_ - 1) ** 2))
    assert d.max() <= 0.6 * k and d.mean() <= 0.08 * k, (d.max(), d.mean(), k)
    safe = gold["margin"] > 0.25 * k
    agree = (toks.cpu().numpy() == gold["tokens"])
    assert agree[safe].all(), f"arg-max differs on {int((~agree[safe]).sum())} safe-margin steps"
    assert agree.mean() > 0.85
    if "pixels" in gold:
        px = eng.vq_decode(forced, cs["H"] // 16, cs["W"] // 16).cpu().numpy()
        dp = np.abs(px - gold["pixels"])
        record_measured(f"pixels_bf16[{name}]", max_abs_diff=dp.max(), mean_abs_diff=dp.mean())
        # 1.5 x the deviation measured on MI355X (0.159 / 0.012, profiles/r05_parity_measured.jsonl; the reference's own bf16-vs-fp32 pixels: 0.132 / 0.0094)
        assert dp.max() <= 0.32 and dp.mean() <= 0.024, (dp.max(), dp.mean())
    eng.close()


@pytest.mark.parametrize("prec,atol,mtol", [("fp32", 2e-3, 1e-4), ("bf16", 0.32, 0.024)])      # bf16: 2 x measured (profiles/r05_parity_measured.jsonl)
def test_vq16_real_architecture(prec, atol, mtol):
    """The real VQ-16 decoder (ch=128, z=256, 16384x8 codebook) on an 8x8 token grid vs the reference."""
    import os
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    from tests.cases import GOLDEN
    gold = np.load(os.path.join(GOLDEN, "vq16_real_8x8.npz"))
    cfg = C.tiny_t2i(64, "canny"); cfg.vq = C.VQConfig()
    gsd, _ = synth.path_state_dicts(cfg, seed=0)
    eng = Engine(cfg, prec)
    eng.load_state_dict(gsd); eng.load_state_dict(synth.vq_state_dict(cfg.vq, seed=2)); eng.finalize()
    px = eng.vq_decode(torch.from_numpy(gold["tokens"]), 8, 8).cpu().numpy()
    d = np.abs(px - gold["pixels"])
    record_measured(f"vq16_8x8[{prec}]", max_abs_diff=d.max(), mean_abs_diff=d.mean())
    assert d.max() <= atol and d.mean() <= mtol, (d.max(), d.mean())
    eng.close()


def test_generate_is_deterministic_and_repeatable():
    """Same inputs twice (graph reuse on the second call) -> identical tokens; KV buffers are not re-zeroed
    between calls, so this also checks that stale cache rows are never observed."""
    cs = load_case("tiny_depth_cfg4")
    eng = _engine(cs, "bf16")
    outs = []
    for _ in range(3):
        eng.encode_control(cs["img"].cuda())
        outs.append(eng.generate(cs["emb"].cuda(), cs["n_new"], _mask(cs), cfg_scale=cs["cfg_scale"],
                                 control_strength=cs["control_strength"]).cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    # a VQ decode in the SAME context re-sizes shared workspaces: the cached decode graph must not be replayed with stale pointers
    px = eng.vq_decode(outs[0], cs["H"] // 16, cs["W"] // 16)
    big = eng.vq_decode(outs[0].repeat(8, 1), cs["H"] // 16, cs["W"] // 16)
    assert bool(torch.isfinite(px).all()) and bool(torch.isfinite(big).all())
    again = eng.generate(cs["emb"].cuda(), cs["n_new"], _mask(cs), cfg_scale=cs["cfg_scale"], control_strength=cs["control_strength"]).cpu()
    assert torch.equal(again, outs[0])
    # shorter request after a longer one (KV/graph re-sizing path, BASELINE config 4)
    short = eng.generate(cs["emb"].cuda(), 16, _mask(cs), cfg_scale=cs["cfg_scale"], control_strength=cs["control_strength"]).cpu()
    assert torch.equal(short, outs[0][:, :16])
    eng.close()


def test_exact_mode_is_batch_invariant(monkeypatch):
    """Exact mode: a sequence decodes to the same BITS alone and as a row of a larger batch (logits included) — every exact-mode kernel sums one
    fixed-order fp32 arithmetic per output and the split-KV attention cuts the cache at ABSOLUTE positions (512 rows per split) and folds the pos/512 + 1
    non-empty splits in position order (a batch-dependent split count would fold a row's softmax partial sums in another order).  At XL the same property is checked by `bench.py --precision fp32`: row 0 of a batch of 192 must
    reproduce all 1024 tokens of the B = 1 golden."""
    cs = load_case("tiny_depth_cfg4")
    eng = _engine(cs, "fp32", dev=True)                 # the development build of the library: the CAR_* schedule switches exist only there
    B = cs["B"]
    reps = 9                                            # 2 x 9 x B rows: another tile count and, before the fix, another split count
    eng.encode_control(cs["img"].cuda())
    t1, l1 = eng.generate(cs["emb"].cuda(), cs["n_new"], _mask(cs), cfg_scale=cs["cfg_scale"], control_strength=cs["control_strength"], return_logits=True)
    t1, l1 = t1.cpu(), l1.cpu()
    assert np.array_equal(t1.numpy(), cs["gold"]["tokens"])
    img, emb, mask = cs["img"].repeat(reps, 1, 1, 1), cs["emb"].repeat(reps, 1, 1), cs["mask"].repeat(reps, 1)
    eng.encode_control(img.cuda())
    t2, l2 = eng.generate(emb.cuda(), cs["n_new"], mask.cuda(), cfg_scale=cs["cfg_scale"], control_strength=cs["control_strength"], return_logits=True)
    t2, l2 = t2.cpu(), l2.cpu()
    for r in range(reps):
        assert torch.equal(t2[r * B:(r + 1) * B], t1), r
        assert torch.equal(l2[r * B:(r + 1) * B], l1), r
    # the two-chain schedule of large exact batches (engine_generate.hip: from 192 sequences up; forced here): chains are row ranges, a row's arithmetic is unchanged
    monkeypatch.setenv("CAR_CHAINS", "2")
    t3, l3 = eng.generate(emb.cuda(), cs["n_new"], mask.cuda(), cfg_scale=cs["cfg_scale"], control_strength=cs["control_strength"], return_logits=True)
    assert eng.stats()["graph_used"]
    assert torch.equal(t3.cpu(), t2) and torch.equal(l3.cpu(), l2)
    monkeypatch.setenv("CAR_PHASE_OFFSET", "0")
    t4 = eng.generate(emb.cuda(), cs["n_new"], mask.cuda(), cfg_scale=cs["cfg_scale"], control_strength=cs["control_strength"])
    assert torch.equal(t4.cpu(), t2)
    eng.close()


def test_exact_mode_prefill_window_invariance(monkeypatch):
    """The prefill runs on a window of the left-padded prefix chosen by the LONGEST prompt of the batch (engine_generate.hip).  In the exact mode a sequence must not
    notice: its tokens and logits are the same bits decoded alone (window of 24 of 120 rows), beside a 60-token prompt (72 rows), beside a full-length prompt (no
    window), and with the window switched off — the window starts on a multiple of 16 (k-blocks of the P.V product) and the row softmax sums every column in the
    lane of its absolute position (softmax_wave_kernel)."""
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    cfg = C.tiny_t2i(64, "canny")
    gsd, _ = synth.path_state_dicts(cfg, seed=0)
    T, cap, n_new = cfg.gpt.cls_token_num, cfg.gpt.caption_dim, 20
    img = synth.canny_like_control(3, 128, 128)
    emb, mask = synth.text_embeddings_with_lengths([9, 60, T], T, cap)
    eng = Engine(cfg, "fp32", dev=True); eng.load_state_dict(gsd); eng.finalize()

    def run(rows):
        eng.encode_control(img[rows].cuda())
        t, l = eng.generate(emb[rows].cuda(), n_new, mask[rows].cuda(), cfg_scale=1.0, return_logits=True)
        return t.cpu()[0], l.cpu()[0]
    t_alone, l_alone = run([0])
    for rows in ([0, 1], [0, 2], [0, 1, 2]):
        t, l = run(rows)
        assert torch.equal(t, t_alone) and torch.equal(l, l_alone), rows
    monkeypatch.setenv("CAR_NO_PREFILL_WINDOW", "1")
    t, l = run([0])
    assert torch.equal(t, t_alone) and torch.equal(l, l_alone)
    # CFG doubles the rows (cond | uncond share the mask): same property
    monkeypatch.delenv("CAR_NO_PREFILL_WINDOW")
    eng.encode_control(img[[0]].cuda()); t1, l1 = eng.generate(emb[[0]].cuda(), n_new, mask[[0]].cuda(), cfg_scale=3.0, return_logits=True)
    eng.encode_control(img[[0, 1]].cuda()); t2, l2 = eng.generate(emb[[0, 1]].cuda(), n_new, mask[[0, 1]].cuda(), cfg_scale=3.0, return_logits=True)
    assert torch.equal(t1.cpu()[0], t2.cpu()[0]) and torch.equal(l1.cpu()[0], l2.cpu()[0])
    eng.close()


def test_first_valid_hint_replaces_the_host_wait_and_is_checked_on_the_device():
    """car_sampling.first_valid_hint: a caller that knows where the shortest padding ends (a host-side mask) lets car_generate size its prefill window without
    reading the device mask back.  Same tokens as the read-back path; a hint beyond the true first valid position would drop prompt rows — the device notices
    and the next call on the context fails (sticky flag), as an out-of-range c2i label does."""
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    cfg = C.tiny_t2i(64, "canny")
    gsd, _ = synth.path_state_dicts(cfg, seed=0)
    T, cap = cfg.gpt.cls_token_num, cfg.gpt.caption_dim
    img = synth.canny_like_control(2, 128, 128)
    emb, mask = synth.text_embeddings_with_lengths([12, 30], T, cap)
    eng = Engine(cfg, "bf16"); eng.load_state_dict(gsd); eng.finalize()
    eng.encode_control(img.cuda())
    want = eng.generate(emb.cuda(), 16, mask.cuda(), cfg_scale=1.0).cpu()                       # device mask, no hint: read-back path
    got = eng.generate(emb.cuda(), 16, mask, cfg_scale=1.0).cpu()                               # host mask: hint derived for free (T - 30 = 90 -> window from 80)
    assert torch.equal(got, want)
    got = eng.generate(emb.cuda(), 16, mask.cuda(), cfg_scale=1.0, first_valid=40).cpu()        # a loose lower bound only costs time
    assert torch.equal(got, want)
    eng.generate(emb.cuda(), 16, mask.cuda(), cfg_scale=1.0, first_valid=T - 12)                # beyond the first valid position of the 30-token prompt
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="first_valid_hint"):
        eng.generate(emb.cuda(), 16, mask.cuda(), cfg_scale=1.0)
    got = eng.generate(emb.cuda(), 16, mask.cuda(), cfg_scale=1.0).cpu()                        # the flag is cleared by the call that reported it
    assert torch.equal(got, want)
    # a wrong hint must not go unnoticed by a caller that makes ONE call — a host mask is checked before anything is enqueued, stats() and close() report the flag
    with pytest.raises(RuntimeError, match="first_valid"):
        eng.generate(emb.cuda(), 16, mask, cfg_scale=1.0, first_valid=T - 12)
    eng.generate(emb.cuda(), 16, mask.cuda(), cfg_scale=1.0, first_valid=T - 12)
    with pytest.raises(RuntimeError, match="first_valid_hint"):
        eng.stats()
    eng.generate(emb.cuda(), 16, mask.cuda(), cfg_scale=1.0, first_valid=T - 12)
    with pytest.raises(RuntimeError, match="first_valid_hint"):
        eng.close()


def test_error_paths_raise():
    cs = load_case("tiny_canny_cfg1")
    from controlar_amd.engine import Engine
    eng = Engine(cs["cfg"], "bf16")
    with pytest.raises(RuntimeError):
        eng.generate(cs["emb"].cuda(), 8, _mask(cs))            # weights not finalized
    eng.load_state_dict(cs["gsd"])
    eng.finalize()
    with pytest.raises(RuntimeError):
        eng.generate(cs["emb"].cuda(), 8, _mask(cs))            # control tokens not encoded for this batch
    with pytest.raises(RuntimeError):
        eng.vq_decode(torch.zeros(1, 64, dtype=torch.int32), 8, 8)       # VQ weights not loaded
    eng.encode_control(cs["img"].cuda())
    with pytest.raises(RuntimeError):
        eng.generate(cs["emb"].cuda(), 4096, _mask(cs))          # beyond block_size
    eng.close()
    # a VQ width the helper kernels cannot take (GroupNorm(32) groups, its 512-channel workspace, conv_out's 8-channel loads) is refused before any launch
    from controlar_amd import config as C, synth
    cfg = C.tiny_t2i(64, "canny")
    cfg.vq = C.VQConfig(codebook_size=cfg.vq.codebook_size, z_channels=64, ch=36, ch_mult=(1,), num_res_blocks=1)
    eng = Engine(cfg, "bf16"); eng.load_state_dict(synth.vq_state_dict(cfg.vq, seed=3), finalize=True)
    with pytest.raises(RuntimeError, match="36 channels"):
        eng.vq_decode(torch.zeros(1, 64, dtype=torch.int32), 8, 8)
    with pytest.raises(RuntimeError, match="36 channels"):
        eng.vq_encode(torch.zeros(1, 3, 16, 16).cuda())
    eng.close()


def test_two_chain_decode_large_batch():
    """B=48 (cfg=1): 48 rows = 3 m-blocks in one chain (chains are only cut from 192 sequences up; the multi-chain schedules at this size
    are covered by test_chain_schedule_knobs_do_not_change_tokens, at the bench size by tests/test_bench_shapes_gpu.py); teacher-forced on the
    oracle's fp32 tokens the logits must stay within the fast-mode tolerance, and identical sequences in different m-blocks must agree."""
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    from oracle import controlar_oracle as O
    cfg = C.tiny_t2i(64, "canny")
    gsd, _ = synth.path_state_dicts(cfg, seed=0)
    B, H, W, n_new = 48, 128, 128, 24
    img = synth.canny_like_control(B, H, W)
    emb, mask = synth.text_embeddings(B, cfg.gpt.cls_token_num, cfg.gpt.caption_dim)
    toks_o, logits_o = O.generate(gsd, cfg, emb, n_new, mask, cfg_scale=1.0, condition=img, return_logits=True)
    eng = Engine(cfg, "bf16")
    eng.load_state_dict(gsd); eng.finalize()
    eng.encode_control(img.cuda())
    toks, logits = eng.generate(emb.cuda(), n_new, mask.cuda(), cfg_scale=1.0, forced_tokens=toks_o, return_logits=True)
    d = (logits.cpu() - logits_o).abs()
    assert d.max() <= 0.6 and d.mean() <= 0.08, (float(d.max()), float(d.mean()))
    per_row = d.amax(dim=(1, 2))
    assert float(per_row.max()) <= 0.6                       # every sequence of both chains
    # free-running: identical sequences in, identical tokens out regardless of which chain decodes them
    emb2 = emb.clone(); emb2[24:] = emb[:24]; mask2 = mask.clone(); mask2[24:] = mask[:24]; img2 = img.clone(); img2[24:] = img[:24]
    eng.encode_control(img2.cuda())
    t2 = eng.generate(emb2.cuda(), n_new, mask2.cuda(), cfg_scale=1.0).cpu()
    assert torch.equal(t2[:24], t2[24:])
    eng.close()


def test_dropin_api_matches_reference_signatures():
    """controlar_amd.generate.generate / GPT_models / VQ_models used exactly like sample_t2i.py:43-83,163-176."""
    from controlar_amd.generate import generate
    from controlar_amd.models import Transformer, VQModel
    cs = load_case("tiny_depth_cfg4"); gold = cs["gold"]; cfg = cs["cfg"]
    gpt = Transformer(cfg.gpt, cfg.vit).to("cuda", dtype=torch.float32)
    gpt.load_state_dict(cs["gsd"], strict=False); gpt.eval()
    vq = VQModel(cfg.vq); vq.to("cuda"); vq.eval(); vq.load_state_dict(cs["vsd"])
    toks = generate(gpt, cs["emb"].cuda(), cs["n_new"], _mask(cs), condition=cs["img"].cuda(), cfg_scale=cs["cfg_scale"],
                    temperature=1.0, top_k=0, top_p=1.0, sample_logits=False, control_strength=cs["control_strength"])
    assert toks.dtype == torch.int32 and tuple(toks.shape) == (cs["B"], cs["n_new"])
    assert np.array_equal(toks.cpu().numpy(), gold["tokens"])
    px = vq.decode_code(toks, [cs["B"], cfg.vq.codebook_embed_dim, cs["H"] // 16, cs["W"] // 16])
    np.testing.assert_allclose(px.cpu().numpy(), gold["pixels"], atol=5e-4, rtol=1e-4)
    # the reference's default call style: sample_logits=True, top_k, top_p, temperature (sample_t2i.py:163-170)
    s1 = generate(gpt, cs["emb"].cuda(), 16, _mask(cs), condition=cs["img"].cuda(), cfg_scale=cs["cfg_scale"], temperature=1.0,
                  top_k=200, top_p=0.95, sample_logits=True, seed=5)
    s2 = generate(gpt, cs["emb"].cuda(), 16, _mask(cs), condition=cs["img"].cuda(), cfg_scale=cs["cfg_scale"], temperature=1.0,
                  top_k=200, top_p=0.95, sample_logits=True, seed=5)
    s3 = generate(gpt, cs["emb"].cuda(), 16, _mask(cs), condition=cs["img"].cuda(), cfg_scale=cs["cfg_scale"], temperature=1.0,
                  top_k=200, top_p=0.95, sample_logits=True, seed=6)
    assert torch.equal(s1, s2) and not torch.equal(s1, s3)
    assert int(s1.min()) >= 0 and int(s1.max()) < cfg.gpt.vocab_size
    # no control image at all (condition=None) is a legal call of the reference too
    t0 = generate(gpt, cs["emb"].cuda(), 8, _mask(cs), condition=None, cfg_scale=1.0, sample_logits=False)
    assert tuple(t0.shape) == (cs["B"], 8)


def _golden_big(name, mk):
    import os
    from tests.cases import GOLDEN
    from controlar_amd import synth
    gold = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    B, H, W, seed, _ = [int(x) for x in gold["meta"]]
    cfg = mk()
    gsd, _ = synth.path_state_dicts(cfg, seed=seed)
    img = synth.canny_like_control(B, H, W)
    emb, mask = synth.text_embeddings(B, cfg.gpt.cls_token_num, cfg.gpt.caption_dim)
    return cfg, gold, gsd, img, emb, mask, B, H, W


def test_gpt_b_256_tokens_exact_vs_reference():
    """GPT-B sized model, 256 tokens, cfg 4: exact mode reproduces the reference's greedy tokens bit-for-bit."""
    from controlar_amd import config as C
    from controlar_amd.engine import Engine
    cfg, gold, gsd, img, emb, mask, B, H, W = _golden_big("b_canny_256_cfg4", lambda: C.b_t2i(256, "small", "canny"))
    eng = Engine(cfg, "fp32"); eng.load_state_dict(gsd); eng.finalize()
    eng.encode_control(img.cuda())
    toks, logits = eng.generate(emb.cuda(), 256, mask.cuda(), cfg_scale=float(gold["cfg_scale"]), return_logits=True)
    assert np.array_equal(toks.cpu().numpy(), gold["tokens"])
    steps = gold["logits_steps"]
    np.testing.assert_allclose(logits.cpu().numpy()[:, steps][:, :, ::4], gold["logits"], atol=2e-3, rtol=1e-4)
    eng.close()


def test_gpt_xl_512_full_size_exact_and_fast():
    """BASELINE config at full size (GPT-XL, 512x512, 1024 tokens, B=1): exact mode must match the reference's
    1024 greedy tokens bit-for-bit (min top-2 margin of this golden: 1.2e-3); fast mode is graded teacher-forced."""
    from controlar_amd import config as C
    from controlar_amd.engine import Engine
    cfg, gold, gsd, img, emb, mask, B, H, W = _golden_big("xl_canny_512_cfg1", lambda: C.xl_t2i(1024, "small", "canny"))
    steps = gold["logits_steps"]
    eng = Engine(cfg, "fp32"); eng.load_state_dict(gsd); eng.finalize()
    eng.encode_control(img.cuda())
    toks, logits = eng.generate(emb.cuda(), 1024, mask.cuda(), cfg_scale=1.0, return_logits=True)
    eq = toks.cpu().numpy() == gold["tokens"]
    assert eq.all(), f"first mismatch at {np.argwhere(~eq)[:1].tolist()}, margin there {gold['margin'][~eq][:1]}"
    np.testing.assert_allclose(logits.cpu().numpy()[:, steps][:, :, ::4], gold["logits"], atol=5e-3, rtol=1e-4)
    eng.close()
    eng = Engine(cfg, "bf16"); eng.load_state_dict(gsd); eng.finalize()
    eng.encode_control(img.cuda())
    toks, logits = eng.generate(emb.cuda(), 1024, mask.cuda(), cfg_scale=1.0, forced_tokens=torch.from_numpy(gold["tokens"]), return_logits=True)
    # tolerance at this depth/width = the reference's OWN bf16-vs-fp32 deviation on the same protocol
    # (tests/golden/make_golden.py xl_bf16_calibration: max 1.45, mean 0.24, arg-max agreement 91.6 %), with 1.5x head-room
    import os
    from tests.cases import GOLDEN
    cal = np.load(os.path.join(GOLDEN, "xl_canny_512_cfg1_refbf16.npz"))
    d = np.abs(logits.cpu().numpy()[:, steps][:, :, ::4] - gold["logits"])
    assert d.max() <= 1.5 * float(cal["ref_bf16_max"]) and d.mean() <= 1.5 * float(cal["ref_bf16_mean"]), (d.max(), d.mean())
    agree = toks.cpu().numpy() == gold["tokens"]
    assert agree.mean() >= float(cal["ref_bf16_agree"]) - 0.03, agree.mean()
    assert agree[gold["margin"] > 2.0 * float(cal["ref_bf16_max"])].all()
    eng.close()


# (tests/golden/l_c2i_depth_fixtures_cfg1.npz — GPT-L on the reference's depth fixtures — is pinned on the CPU side by tests/test_oracle_golden.py;
#  it joins this list, with the depth-scaled tolerance used there, once a GPU run of it has been seen)
@pytest.mark.parametrize("name,mk", [("tiny_c2i_cfg1", "tiny"), ("b_c2i_canny_fixtures_cfg1", "b")])
def test_c2i_class_conditional(name, mk):
    """BASELINE config 1 (LlamaGen c2i + ViT-S/16 control, gpt.py): exact mode vs the fp32 oracle bit-for-bit on tokens;
    fast mode teacher-forced vs the reference's bf16 golden (the only precision the reference runs c2i in)."""
    import os
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    from oracle import controlar_oracle as O
    from tests.cases import GOLDEN
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = C.tiny_c2i(64) if mk == "tiny" else C.b_c2i(256)
    B, H, W, seed, _ = [int(x) for x in gold["meta"]]
    gsd, _ = synth.path_state_dicts(cfg, seed=seed)
    x = torch.from_numpy(gold["images_u8"]).float() / 255
    x = (2 * (x - 0.5))[:, None].repeat(1, 3, 1, 1)
    labels = torch.from_numpy(gold["labels"])
    n_new = gold["tokens"].shape[1]
    n_chk = n_new if mk == "tiny" else 48               # CPU oracle budget for the GPT-B case
    toks_o, logits_o = O.generate(gsd, cfg, labels, n_chk, None, cfg_scale=1.0, condition=x, return_logits=True)
    eng = Engine(cfg, "fp32"); eng.load_state_dict(gsd); eng.finalize()
    a = eng.encode_control(x.cuda(), want_output=True).cpu()
    ref_a = O.mlp(O.control_encoder(gsd, cfg, x), gsd["adapter_mlp.fc1.weight"], gsd["adapter_mlp.fc2.weight"])
    np.testing.assert_allclose(a.numpy(), ref_a.numpy(), atol=1e-4, rtol=1e-4)
    toks, logits = eng.generate(labels.cuda(), n_chk, None, cfg_scale=1.0, return_logits=True)
    assert np.array_equal(toks.cpu().numpy(), toks_o.numpy())
    np.testing.assert_allclose(logits.cpu().numpy(), logits_o.numpy(), atol=2e-3, rtol=1e-4)
    eng.close()
    eng = Engine(cfg, "bf16"); eng.load_state_dict(gsd); eng.finalize()
    eng.encode_control(x.cuda())
    toks, logits = eng.generate(labels.cuda(), n_new, None, cfg_scale=1.0, forced_tokens=torch.from_numpy(gold["tokens"]), return_logits=True)
    st = int(gold["logits_step_stride"]); vs = 2 if st == 1 else 4
    d = np.abs(logits.cpu().numpy()[:, ::st, ::vs] - gold["logits"].astype(np.float32))
    assert d.max() < 0.8 and d.mean() < 0.08, (d.max(), d.mean())
    agree = toks.cpu().numpy() == gold["tokens"]
    assert agree[gold["margin"] > 0.5].all() and agree.mean() > 0.9
    eng.close()


def test_c2i_label_errors_without_host_round_trip():
    """car_generate_c2i builds the label -> table-row map on the device (no stream synchronise, SURVEY §8b "no hidden sync"): host labels are range-checked
    for free by the shim; device labels are checked by the kernel — clamped to the null class, reported by the next stats() — and the
    result for VALID labels is unchanged (bit-identical to the host-validated path, including under CFG where the uncond rows take the null class)."""
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    cfg = C.tiny_c2i(64)
    gsd, _ = synth.path_state_dicts(cfg, seed=0)
    B = 3
    x = synth.canny_like_control(B, 128, 128)
    labels = torch.tensor([1, cfg.gpt.num_classes - 1, 0], dtype=torch.int64)
    eng = Engine(cfg, "fp32"); eng.load_state_dict(gsd); eng.finalize()
    eng.encode_control(x.cuda())
    a = eng.generate(labels, 8, None, cfg_scale=1.0).cpu()               # host labels (validated by the shim)
    b = eng.generate(labels.cuda(), 8, None, cfg_scale=1.0).cpu()        # device labels (validated on the device)
    assert torch.equal(a, b)
    eng.stats()                                                          # no flag raised
    with pytest.raises(RuntimeError, match="out of range"):
        eng.generate(torch.tensor([1, cfg.gpt.num_classes + 3, 0]), 8, None)
    bad = torch.tensor([1, cfg.gpt.num_classes + 3, 0], dtype=torch.int64).cuda()
    t = eng.generate(bad, 8, None, cfg_scale=1.0).cpu()                  # enqueued without a host round trip: the error surfaces at the next sync point
    with pytest.raises(RuntimeError, match="class label outside"):
        eng.stats()
    null = eng.generate(torch.tensor([1, cfg.gpt.num_classes, 0]).cuda(), 8, None, cfg_scale=1.0).cpu()
    assert torch.equal(t, null)                                          # the offending row was decoded with the null class
    eng.stats()                                                          # the flag is sticky once, then cleared
    # the flag lives in host-mapped memory: a caller that never asks for stats() still gets the failure — on the generate path itself (the next
    # call on the context after the offending kernel ran) or at once through check_errors()
    eng.generate(bad, 8, None, cfg_scale=1.0).cpu()                      # .cpu() waits for the caller's stream: the label kernel has run
    with pytest.raises(RuntimeError, match="class label outside"):
        eng.generate(labels.cuda(), 8, None, cfg_scale=1.0)
    eng.generate(labels.cuda(), 8, None, cfg_scale=1.0)                  # reported once, cleared
    eng.generate(bad, 8, None, cfg_scale=1.0)
    with pytest.raises(RuntimeError, match="class label outside"):
        eng.check_errors()                                               # waits for the context's stream, then reports
    eng.check_errors()
    eng.close()


@pytest.mark.parametrize("temperature,top_k,top_p", [(1.0, 0, 1.0), (0.7, 20, 1.0), (1.0, 0, 0.8), (1.3, 40, 0.9)])
def test_stochastic_sampler_matches_reference_distribution(temperature, top_k, top_p):
    """sample() with sample_logits=True (generate.py:59-74): RNG streams cannot match torch.multinomial, so parity is
    distributional — the empirical token histogram of 32768 independent draws vs the reference's filtered softmax."""
    from oracle import controlar_oracle as O
    from controlar_amd.engine import Engine
    cs = load_case("tiny_canny_cfg1")
    eng = Engine(cs["cfg"], "bf16")
    V, N = 256, 32768
    g = torch.Generator().manual_seed(3)
    row = torch.randn(V, generator=g) * 2.0
    lg = row[None].repeat(N, 1)
    toks = eng.sample(lg.cuda(), temperature=temperature, top_k=top_k, top_p=top_p, sample_logits=True, seed=42, step=0).cpu().long()
    want = torch.softmax(O.top_k_top_p_filtering(row[None] / max(temperature, 1e-5), top_k, top_p), dim=-1)[0]
    emp = torch.bincount(toks, minlength=V).float() / N
    assert float(emp[want == 0].sum()) == 0.0                   # nothing outside the filtered support
    tv = 0.5 * float((emp - want).abs().sum())
    assert tv < 0.05, tv
    # greedy through the same entry = lowest-index arg-max
    lg2 = torch.randn(64, V, generator=g); lg2[:, 7] = lg2.max() + 1; lg2[:, 3] = lg2[:, 7]
    t = eng.sample(lg2.cuda(), sample_logits=False).cpu()
    assert torch.equal(t.long(), torch.full((64,), 3))
    # CFG layout: rows = [cond | uncond]
    c_, u_ = torch.randn(8, V, generator=g), torch.randn(8, V, generator=g)
    t = eng.sample(torch.cat([c_, u_]).cuda(), cfg_scale=3.0, sample_logits=False).cpu().long()
    assert torch.equal(t, (u_ + (c_ - u_) * 3.0).argmax(-1))
    eng.close()


@pytest.mark.parametrize("chains", [1, 2])
def test_cfg_large_batch_chains_and_row_tiling(chains, monkeypatch):
    """CFG with 2B = 144 rows laid out [cond | uncond]: nine m-blocks (ragged J = 4 tiles) in ONE chain (what 144 rows take by default: the cut into
    two chains starts at 192 sequences), and the same batch forced into TWO chains of [cond 36 | uncond 36] rows — the per-chain row layout, sampler
    offsets and control-token slices of the schedule the 768-image bench runs."""
    monkeypatch.setenv("CAR_CHAINS", str(chains))
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    from oracle import controlar_oracle as O
    cfg = C.tiny_t2i(64, "canny")
    gsd, _ = synth.path_state_dicts(cfg, seed=0)
    B, H, W, n_new = 72, 128, 128, 12
    img = synth.canny_like_control(B, H, W)
    emb, mask = synth.text_embeddings(B, cfg.gpt.cls_token_num, cfg.gpt.caption_dim)
    toks_o, logits_o = O.generate(gsd, cfg, emb, n_new, mask, cfg_scale=2.0, condition=img, return_logits=True)
    eng = Engine(cfg, "bf16", dev=True); eng.load_state_dict(gsd); eng.finalize()      # CAR_CHAINS is a switch of the development build
    eng.encode_control(img.cuda())
    toks, logits = eng.generate(emb.cuda(), n_new, mask.cuda(), cfg_scale=2.0, forced_tokens=toks_o, return_logits=True)
    d = (logits.cpu() - logits_o).abs()
    k = float(np.sqrt(2.0 ** 2 + 1.0 ** 2))
    assert float(d.amax(dim=(1, 2)).max()) <= 0.6 * k and float(d.mean()) <= 0.08 * k, (float(d.max()), float(d.mean()))
    eng.close()


def _quantize_like_library(sd, cfg):
    """Per-output-row e4m3 quantise/dequantise of the five decode linears, as engine_weights.hip: dev_linear does."""
    out = dict(sd)
    names = ["output.weight"]
    for i in range(cfg.gpt.n_layer):
        p = f"layers.{i}."
        names += [p + "attention.wqkv.weight", p + "attention.wo.weight", p + "feed_forward.w1.weight", p + "feed_forward.w3.weight", p + "feed_forward.w2.weight"]
    for n in names:
        w = sd[n].float()
        s = w.abs().amax(dim=1, keepdim=True) / 448.0
        s = torch.where(s > 0, s, torch.ones_like(s))
        out[n] = (w / s).clamp(-448, 448).to(torch.float8_e4m3fn).float() * s
    return out


def test_fp8_weight_decode_config5():
    """BASELINE config 5: fp8 (e4m3, per-row scale) decode weights.  Kernel correctness: against the fp32 oracle run on the
    SAME dequantised weights the fast-mode tolerance must hold; the quantisation error itself (vs the original weights)
    is reported and bounded loosely (the reference has no fp8 path to compare with)."""
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    from oracle import controlar_oracle as O
    cfg = C.tiny_t2i(64, "canny")
    gsd, _ = synth.path_state_dicts(cfg, seed=0)
    B, H, W, n_new = 8, 128, 128, 32
    img = synth.canny_like_control(B, H, W)
    emb, mask = synth.text_embeddings(B, cfg.gpt.cls_token_num, cfg.gpt.caption_dim)
    qsd = _quantize_like_library(gsd, cfg)
    toks_q, logits_q = O.generate(qsd, cfg, emb, n_new, mask, cfg_scale=1.0, condition=img, return_logits=True)
    toks_o, logits_o = O.generate(gsd, cfg, emb, n_new, mask, cfg_scale=1.0, condition=img, forced_tokens=toks_q, return_logits=True)
    eng = Engine(cfg, "bf16", weights_fp8=True); eng.load_state_dict(gsd); eng.finalize()
    eng.encode_control(img.cuda())
    toks, logits = eng.generate(emb.cuda(), n_new, mask.cuda(), cfg_scale=1.0, forced_tokens=toks_q, return_logits=True)
    d = (logits.cpu() - logits_q).abs()
    assert d.max() <= 0.6 and d.mean() <= 0.08, (float(d.max()), float(d.mean()))
    agree = (toks.cpu() == toks_q)
    top2 = logits_q.topk(2, dim=-1).values
    assert bool(agree[(top2[..., 0] - top2[..., 1]) > 0.25].all())
    dq = (logits.cpu() - logits_o).abs()          # total error incl. quantisation
    print(f"fp8 weights: vs dequantised-weight oracle max {float(d.max()):.3f} mean {float(d.mean()):.4f}; "
          f"vs original weights max {float(dq.max()):.3f} mean {float(dq.mean()):.4f}")
    assert dq.mean() <= 0.5
    with pytest.raises(RuntimeError):
        Engine(cfg, "fp32", weights_fp8=True)      # fp8 weights exist only in the fast mode
    eng.close()


def test_fp8_mfma_w8a8_decode():
    """car_config.decode_weight_fp8 = 2: e4m3 weights x e4m3 activations on v_mfma_f32_16x16x32_fp8_fp8 (north_star "MFMA bf16/fp8",
    BASELINE config 5 "fp8 weights on CDNA4 fp8 MFMA").  No reference counterpart: the kernel is graded against the oracle running
    the SAME arithmetic model (dequantised weights, inputs of the five decode linears rounded to e4m3 on single-token steps,
    oracle/controlar_oracle.py GPTState.lin), teacher-forced; the cost of the activation rounding itself is reported vs the
    weight-only model and bounded loosely."""
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    from oracle import controlar_oracle as O
    cfg = C.tiny_t2i(64, "canny")
    gsd, _ = synth.path_state_dicts(cfg, seed=0)
    B, H, W, n_new = 8, 128, 128, 32
    img = synth.canny_like_control(B, H, W)
    emb, mask = synth.text_embeddings(B, cfg.gpt.cls_token_num, cfg.gpt.caption_dim)
    qsd = _quantize_like_library(gsd, cfg)
    toks_q, logits_w = O.generate(qsd, cfg, emb, n_new, mask, cfg_scale=1.0, condition=img, return_logits=True)
    _, logits_a = O.generate(qsd, cfg, emb, n_new, mask, cfg_scale=1.0, condition=img, forced_tokens=toks_q, return_logits=True, act_fp8_decode=True)
    for bsz in (B, 2):       # 8 rows: plain kernels; 2 rows: the fused-norm (NORM) variants
        eng = Engine(cfg, "bf16", weights_fp8="mfma"); eng.load_state_dict(gsd); eng.finalize()
        eng.encode_control(img[:bsz].cuda())
        toks, logits = eng.generate(emb[:bsz].cuda(), n_new, mask[:bsz].cuda(), cfg_scale=1.0, forced_tokens=toks_q[:bsz], return_logits=True)
        d = (logits.cpu() - logits_a[:bsz]).abs()
        dw = (logits.cpu() - logits_w[:bsz]).abs()
        print(f"W8A8 b={bsz}: vs same-model oracle max {float(d.max()):.3f} mean {float(d.mean()):.4f}; vs weight-only model max {float(dw.max()):.3f} mean {float(dw.mean()):.4f}")
        # the e4m3 grid is coarse (3 mantissa bits): a bf16-vs-fp32 difference of the activation before rounding can flip an e4m3
        # code, so the same-model tolerance is wider than the bf16 one
        assert d.mean() <= 0.15 and d.max() <= 1.5, (float(d.max()), float(d.mean()))
        assert dw.mean() <= 0.5
        eng.close()


@pytest.mark.parametrize("name,mk,hw", [("vq_encode_tiny", "tiny", 128), ("vq_encode_vq16_64x64", "vq16", 64)])
def test_vq_encode_tokens(name, mk, hw):
    """VQModel.encode: encoder + quant_conv + quantizer arg-min.  Exact mode reproduces the reference's
    min_encoding_indices bit-for-bit; bf16 mode must agree on the large majority (arg-min over 16384 near-equidistant codes)."""
    import os
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    from tests.cases import GOLDEN
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = C.tiny_t2i(64, "canny")
    if mk == "vq16":
        cfg.vq = C.VQConfig()
    vsd = synth.vq_state_dict(cfg.vq, seed=int(gold["meta"][3]))
    img = synth.smooth_control(2, hw, hw, seed=77) + 0.1 * synth.canny_like_control(2, hw, hw, seed=78)
    for prec in ("fp32", "bf16"):
        eng = Engine(cfg, prec); eng.load_state_dict(vsd, finalize=True)
        toks = eng.vq_encode(img.cuda()).cpu().numpy()
        if prec == "fp32":
            assert np.array_equal(toks, gold["tokens"]), (toks != gold["tokens"]).sum()
            # encode -> decode round trip stays finite and in range
            px = eng.vq_decode(torch.from_numpy(toks), hw // 16, hw // 16)
            assert bool(torch.isfinite(px).all())
        else:
            assert (toks == gold["tokens"]).mean() >= 0.6, (toks == gold["tokens"]).mean()
        eng.close()


@pytest.mark.parametrize("chains", ["2", "3"])
def test_chain_schedule_knobs_do_not_change_tokens(chains, monkeypatch):
    """The decode-loop schedule (phase offset between the chains, several tokens per captured graph with a single-step remainder,
    raised wave priority of the linears) only moves launches around: free-running tokens must equal the lockstep schedule's bit for bit."""
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    cfg = C.tiny_t2i(64, "canny")
    gsd, _ = synth.path_state_dicts(cfg, seed=0)
    B, H, W, n_new = 48, 128, 128, 24                       # 23 decode steps = 4 x 5 + 3
    img = synth.canny_like_control(B, H, W)
    emb, mask = synth.text_embeddings(B, cfg.gpt.cls_token_num, cfg.gpt.caption_dim)
    eng = Engine(cfg, "bf16", dev=True); eng.load_state_dict(gsd); eng.finalize()      # the switches exist only in the development build of the library
    eng.encode_control(img.cuda())
    monkeypatch.setenv("CAR_CHAINS", chains)
    monkeypatch.setenv("CAR_PHASE_OFFSET", "0"); monkeypatch.setenv("CAR_GRAPH_STEPS", "1"); monkeypatch.setenv("CAR_LINEAR_PRIO", "0")
    want = eng.generate(emb.cuda(), n_new, mask.cuda(), cfg_scale=1.0).cpu()
    assert eng.stats()["graph_used"]
    for env in ({"CAR_PHASE_OFFSET": "1"}, {"CAR_PHASE_OFFSET": "1", "CAR_GRAPH_STEPS": "5"}, {"CAR_GRAPH_STEPS": "23"},
                {"CAR_PHASE_OFFSET": "1", "CAR_GRAPH_STEPS": "64", "CAR_LINEAR_PRIO": "1"}):
        for k, v in {"CAR_PHASE_OFFSET": "0", "CAR_GRAPH_STEPS": "1", "CAR_LINEAR_PRIO": "0", **env}.items():
            monkeypatch.setenv(k, v)
        got = eng.generate(emb.cuda(), n_new, mask.cuda(), cfg_scale=1.0).cpu()
        assert eng.stats()["graph_used"], env
        assert torch.equal(got, want), env
        again = eng.generate(emb.cuda(), n_new, mask.cuda(), cfg_scale=1.0).cpu()      # replay of the cached graphs
        assert torch.equal(again, want), env
    eng.close()


@pytest.mark.parametrize("B,cfg_scale", [(1, 4.0), (8, 1.0), (3, 1.0), (64, 1.0), (32, 4.0), (24, 1.0), (48, 1.0)])      # 64 rows: the mid-chain form (helpers ride on the rmsnorm2 launches)
def test_small_chain_runahead_and_attention_do_not_change_a_bit(B, cfg_scale, monkeypatch):
    """Round 6, chains of one m-block (BASELINE configs 2, 4, 5): the L2 run-ahead helper workgroups only READ weights, and the two-blocks-in-flight attention
    (dec_attn2s_kernel) keeps dec_attn2_kernel<16>'s block -> wave assignment and merge order — tokens AND logits must equal the round-5 schedule's bit for bit
    (B = 3 is a grid that is not a multiple of 8: the helpers switch themselves off there)."""
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    cfg = C.tiny_t2i(64, "canny")
    gsd, _ = synth.path_state_dicts(cfg, seed=0)
    H, W, n_new = 128, 128, 40
    img = synth.canny_like_control(B, H, W)
    emb, mask = synth.text_embeddings(B, cfg.gpt.cls_token_num, cfg.gpt.caption_dim)
    eng = Engine(cfg, "bf16", dev=True); eng.load_state_dict(gsd); eng.finalize()
    eng.encode_control(img.cuda())
    monkeypatch.setenv("CAR_NO_RUNAHEAD", "1"); monkeypatch.setenv("CAR_ATTN_OLD_SMALL", "1"); monkeypatch.setenv("CAR_NO_STAGED_NORMX", "1")
    want, want_l = eng.generate(emb.cuda(), n_new, mask.cuda(), cfg_scale=cfg_scale, return_logits=True)
    want, want_l = want.cpu(), want_l.cpu()
    for env in ({"CAR_ATTN_OLD_SMALL": "1"}, {"CAR_NO_RUNAHEAD": "1"}, {"CAR_NO_STAGED_NORMX": "1"}, {}):      # (staged on-the-fly norm, NORM == 3: the NORM == 2 arithmetic with lane-dense operand loads)
        for k in ("CAR_NO_RUNAHEAD", "CAR_ATTN_OLD_SMALL", "CAR_NO_STAGED_NORMX"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got, got_l = eng.generate(emb.cuda(), n_new, mask.cuda(), cfg_scale=cfg_scale, return_logits=True)
        assert eng.stats()["graph_used"], env
        assert torch.equal(got.cpu(), want), env
        assert torch.equal(got_l.cpu(), want_l), env
    eng.close()


def test_switch_changed_between_calls_is_recaptured_not_replayed(monkeypatch):
    """The graph-cache key is the decode plan: a schedule switch flipped between two calls on ONE engine must give a new capture.  The schedule-invariance tests
    above cannot see a stale replay (every schedule computes the same bits); the kernel count of the captured step can: CAR_ATTN_SPLIT_SMALL turns the one-launch
    attention of an 8-row chain into split-KV (nsplit = 16) + combine, one more kernel per layer."""
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    cfg = C.tiny_t2i(64, "canny")
    gsd, _ = synth.path_state_dicts(cfg, seed=0)
    B, H, W, n_new = 8, 128, 128, 8
    img = synth.canny_like_control(B, H, W)
    emb, mask = synth.text_embeddings(B, cfg.gpt.cls_token_num, cfg.gpt.caption_dim)
    eng = Engine(cfg, "bf16", dev=True); eng.load_state_dict(gsd); eng.finalize()
    eng.encode_control(img.cuda())
    monkeypatch.delenv("CAR_ATTN_SPLIT_SMALL", raising=False)
    want = eng.generate(emb.cuda(), n_new, mask.cuda(), cfg_scale=1.0).cpu()
    st = eng.stats(); k0 = st["decode_kernels_per_step"]
    assert st["graph_used"]
    monkeypatch.setenv("CAR_ATTN_SPLIT_SMALL", "1")
    eng.generate(emb.cuda(), n_new, mask.cuda(), cfg_scale=1.0)
    st = eng.stats()
    assert st["graph_used"] and st["decode_kernels_per_step"] == k0 + cfg.gpt.n_layer, (k0, st)
    monkeypatch.delenv("CAR_ATTN_SPLIT_SMALL")
    got = eng.generate(emb.cuda(), n_new, mask.cuda(), cfg_scale=1.0).cpu()
    st = eng.stats()
    assert st["graph_used"] and st["decode_kernels_per_step"] == k0, (k0, st)
    assert torch.equal(got, want)
    eng.close()


def test_two_chains_free_running_twins_agree_at_model_b():
    """Two decode chains as parallel graph branches, FREE-RUNNING (what bench.py's twin check asserts at XL): identical inputs in row 0 (chain 0) and row B/2
    (chain 1) must give identical tokens and logits on every call.  Round 6 found the teacher-forced comparison blind to a stale step position: a dec_gemm that
    took *pos from a register loaded at kernel entry instead of a fresh load in its epilogue made the chain on the second graph branch drift (lane-level faults
    in q / K units; the position VALUE was never stale: profiles/r06_posdbg_*.txt), and only the fed-back tokens showed it."""
    from controlar_amd import config as C, synth
    from controlar_amd.engine import Engine
    cfg = C.b_t2i(256, adapter_size="small", condition_type="canny")
    gsd, _ = synth.path_state_dicts(cfg, seed=0)
    B, n_new = 384, 96
    img = synth.canny_like_control(B, 256, 256); emb, mask = synth.text_embeddings(B, cfg.gpt.cls_token_num, cfg.gpt.caption_dim)
    t = B // 2
    img[t], emb[t], mask[t] = img[0], emb[0], mask[0]
    eng = Engine(cfg, "bf16"); eng.load_state_dict(gsd); eng.finalize()
    eng.encode_control(img.cuda())
    for it in range(3):
        toks, logits = eng.generate(emb.cuda(), n_new, mask.cuda(), cfg_scale=1.0, return_logits=True)
        assert eng.stats()["graph_used"]
        assert torch.equal(toks[0], toks[t]), (it, int((toks[0] != toks[t]).nonzero()[0]))
        assert torch.equal(logits[0], logits[t]), it
    eng.close()
