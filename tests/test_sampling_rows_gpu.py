"""GPU (pytest -m gpu): per-request sampling parameters inside one batch — car_generate_rows, car_generate_c2i_rows, car_score_rows,
car_sample_logits_rows behind Engine.generate / score / sample.

Contract: every image of a batch carries its own car_sampling_row and its own RNG stream, and its result is a function of that row alone.  The fp32
mode is batch-invariant by construction, so there the property is checked bit for bit against the plain (uniform) call on the image alone; in bf16 the
batch size is kept equal on both sides, so that the tile choice cannot differ.  The only check that does not lean on the uniform path is the
distributional one, which uses the oracle's filter with the project's existing N = 32768 and total-variation bound 0.05."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.cases import load_case

pytestmark = pytest.mark.gpu

N_NEW = 64


def _engine(cs, prec, dev=None):
    from controlar_amd.engine import Engine
    eng = Engine(cs["cfg"], prec, dev=dev)
    eng.load_state_dict(cs["gsd"]); eng.finalize()
    return eng


def _inputs(cs, B):
    """B images of the tiny_depth_cfg4 family with distinct controls, prompts and masks (images 0 and 1 are the case's own)."""
    from controlar_amd import synth
    g = cs["cfg"].gpt
    img = synth.smooth_control(B, cs["H"], cs["W"])
    emb, mask = synth.text_embeddings(B, g.cls_token_num, g.caption_dim)
    return img, emb, mask


def _gen(eng, img, emb, mask, sel, **kw):
    """encode_control + generate on the images `sel` (an index list or a slice); returns (tokens, logits) on the host."""
    eng.encode_control(img[sel].cuda())
    t, l = eng.generate(emb[sel].cuda(), N_NEW, mask[sel].cuda(), return_logits=True, **kw)
    return t.cpu(), l.cpu()


# ------------------------------------------------------------------------------------------------ the sampler alone
def _six_rows(V):
    return dict(sample_logits=[False, True, True, True, True, True], temperature=[1.0, 0.7, 1.0, 1.3, 1.0, 1e-6], top_k=[0, 20, 0, 40, V, 0],
                top_p=[1.0, 1.0, 0.8, 0.9, 1.0, 1.0], seed=[11, 12, 13, 14, 15, 16])


def _row(params, i):
    return {k: (v[i] if isinstance(v, list) else v) for k, v in params.items()}


@pytest.fixture(scope="module")
def sampler_engine():
    from controlar_amd.engine import Engine
    eng = Engine(load_case("tiny_canny_cfg1")["cfg"], "bf16")
    yield eng
    eng.close()


@pytest.mark.parametrize("V", [256, 16384])
def test_sampler_rows_equal_the_uniform_call_on_each_row(sampler_engine, V):
    """Six parameter sets in ONE launch — greedy, top-k alone (radix select), top-p (sort), all three, k = V, T = 1e-6 — each with its own seed: every
    row's token is the token of the uniform call on that row alone (there the row is image 0: rng_stream 0, the row call's default)."""
    eng = sampler_engine
    g = torch.Generator().manual_seed(100 + V)
    lg = (torch.randn(6, V, generator=g) * 2.0).cuda()
    params = _six_rows(V)
    for step in (0, 7):
        got = eng.sample(lg, step=step, **params).cpu()
        for i in range(6):
            want = eng.sample(lg[i:i + 1], step=step, **_row(params, i)).cpu()
            assert int(got[i]) == int(want[0]), (V, step, i)
    assert int(got[0]) == int(lg[0].argmax())                                                        # the greedy row, inside the stochastic launch
    assert int(got[5]) == int(lg[5].argmax())                                                        # T = 1e-6 is greedy in effect
    # no stochastic row: the greedy kernel alone
    got = eng.sample(lg, sample_logits=[False] * 6, seed=[1, 2, 3, 4, 5, 6]).cpu().long()
    assert torch.equal(got, lg.argmax(-1).cpu())


@pytest.mark.parametrize("V", [256, 16384])
def test_sampler_rows_under_cfg_with_per_row_scale_and_interval(sampler_engine, V):
    """The CFG layout [cond | uncond] with a scale and an interval per row, at a step on each side of every finite interval."""
    eng = sampler_engine
    g = torch.Generator().manual_seed(200 + V)
    c_, u_ = torch.randn(6, V, generator=g) * 2.0, torch.randn(6, V, generator=g) * 2.0
    lg = torch.cat([c_, u_]).cuda()
    params = dict(_six_rows(V), cfg_scale=[1.5, 3.0, 7.5, 3.0, 1.5, 7.5], cfg_interval=[5, 8, -1, 5, 8, 5])
    for step in (3, 12):                                                                             # step - 1 = 2 <= 5: mixed; step - 1 = 11 > 8: the conditional row alone
        got = eng.sample(lg, step=step, **params).cpu()
        for i in range(6):
            want = eng.sample(torch.cat([lg[i:i + 1], lg[6 + i:7 + i]]), step=step, **_row(params, i)).cpu()
            assert int(got[i]) == int(want[0]), (V, step, i)
        mixed = u_[0] + (c_[0] - u_[0]) * 1.5
        assert int(got[0]) == int((mixed if step == 3 else c_[0]).argmax())                          # the greedy row: the interval is honoured per row
        assert int(got[5]) == int((u_[5] + (c_[5] - u_[5]) * 7.5 if step == 3 else c_[5]).argmax())


def test_sampler_rows_match_the_reference_distribution():
    """Independent of the uniform path: 4 parameter groups x 32768 rows interleaved in one call, every row on its own rng_stream, against the oracle's
    filtered softmax — the logits row, N and bound of test_stochastic_sampler_matches_reference_distribution."""
    from oracle import controlar_oracle as O
    from controlar_amd.engine import Engine
    groups = [(1.0, 0, 1.0), (0.7, 20, 1.0), (1.0, 0, 0.8), (1.3, 40, 0.9)]
    eng = Engine(load_case("tiny_canny_cfg1")["cfg"], "bf16")
    V, N, G = 256, 32768, len(groups)
    g = torch.Generator().manual_seed(3)
    row = torch.randn(V, generator=g) * 2.0
    lg = row[None].repeat(N * G, 1).cuda()
    idx = list(range(N * G))
    toks = eng.sample(lg, temperature=[groups[r % G][0] for r in idx], top_k=[groups[r % G][1] for r in idx], top_p=[groups[r % G][2] for r in idx],
                      sample_logits=True, seed=42, step=0, rng_stream=idx).cpu().long()
    for k, (temperature, top_k, top_p) in enumerate(groups):
        want = torch.softmax(O.top_k_top_p_filtering(row[None] / max(temperature, 1e-5), top_k, top_p), dim=-1)[0]
        emp = torch.bincount(toks[k::G], minlength=V).float() / N
        tv = 0.5 * float((emp - want).abs().sum())
        print(f"group {k} (T={temperature}, k={top_k}, p={top_p}): total variation {tv:.4f}, mass outside the support {float(emp[want == 0].sum())}")
        assert float(emp[want == 0].sum()) == 0.0, k                                                  # nothing outside the filtered support
        assert tv < 0.05, (k, tv)
    eng.close()


# ------------------------------------------------------------------------------------------------ generate: broadcast identity
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_broadcast_rows_reproduce_the_uniform_call(prec):
    """A row table that repeats the uniform parameters with rng_stream[i] = i (the counter the plain call uses) returns the plain call's tokens and
    logits_out.  Other seeds replay the captured graph and change the tokens; the plain call afterwards is unchanged.  The strength is the case's 0.6 in
    bf16, where both paths round the product explicitly; in fp32 it is 0.5: the plain fp32 kernels may contract v + cs * c into one FMA, the row path
    rounds the product first, and the two agree exactly for powers of two."""
    cs = load_case("tiny_depth_cfg4")
    eng = _engine(cs, prec)
    B = cs["B"]
    img, emb, mask = _inputs(cs, B)
    kw = dict(cfg_scale=cs["cfg_scale"], control_strength=cs["control_strength"] if prec == "bf16" else 0.5, temperature=1.0, top_k=20, top_p=1.0,
              sample_logits=True)
    sel = slice(0, B)
    t0, l0 = _gen(eng, img, emb, mask, sel, seed=5, **kw)
    t1, l1 = _gen(eng, img, emb, mask, sel, seed=5, rng_stream=list(range(B)), **kw)
    assert torch.equal(t1, t0) and torch.equal(l1, l0)
    t2, l2 = _gen(eng, img, emb, mask, sel, seed=[5] * B, cfg_scale=[kw["cfg_scale"]] * B, rng_stream=list(range(B)), **{k: v for k, v in kw.items() if k != "cfg_scale"})
    assert torch.equal(t2, t0) and torch.equal(l2, l0)
    t3, _ = _gen(eng, img, emb, mask, sel, seed=[77, 78], rng_stream=list(range(B)), **kw)
    assert eng.stats()["graph_used"]
    assert not torch.equal(t3, t0)
    t4, l4 = _gen(eng, img, emb, mask, sel, seed=5, **kw)
    assert torch.equal(t4, t0) and torch.equal(l4, l0)
    eng.close()


# ------------------------------------------------------------------------------------------------ generate: request independence (fp32)
SIX = dict(cfg_scale=[4.0, 1.5, 3.0, 7.5, 2.0, 4.0], cfg_interval=[-1, 20, 5, -1, 40, 10], temperature=[1.0, 0.7, 1.0, 1.3, 1.0, 0.9],
           top_k=[0, 20, 0, 40, 0, 100], top_p=[1.0, 1.0, 0.8, 0.9, 1.0, 1.0], sample_logits=[False, True, True, True, False, True],
           seed=[11, 12, 13, 14, 15, 16], control_strength=[1.0, 0.5, 0.25, 2.0, 0.5, 1.0])


@pytest.fixture(scope="module")
def six():
    """The fp32 references, computed once: each of six requests decoded ALONE by the plain call (B = 1) with its own parameters, and the six decoded
    together by the row call.  The development build of the library, so that one test can force two chains."""
    cs = load_case("tiny_depth_cfg4")
    eng = _engine(cs, "fp32", dev=True)
    img, emb, mask = _inputs(cs, 6)
    alone = [_gen(eng, img, emb, mask, [i], **_row(SIX, i)) for i in range(6)]
    full = _gen(eng, img, emb, mask, slice(0, 6), **SIX)
    yield dict(eng=eng, img=img, emb=emb, mask=mask, alone=alone, full=full)
    eng.close()


def test_each_request_equals_its_own_uniform_call(six):
    """Own (cfg_scale > 1, cfg_interval, temperature, top_k, top_p, greedy flag, seed, control_strength in {1, 0.5, 0.25, 2}) per row: tokens AND logits of
    row i are those of the B = 1 plain call with row i's parameters."""
    t, l = six["full"]
    for i, (ta, la) in enumerate(six["alone"]):
        assert torch.equal(t[i], ta[0]), i
        assert torch.equal(l[i], la[0]), i
    assert len({tuple(r.tolist()) for r in t}) == 6                                                   # six different requests, six different images


def test_a_permutation_of_the_requests_permutes_the_outputs(six):
    perm = [3, 0, 5, 1, 4, 2]
    t, l = _gen(six["eng"], six["img"], six["emb"], six["mask"], perm, **{k: [v[p] for p in perm] for k, v in SIX.items()})
    assert torch.equal(t, six["full"][0][perm]) and torch.equal(l, six["full"][1][perm])


def test_shard_rows_over_two_ranks_reproduces_the_unsharded_tokens(six):
    """dist.shard_rows over world 2, the two ranks run one after the other on the one GPU: a rank's parameters travel with its images."""
    from controlar_amd import dist
    for rank in range(2):
        sl = dist.shard_slice(6, 2, rank)
        t, l = _gen(six["eng"], six["img"], six["emb"], six["mask"], sl, **dist.shard_rows(SIX, 6, 2, rank))
        assert torch.equal(t, six["full"][0][sl]) and torch.equal(l, six["full"][1][sl]), rank


def test_two_chains_take_their_slice_of_the_table(six, monkeypatch):
    """CAR_CHAINS=2 (development build): chain 1's sampler reads rows 3..5 of the table — the same tokens and logits as one chain."""
    monkeypatch.setenv("CAR_CHAINS", "2")
    t, l = _gen(six["eng"], six["img"], six["emb"], six["mask"], slice(0, 6), **SIX)
    assert six["eng"].stats()["graph_used"]
    assert torch.equal(t, six["full"][0]) and torch.equal(l, six["full"][1])


# ------------------------------------------------------------------------------------------------ generate: strength per row in bf16
def test_bf16_strength_per_row_equals_the_uniform_call_at_that_strength():
    """One arbitrary strength per row, everything else uniform and greedy, teacher-forced so that rows cannot drift; the batch size is the same on both
    sides.  Scaling the control tokens once (c' = bf16(cs_i * c), then bf16(h + bf16(1 * c'))) is bit-equal to scaling on the fly, because both round
    the product to bf16 explicitly: logits_out of row i equals row i of the plain call run at cs_i."""
    cs = load_case("tiny_depth_cfg4")
    eng = _engine(cs, "bf16")
    strengths = [0.6, 0.35, 1.0, 0.85]
    B = len(strengths)
    img, emb, mask = _inputs(cs, B)
    forced = torch.from_numpy(np.concatenate([cs["gold"]["tokens"], cs["gold"]["tokens"][::-1, ::-1]])).to(torch.int32).contiguous()
    assert forced.shape == (B, N_NEW)
    kw = dict(cfg_scale=cs["cfg_scale"], forced_tokens=forced)
    _, lr = _gen(eng, img, emb, mask, slice(0, B), control_strength=strengths, **kw)
    seen = []
    for i, s in enumerate(strengths):
        _, lu = _gen(eng, img, emb, mask, slice(0, B), control_strength=s, **kw)
        assert torch.equal(lr[i], lu[i]), (i, s)
        seen.append(lu[0])
    assert not torch.equal(seen[0], seen[2])                                                          # the strength reaches the logits at all
    eng.close()


# ------------------------------------------------------------------------------------------------ c2i
def _c2i_case():
    import os
    from controlar_amd import config as Cfg, synth
    from tests.cases import GOLDEN
    gold = np.load(os.path.join(GOLDEN, "tiny_c2i_cfg1.npz"))
    cfg = Cfg.tiny_c2i(64)
    gsd, _ = synth.path_state_dicts(cfg, seed=int(gold["meta"][3]))
    x = torch.from_numpy(gold["images_u8"]).float() / 255
    x = (2 * (x - 0.5))[:, None].repeat(1, 3, 1, 1)
    return cfg, gsd, x, torch.from_numpy(gold["labels"])


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_c2i_rows(prec):
    """car_generate_c2i_rows on tiny_c2i_cfg1: the broadcast identity in both modes; per-row temperature, seed and greedy flag against the B = 1 plain
    call in fp32."""
    from controlar_amd.engine import Engine
    cfg, gsd, x, labels = _c2i_case()
    eng = Engine(cfg, prec); eng.load_state_dict(gsd); eng.finalize()
    B = labels.shape[0]

    def run(sel, **kw):
        eng.encode_control(x[sel].cuda())
        t, l = eng.generate(labels[sel].cuda(), N_NEW, None, cfg_scale=1.0, return_logits=True, **kw)
        return t.cpu(), l.cpu()
    kw = dict(temperature=0.9, top_k=20, sample_logits=True)
    t0, l0 = run(slice(0, B), seed=5, **kw)
    t1, l1 = run(slice(0, B), seed=[5] * B, rng_stream=list(range(B)), **kw)
    assert torch.equal(t1, t0) and torch.equal(l1, l0)
    t2, _ = run(slice(0, B), seed=[8, 9], rng_stream=list(range(B)), **kw)
    assert eng.stats()["graph_used"] and not torch.equal(t2, t0)
    if prec == "fp32":
        rows = dict(temperature=[0.8, 1.2], seed=[3, 4], sample_logits=[True, False], top_k=[20, 0])
        t, l = run(slice(0, B), **rows)
        for i in range(B):
            ta, la = run([i], **_row(rows, i))
            assert torch.equal(t[i], ta[0]) and torch.equal(l[i], la[0]), i
    eng.close()


# ------------------------------------------------------------------------------------------------ score
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_score_rows_equal_the_single_image_uniform_score(prec):
    """Per-row cfg_scale, cfg_interval and power-of-two strengths: row i of the row call is the single-image plain car_score bit for bit, nll and logits
    (car_score is chunk- and batch-invariant in both modes)."""
    cs = load_case("tiny_depth_cfg4")
    eng = _engine(cs, prec)
    B = 3
    img, emb, mask = _inputs(cs, B)
    g = torch.Generator().manual_seed(9)
    tokens = torch.randint(0, cs["cfg"].gpt.vocab_size, (B, N_NEW), generator=g, dtype=torch.int32)
    rows = dict(cfg_scale=[1.5, 3.0, 7.5], cfg_interval=[-1, 10, 30], control_strength=[0.5, 2.0, 0.25])
    eng.encode_control(img.cuda())
    nll, lg = eng.score(emb.cuda(), tokens.cuda(), mask.cuda(), return_logits=True, **rows)
    nll, lg = nll.cpu(), lg.cpu()
    for i in range(B):
        eng.encode_control(img[i:i + 1].cuda())
        n1, l1 = eng.score(emb[i:i + 1].cuda(), tokens[i:i + 1].cuda(), mask[i:i + 1].cuda(), return_logits=True, **_row(rows, i))
        assert torch.equal(nll[i], n1.cpu()[0]), (prec, i)
        assert torch.equal(lg[i], l1.cpu()[0]), (prec, i)
    # the interval is honoured per row: without it row 1 changes from position cfg_interval + 2 = 12 on and nowhere else; row 0 (interval -1) not at all
    eng.encode_control(img.cuda())
    _, l2 = eng.score(emb.cuda(), tokens.cuda(), mask.cuda(), return_logits=True, **dict(rows, cfg_interval=[-1, -1, -1]))
    l2 = l2.cpu()
    assert torch.equal(l2[0], lg[0]) and torch.equal(l2[1, :12], lg[1, :12])
    assert all(not torch.equal(l2[1, j], lg[1, j]) for j in range(12, N_NEW))
    eng.close()


# ------------------------------------------------------------------------------------------------ errors
def test_bad_rows_fail_the_call_and_leave_the_context_usable():
    from controlar_amd import _lib as L
    cs = load_case("tiny_depth_cfg4")
    eng = _engine(cs, "bf16")
    B = cs["B"]
    img, emb, mask = _inputs(cs, B)
    kw = dict(cfg_scale=cs["cfg_scale"], control_strength=cs["control_strength"])
    want, _ = _gen(eng, img, emb, mask, slice(0, B), rng_stream=0, **kw)
    # top_p = 0 through the public interface
    with pytest.raises(RuntimeError, match=r"car_generate_rows: row 1: top_p must be in \(0, 1\]"):
        _gen(eng, img, emb, mask, slice(0, B), top_p=[1.0, 0.0], **kw)
    with pytest.raises(RuntimeError, match="top_k must be >= 0"):
        _gen(eng, img, emb, mask, slice(0, B), top_k=[0, -3], **kw)
    with pytest.raises(RuntimeError, match="top_p"):
        eng.sample(torch.zeros(2, 256), top_p=[0.0, 1.0])
    # mixed CFG rows: Engine refuses them before the library is entered ...
    with pytest.raises(ValueError, match="call-wide"):
        _gen(eng, img, emb, mask, slice(0, B), cfg_scale=[4.0, 1.0])
    # ... and the library refuses them itself when a caller of the C ABI hands them over
    rows = (L.CarSamplingRow * B)()
    for i, r in enumerate(rows):
        r.cfg_scale, r.cfg_interval, r.temperature, r.top_k, r.top_p, r.control_strength = (4.0 if i == 0 else 1.0), -1, 1.0, 0, 1.0, 1.0
    sp = L.CarSampling()
    e, m = emb.cuda().contiguous(), mask.cuda().contiguous()
    out = torch.empty(B, N_NEW, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(int(torch.cuda.current_stream().cuda_stream))
    rc = eng.lib.car_generate_rows(eng._h, C.c_void_p(e.data_ptr()), L.CAR_DT_F32, C.c_void_p(m.data_ptr()), B, N_NEW, 1, C.byref(sp), rows,
                                   C.c_void_p(out.data_ptr()), None, None, stream)
    msg = eng.lib.car_last_error(eng._h).decode()
    assert rc != 0 and "call-wide" in msg and "cfg_scale" in msg, msg
    lg = torch.zeros(2 * B, 256, device="cuda")
    rc = eng.lib.car_sample_logits_rows(eng._h, C.c_void_p(lg.data_ptr()), B, 256, C.byref(sp), rows, 0, C.c_void_p(out.data_ptr()), stream)
    assert rc != 0 and "call-wide" in eng.lib.car_last_error(eng._h).decode()
    eng.encode_control(img.cuda())
    nll_rc = eng.lib.car_score_rows(eng._h, C.c_void_p(e.data_ptr()), L.CAR_DT_F32, C.c_void_p(m.data_ptr()), B, N_NEW, 1, C.byref(sp), rows,
                                    C.c_void_p(out.data_ptr()), C.c_void_p(lg.data_ptr()), None, stream)
    assert nll_rc != 0 and "call-wide" in eng.lib.car_last_error(eng._h).decode()
    # the context stays usable
    got, _ = _gen(eng, img, emb, mask, slice(0, B), rng_stream=0, **kw)
    assert torch.equal(got, want)
    eng.close()
