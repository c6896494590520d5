// engine_prompt.hip — the prompt pass that car_generate's prefill and car_score share: the prefill window, stage C (control tokens), stage D (text prefix)
// and stage E (the layers over the prompt rows, then the final norm).  Each caller keeps its argument checks, its row layout and what follows the pass.
// (one of the translation units behind include/controlar_hip.h; shared declarations: engine_internal.h)
#include "engine_internal.h"

// ------------------------------------------------------------------------------------- the prefill window
// (round 4; SURVEY Appendix E: result-preserving).  Prompts are LEFT-padded (sample_t2i.py:146-160): a pad column is masked for every row of the prompt
// pass and for every decode step, so the hidden states and K / V of pad rows influence nothing that is returned — yet the reference (and rounds 1-3 here)
// pushed all T = 120 rows of every sequence through the 36 layers.  The pass runs on the LAST Tv rows only, Tv = the longest valid prompt of the batch
// rounded up (8-40 of 120 in the reference's caption statistics): every kernel of the pass sees sequences of Tv rows, cache rows and rope rows are offset
// by t0 = T - Tv, the mask by the same columns.  A valid row's arithmetic is unchanged (masked keys contributed exact zeros), so exact-mode tokens stay
// bit-identical.
//
// The rule: t0 is the largest multiple of `grain` that is <= min(clamp(first_valid, 0, T), T - 8), and there is no window (t0 = 0, Tv = T) unless T > 8 and
// T % 8 == 0.  The grain is the caller's:
//   16 (car_generate): a key keeps its slot inside the 16-wide k-blocks of the P·V product (one MFMA chain over the k-blocks in order: leading all-zero
//      blocks add exact zeros), and the row softmax sums a column in the lane of its ABSOLUTE position (softmax_wave_kernel) — so a valid row's K / V rows
//      and logits are the same bits whatever the batch-mates' prompt lengths make of t0 (tests/test_parity_gpu.py::test_exact_mode_prefill_window_invariance).
//   32 (car_score): the key block of flash64, a multiple of the 16 above — a sequence scored alone returns the bits of its slice of any batch and of any
//      chunk, in both modes (the chunk rule at the top of engine_score.hip).
// Whether there is a window at all (a mask, the mode, the model type, the development switch) is the caller's decision.
static void prompt_window_rule(int T, int first_valid, int grain, int* t0, int* Tv) {
    *t0 = 0; *Tv = T;
    if (!prompt_has_window(T)) return;
    const int fv = first_valid < 0 ? 0 : (first_valid > T ? T : first_valid);
    *t0 = std::min(fv, T - 8) / grain * grain;
    *Tv = T - *t0;
    if (*Tv % 8) { *Tv = T; *t0 = 0; }
}

// host-only view of the rule (tests/test_modes_cpu.py)
extern "C" int car_debug_prompt_window(int32_t T, int32_t first_valid, int32_t grain, int32_t* t0, int32_t* Tv) {
    if (!t0 || !Tv || T <= 0 || grain <= 0 || grain % 8) return -1;
    int a, b; prompt_window_rule(T, first_valid, grain, &a, &b);
    *t0 = a; *Tv = b;
    return 0;
}

// The window size has to be known on the HOST before the pass is enqueued.  With the caller's car_sampling.first_valid_hint (`hint` = the bound + 1; 0: none)
// nothing is read back and the call only enqueues: the device checks the bound against the batch minimum of jmin[n] (the first valid column of every row)
// and raises the sticky flag host_flags[1] if valid rows would fall outside the window.  Without a hint: ONE 4-byte device-to-host read of that minimum — the
// only host wait of car_generate / car_score, and only when a mask is given (it also waits for whatever the caller had queued before).
int prompt_window(car_ctx* c, int hint, const int* jmin, int n, int* jmin_min, int T, int grain, int* t0, int* Tv, hipStream_t st) {
    int hmin = hint - 1;
    if (hint <= 0) {
        car_launch_min_int(jmin, n, jmin_min, -1, nullptr, st);
        HIPCHK(c, hipMemcpyAsync(&hmin, jmin_min, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    prompt_window_rule(T, hmin, grain, t0, Tv);
    if (hint > 0 && *t0 > 0) {
        if (ensure_host_flags(c)) return -1;
        car_launch_min_int(jmin, n, jmin_min, *t0, c->host_flags + 1, st);
    }
    return 0;
}

// ------------------------------------------------------------------------------------- C. control tokens
// condition_mlp over all images, then the 3 condition_layers (gpt_t2i.py:437-442) per row group, cached in c->ctrl[0..2] for the whole call.  Group g =
// images [img0[g], img0[g+1]), its rows [cond | uncond] under CFG.  `strength_rows` (row mode, some row's strength is not 1; else NULL): the device row table
// in image order — image i's conditional tokens become c' = rnd(cs_i * c) once, here; every later add is rnd(1 * c') == c' (the unconditional half stays
// exact zeros).  The MLPs' hidden activations sit in ws[WS_ATTN_S], idle until the pass's attention: the caller sizes it for both uses.
int prompt_control_tokens(car_ctx* c, const int* img0, int n_groups, bool use_cfg, const SampleRow* strength_rows, hipStream_t st) {
    const int D = c->cfg.dim, n_tok = c->ctrl_ntok, mult = use_cfg ? 2 : 1; const size_t e = c->esz;
    void* ce = c->ws[WS_CTRL_MLP].p; void* scratch = c->ws[WS_ATTN_S].p;
    mlp_tanh(c, c->ctrl_in.p, D, 0, 1, img0[n_groups] * n_tok, D, "condition_mlp.cap_proj.", scratch, ce, D, st);
    for (int k = 0; k < 3; ++k) for (int gi = 0; gi < n_groups; ++gi) {
        const int ng = img0[gi + 1] - img0[gi]; const size_t rows = (size_t)ng * n_tok, base = (size_t)mult * img0[gi] * n_tok;
        mlp_tanh(c, off(ce, (size_t)img0[gi] * n_tok * D, e), D, 0, 1, (int)rows, D, "condition_layers." + std::to_string(k) + ".", scratch, off(c->ctrl[k].p, base * D, e), D, st);
        if (use_cfg) HIPCHK(c, hipMemsetAsync(off(c->ctrl[k].p, (base + rows) * D, e), 0, rows * D * e, st));   // uncond rows: MLP(0) = 0 exactly
        if (strength_rows) car_launch_ctrl_scale_rows(c->mode, off(c->ctrl[k].p, base * D, e), strength_rows + img0[gi], ng, (long)n_tok * D, st);
    }
    return 0;
}

// ------------------------------------------------------------------------------------- D. text prefix
// cls_embedding.cap_proj (gpt_t2i.py:435) over the window [t0, t0 + Tv) of the captions of the groups' images; uncond rows = uncond_embedding
// (generate.py:157).  The groups' rows land densely in `out`, [cond | uncond] per group: mult * (img0[n_groups] - img0[0]) sequences of Tv rows.
void prompt_text(car_ctx* c, const void* text_emb, int text_dtype, const int* img0, int n_groups, bool use_cfg, int t0, int Tv, void* out, hipStream_t st) {
    const car_config& g = c->cfg; const int mult = use_cfg ? 2 : 1;
    const long per_src = (long)g.cls_token_num * g.caption_dim, per = (long)Tv * g.caption_dim; const size_t ib = text_dtype == CAR_DT_BF16 ? 2 : 4;
    void* text = c->ws[WS_TEXT].p;
    for (int gi = 0; gi < n_groups; ++gi)
        car_launch_build_text(c->mode, (const char*)text_emb + (size_t)img0[gi] * per_src * ib, text_dtype, Wp(c, "cls_embedding.uncond_embedding"),
                              off(text, (size_t)mult * (img0[gi] - img0[0]) * per, c->esz), img0[gi + 1] - img0[gi], per, per_src, (long)t0 * g.caption_dim, use_cfg, st);
    mlp_tanh(c, text, g.caption_dim, 0, 1, mult * (img0[n_groups] - img0[0]) * Tv, g.caption_dim, "cls_embedding.cap_proj.", c->ws[WS_XN].p, out, g.dim, st);
}

// ------------------------------------------------------------------------------------- E. the layers
// h += wo(att); xn = ffn_norm(h); h += w2(silu(w1 xn) * w3 xn) over `rows` rows of layer prefix L (gpt_t2i.py:291-295).  mid holds rows * ffn_hidden
// elements, in the fp32 mode three times that: the interleaved w13 output sits behind the gated product.
static void gpt_layer_tail(car_ctx* c, const std::string& L, void* h, void* xn, const void* att, void* mid, long rows, hipStream_t st) {
    const car_config& g = c->cfg; const int mode = c->mode, D = g.dim, Fh = g.ffn_hidden;
    { GemmP q = gp(att, D, Wp(c, L + "attention.wo.weight"), D, h, D, (int)rows, D, D); q.R = h; q.ldr = D; car_launch_gemm(mode, AMODE_PLAIN, &q, st); }
    { NormP np; memset(&np, 0, sizeof(np)); np.h_in = h; np.xn = xn; np.w = Wp(c, L + "ffn_norm.weight"); np.D = D; np.eps = g.norm_eps; car_launch_rmsnorm(mode, &np, rows, st); }
    if (mode == CAR_BF16) {
        GemmP q = gp(xn, D, Wp(c, L + "feed_forward.w13.weight"), D, mid, Fh, (int)rows, 2 * Fh, D); q.swiglu = 1; car_launch_gemm(mode, AMODE_PLAIN, &q, st);
    } else {
        void* mid2 = off(mid, (size_t)rows * Fh, c->esz);
        GemmP q = gp(xn, D, Wp(c, L + "feed_forward.w13.weight"), D, mid2, 2 * Fh, (int)rows, 2 * Fh, D); car_launch_gemm(mode, AMODE_PLAIN, &q, st);
        car_launch_swiglu(mode, mid2, mid, rows, Fh, st);
    }
    { GemmP q = gp(mid, Fh, Wp(c, L + "feed_forward.w2.weight"), Fh, h, D, (int)rows, D, Fh); q.R = h; q.ldr = D; car_launch_gemm(mode, AMODE_PLAIN, &q, st); }
}

// Per layer (gpt_t2i.py:446-470): rmsnorm (+ the control add at layers 0, n/3, 2n/3) -> wqkv -> the caller's rope step -> attn_run (causal + pad mask;
// q | k | v packed in the wqkv output) -> gpt_layer_tail; then the final norm of all rows into p.xn.  Non-zero: the fused attention kernel refused the shape
// and nothing further was launched — the caller fails the call in its own words.
int prompt_layers(car_ctx* c, const PromptPass& p, hipStream_t st) {
    const car_config& g = c->cfg; const int mode = c->mode, D = g.dim, li = g.n_layer / 3; const size_t e = c->esz;
    const long rows = (long)p.nseq * p.Tn;
    for (int l = 0; l < g.n_layer; ++l) {
        const std::string L = "layers." + std::to_string(l) + ".";
        {
            NormP np; memset(&np, 0, sizeof(np));
            np.h_in = p.h; np.h_out = p.h; np.xn = p.xn; np.w = Wp(c, L + "attention_norm.weight"); np.D = D; np.eps = g.norm_eps;
            if (p.add_mode && l % li == 0 && l / li < 3) {
                np.add_mode = p.add_mode; np.ctrl = off(c->ctrl[l / li].p, p.ctrl_off, e); np.T = p.Tn; np.row0 = p.ctrl_row0; np.n_tok = c->ctrl_ntok; np.cs = p.cs;
            }
            car_launch_rmsnorm(mode, &np, rows, st);
        }
        { GemmP q = gp(p.xn, D, Wp(c, L + "attention.wqkv.weight"), D, p.qkv, 3 * D, (int)rows, 3 * D, D); car_launch_gemm(mode, AMODE_PLAIN, &q, st); }
        p.rope(l);
        const AttnCall at = {p.qkv, off(p.qkv, (size_t)D, e), off(p.qkv, (size_t)2 * D, e), 3 * D, p.att, p.nseq, p.Tn, g.n_head, 64, 0.125f, ATTN_CAUSAL, p.mask, nullptr, p.col0};
        if (attn_run(c, at, st)) return -1;      // flash64 takes every shape these passes build (engine_attn.hip)
        gpt_layer_tail(c, L, p.h, p.xn, p.att, p.mid, rows, st);
    }
    NormP np; memset(&np, 0, sizeof(np)); np.h_in = p.h; np.xn = p.xn; np.w = Wp(c, "norm.weight"); np.D = D; np.eps = g.norm_eps;
    car_launch_rmsnorm(mode, &np, rows, st);
    return 0;
}
