// engine_score.hip — car_score: the per-token negative log-likelihood of GIVEN image tokens in one parallel pass (the training branch of
// Transformer.forward, gpt_t2i.py:420-431,456-459,472-481, evaluated with generate()'s inference conventions), and car_debug_score_rows.
// (one of the translation units behind include/controlar_hip.h; shared declarations: engine_internal.h)
//
// The causal structure makes the logits of all n_new positions computable from ONE pass over Ts = Tv + n_new - 1 rows per sequence: the Tv rows of the
// prefix window (as car_generate's prefill: the prompt pass of engine_prompt.hip) followed by the embeddings of tokens[:, :n_new-1]; the logits row that generate()
// hands to sample() at step i is the output of sequence row Tv - 1 + i.  Stages C (control tokens) and D (text prefix) and the layer loop are the prefill's,
// on the same generic GEMMs (row-count agnostic; every output element sums its k-blocks in order whatever M), with three differences: the control token j is
// added on row Tv - 1 + j at layers 0, n/3, 2n/3 (rmsnorm add_mode 3; the unconditional half adds exact zeros), RoPE runs in place without a KV cache
// (score.hip), and the final norm feeds the fused projection + cross-entropy kernel instead of a logits GEMM.  Nothing of the context that car_generate
// reads later is changed except scratch that it rewrites itself.
//
// Chunk rule (fixed): at most cap = max(1, 16384 / (mult * Ts)) consecutive images per chunk (mult = 2 under CFG: an image and its unconditional twin are
// always in the same chunk, rows [cond | uncond]); in the fp32 mode the cap is lowered until the chunk's score tensor b * H * Ts * Ts * 4 bytes fits 1 GiB.
// The call runs ceil(B / cap) chunks of ceil(B / chunks) images (equal sizes: every chunk's GEMMs see the same row count; the last may be shorter).
// A chunk runs the whole pass, so the activation buffers hold at most max(16384, mult * Ts) rows and the weights are read once per chunk.  No kernel of the
// pass lets a row depend on its chunk-mates, and the window start is a multiple of 32 — the key block of flash64, a multiple of the 16-wide k-blocks of the
// fp32 P·V product; the fp32 softmax sums a column in the thread of its absolute position — so leading masked columns add exact zeros: a sequence scored
// alone returns the bits of its slice of any batch, in both modes, CFG pair included.
#include "engine_internal.h"

extern "C" {
int car_score_nparts(int V);
int car_launch_score(int mode, const ScoreP* p, float* nll, int* err_flag, hipStream_t st);
void car_launch_score_embed(int mode, const void* emb, const int* tokens, void* h, int nseq, int ng, int n_new, int Ts, int Tv, int D, int V, int* err_flag, hipStream_t st);
void car_launch_score_rope(int mode, void* qkv, const float* rope, int b, int Tn, int H, int dim, int t0, hipStream_t st);
void car_launch_score_mask(const int64_t* emb_mask, unsigned char* out, int nseq, int ng, int img0, int T, int t0, int Tv, int Ts, hipStream_t st);
}

enum { kScoreRows = 16384 };                      // activation rows per chunk (the chunk rule above)
static const size_t kScoreTensorCap = (size_t)1 << 30;

extern "C" int car_score(car_ctx* c, const void* text_emb, int32_t text_dtype, const int64_t* emb_mask, int32_t B, int32_t n_new, int32_t use_control,
                         const car_sampling* sp, const int32_t* tokens, float* nll_out, float* logits_out, void* stream_) {
    return car_score_rows(c, text_emb, text_dtype, emb_mask, B, n_new, use_control, sp, nullptr, tokens, nll_out, logits_out, stream_);
}

// Row mode (trows != NULL): image i is scored under its own cfg_scale, cfg_interval and control_strength.  The projection kernel already mixes with a per-row
// scale (ScoreP::scale, the pair_scale plumbing of car_debug_score_rows): the table's scale / interval become one fp32 per (image, position) on the device.  The
// strength is folded into the image's control tokens after stage C, as in car_generate_rows, and the pass runs at cs = 1.  A chunk takes its slice of both.
extern "C" int car_score_rows(car_ctx* c, const void* text_emb, int32_t text_dtype, const int64_t* emb_mask, int32_t B, int32_t n_new, int32_t use_control,
                              const car_sampling* sp, const car_sampling_row* trows, const int32_t* tokens, float* nll_out, float* logits_out, void* stream_) {
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (c->cfg.model_type != 0) FAIL(c, "car_score: context was created for the c2i model; scoring covers the t2i model only");
    if (!c->finalized) FAIL(c, "car_score: call car_finalize_weights first");
    if (!c->has_gpt) FAIL(c, "car_score: this context holds no GPT weights");
    if (!text_emb || !sp || !tokens || !nll_out || B <= 0 || n_new <= 0) FAIL(c, "car_score: bad arguments");
    if (text_dtype != CAR_DT_F32 && text_dtype != CAR_DT_BF16) FAIL(c, "car_score: text dtype must be F32 or BF16");
    const car_config& g = c->cfg;
    if (g.vocab_size % 4) FAIL(c, "car_score: vocab_size must be a multiple of 4");
    const int T = g.cls_token_num;
    if (n_new > g.block_size) FAIL(c, "car_score: %d tokens exceed block_size %d (rope table rows, gpt_t2i.py:454)", n_new, g.block_size);
    if (use_control && (c->ctrl_B != B || c->ctrl_ntok < n_new)) FAIL(c, "car_score: control tokens cached for B=%d n=%d, requested B=%d n_new=%d (call car_encode_control first)", c->ctrl_B, c->ctrl_ntok, B, n_new);
    RowInfo ri = {sp->cfg_scale > 1.0f, false};
    if (trows && rows_check(c, "car_score_rows", trows, B, 0, &ri)) return -1;
    const bool use_cfg = ri.use_cfg;
    const int mult = use_cfg ? 2 : 1, b = mult * B;
    const float cs = (use_cfg && !trows) ? sp->control_strength : 1.0f;         // generate.py:87-92: strength ignored when cfg <= 1
    bool row_strength = false;
    if (trows && use_cfg && use_control) for (int i = 0; i < B; ++i) row_strength |= trows[i].control_strength != 1.0f;
    const int D = g.dim, Hn = g.n_head, Fh = g.ffn_hidden, V = g.vocab_size, n_tok = c->ctrl_ntok;
    const int mode = c->mode; const size_t e = c->esz; const bool fast = mode == CAR_BF16;
    if (D != Hn * 64) FAIL(c, "car_score: heads must be 64 wide");
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    if (ensure_host_flags(c)) return -1;
    int* err_flag = c->host_flags + 2;

    fence_in(c, caller);
    const SampleRow* rows_dev = nullptr; const float* row_scale = nullptr;
    if (trows) {
        if (rows_upload(c, trows, B, st)) return -1;
        rows_dev = (const SampleRow*)c->rows_dev.p;
        if (use_cfg) {
            NEED(c, c->row_scale, (size_t)B * n_new * 4);
            car_launch_row_mix_scale(rows_dev, (float*)c->row_scale.p, B, n_new, st);
            row_scale = (const float*)c->row_scale.p;
        }
    }
    // ---- the prefill window of car_generate on the valid tail of the left-padded prompts, its start a multiple of 32 (see the chunk rule)
    int Tv = T, t0 = 0;
    if (emb_mask && prompt_has_window(T) && (fast || T <= 128)) {
        // scratch of its own (ws[WS_LOGITS], the token loop's logits buffer, idle here): car_generate's device scalars stay as its car_get_stats expects them
        NEED(c, c->ws[WS_LOGITS], (size_t)(B + 4) * 4 + (size_t)B * T);
        int* jmin = (int*)c->ws[WS_LOGITS].p; int* jmin_min = jmin + B; unsigned char* mask_all = (unsigned char*)(jmin_min + 4);
        car_launch_score_mask(emb_mask, mask_all, B, B, 0, T, 0, T, T, st);      // [B][T]: the whole prefix of every image
        car_launch_mask_first_valid(mask_all, jmin, B, T, st);
        if (prompt_window(c, sp->first_valid_hint, jmin, B, jmin_min, T, 32, &t0, &Tv, st)) return -1;
    }
    const int Ts = Tv + n_new - 1;
    int nc = kScoreRows / (mult * Ts); if (nc < 1) nc = 1; if (nc > B) nc = B;
    const bool pf_flash = use_flash(c, 64);
    if (!pf_flash) while (nc > 1 && (size_t)nc * mult * Hn * Ts * Ts * 4 > kScoreTensorCap) --nc;
    nc = (B + (B + nc - 1) / nc - 1) / ((B + nc - 1) / nc);      // the same number of chunks, of equal size (the last one may be shorter)
    const int bc = mult * nc; const long rowsC = (long)bc * Ts;
    const int nparts = car_score_nparts(V);

    // ---- buffers (the prefill's workspaces, sized for one chunk)
    NEED(c, c->ws[WS_TEXT], (size_t)bc * Tv * g.caption_dim * e);
    NEED(c, c->ws[WS_H], (size_t)rowsC * D * e);
    NEED(c, c->ws[WS_XN], (size_t)rowsC * D * e);
    NEED(c, c->ws[WS_QKV], (size_t)rowsC * 3 * D * e);
    const AttnBytes ab = attn_bytes(c, bc, Ts, Hn, 64);
    { const size_t s4 = std::max(use_control ? (size_t)B * n_tok * D * e : 0, ab.S); if (s4) NEED(c, c->ws[WS_ATTN_S], s4); }      // control-MLP scratch, then S
    if (ab.P) NEED(c, c->ws[WS_ATTN_P], ab.P);
    NEED(c, c->ws[WS_ATTN_VT], ab.Vt);
    NEED(c, c->ws[WS_MID], (size_t)rowsC * (fast ? Fh : 3 * Fh) * e);
    NEED(c, c->ws[WS_ATT_OUT], (size_t)rowsC * D * e);
    NEED(c, c->ws[WS_PARTS], (size_t)nparts * nc * n_new * 16);
    NEED(c, c->maskw, (size_t)bc * Ts);
    if (use_control) { NEED(c, c->ws[WS_CTRL_MLP], (size_t)B * n_tok * D * e); for (int k = 0; k < 3; ++k) NEED(c, c->ctrl[k], (size_t)b * n_tok * D * e); }
    void *h = c->ws[WS_H].p, *xn = c->ws[WS_XN].p, *qkv = c->ws[WS_QKV].p, *mid = c->ws[WS_MID].p, *att = c->ws[WS_ATT_OUT].p;

    std::vector<int> chunk0;      // chunk ci = images [chunk0[ci], chunk0[ci + 1])
    for (int i0 = 0; i0 < B; i0 += nc) chunk0.push_back(i0);
    chunk0.push_back(B);
    const int n_chunks = (int)chunk0.size() - 1;
    // ---- C. control tokens of every chunk; rows [cond | zeros] per chunk
    if (use_control && prompt_control_tokens(c, chunk0.data(), n_chunks, use_cfg, row_strength ? rows_dev : nullptr, st)) return -1;
    int rc = 0;
    for (int ci = 0; ci < n_chunks; ++ci) {
        const int i0 = chunk0[ci], ng = chunk0[ci + 1] - i0, nseq = mult * ng;
        // ---- D. input rows: the window of the text prefix in the first Tv rows of every sequence, then the token embeddings
        prompt_text(c, text_emb, text_dtype, &chunk0[ci], 1, use_cfg, t0, Tv, att, st);
        HIPCHK(c, hipMemcpy2DAsync(h, (size_t)Ts * D * e, att, (size_t)Tv * D * e, (size_t)Tv * D * e, (size_t)nseq, hipMemcpyDeviceToDevice, st));
        car_launch_score_embed(mode, Wp(c, "tok_embeddings.weight"), tokens + (size_t)i0 * n_new, h, nseq, ng, n_new, Ts, Tv, D, V, err_flag, st);
        car_launch_score_mask(emb_mask, (unsigned char*)c->maskw.p, nseq, ng, i0, T, t0, Tv, Ts, st);
        // ---- E. the layers over all Ts rows: control token j lands on row Tv - 1 + j (add_mode 3), and RoPE runs in place (no KV cache)
        PromptPass pp = {h, xn, qkv, att, mid, nseq, Ts, (const unsigned char*)c->maskw.p, t0, use_control ? 3 : 0, Tv - 1, (size_t)mult * i0 * n_tok * D, cs,
                         [&](int) { car_launch_score_rope(mode, qkv, c->rope, nseq, Ts, Hn, D, t0, st); }};
        if (prompt_layers(c, pp, st)) { rc = -2; break; }
        // ---- the loss: rows Tv - 1 + i of every sequence against output.weight, the CFG pair mixed on the accumulators (score.hip)
        ScoreP p; memset(&p, 0, sizeof(p));
        p.x = xn; p.w = Wp(c, "output.weight"); p.targets = tokens + (size_t)i0 * n_new; p.part = (float*)c->ws[WS_PARTS].p;
        p.logits = logits_out ? logits_out + (size_t)i0 * n_new * V : nullptr;
        p.ldx = D; p.seq_stride = Ts; p.row_off = Tv - 1; p.unc_off = (long)ng * Ts; p.R = ng * n_new; p.V = V; p.D = D; p.rows_per_seq = n_new;
        p.paired = use_cfg ? 1 : 0; p.round_bf16 = fast ? 1 : 0;      // fast mode: the logits are a bf16 linear's output widened to fp32 (gpt_t2i.py:470), as the decode step rounds them
        p.cfg_interval = sp->cfg_interval; p.cfg_scale = sp->cfg_scale;
        if (row_scale) p.scale = row_scale + (size_t)i0 * n_new;      // row mode: the chunk's slice of the per-(image, position) scales
        if (car_launch_score(mode, &p, nll_out + (size_t)i0 * n_new, err_flag, st)) { rc = -3; break; }
    }
    fence_out(c, caller);
    if (rc == -2) FAIL(c, "car_score: the fused attention kernel rejected the pass's shape (dim=%d, rows per sequence=%d)", D, Ts);
    if (rc == -3) FAIL(c, "car_score: the projection kernel rejected the model's shape (dim=%d must be a multiple of 32, vocab=%d of 4; 16-byte aligned outputs)", D, V);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// Runs score.hip's fused projection + cross-entropy alone (tests).  x [R,D] and w [V,D] in the context's element type, device.  Without pair_scale: targets
// [R], nll [R], logits [R,V] or NULL.  With pair_scale [R/2] (R even): rows [0,R/2) are conditional, rows [R/2,R) their unconditional twins; targets, nll
// and logits have R/2 rows.  Works on any context (no weights needed).
extern "C" int car_debug_score_rows(car_ctx* c, const void* x, const void* w, const int32_t* targets, const float* pair_scale, int32_t R, int32_t V, int32_t D,
                                    int32_t round_bf16, float* nll, float* logits, void* stream_) {
    if (!c) return -1;
    if (check_sticky(c)) return -1;
    if (!x || !w || !targets || !nll || R <= 0 || V <= 0 || D <= 0) FAIL(c, "car_debug_score_rows: bad arguments");
    if (pair_scale && (R & 1)) FAIL(c, "car_debug_score_rows: a pair scale needs an even number of rows");
    if (ensure_host_flags(c)) return -1;
    const int Ro = pair_scale ? R / 2 : R;
    NEED(c, c->ws[WS_PARTS], (size_t)car_score_nparts(V) * Ro * 16);
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;
    fence_in(c, caller);
    ScoreP p; memset(&p, 0, sizeof(p));
    p.x = x; p.w = w; p.targets = targets; p.scale = pair_scale; p.part = (float*)c->ws[WS_PARTS].p; p.logits = logits;
    p.ldx = D; p.seq_stride = 0; p.row_off = 0; p.unc_off = Ro; p.R = Ro; p.V = V; p.D = D; p.rows_per_seq = Ro;
    p.paired = pair_scale ? 1 : 0; p.round_bf16 = round_bf16 ? 1 : 0; p.cfg_interval = -1; p.cfg_scale = 1.f;
    const int rc = car_launch_score(c->mode, &p, nll, c->host_flags + 2, st);
    fence_out(c, caller);
    if (rc) FAIL(c, "car_debug_score_rows: shape not supported (D %% %d, V %% 4, 16-byte aligned pointers)", c->mode == CAR_BF16 ? 32 : 16);
    HIPCHK(c, hipGetLastError());
    return 0;
}
