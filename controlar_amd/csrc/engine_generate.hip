// engine_generate.hip — stages D-G: the prefill (the prompt pass of engine_prompt.hip on car_generate's row layout), the captured decode step (bf16 fast path and the exact fp32 path), car_generate / car_generate_c2i
// (one of the translation units behind include/controlar_hip.h; shared declarations: engine_internal.h)
#include "engine_internal.h"

// ------------------------------------------------------------------------------------- decode step (one token for all b sequences)
// A chain = a contiguous slice [b0, b0+bg) of the sequences decoded as its own dependency chain.  With several chains the
// captured step has parallel branches: one chain's HBM-bound attention overlaps the other chains' latency-bound GEMMs
// (each chain re-streams the weights; a layer's 40 MB sits in the 256 MiB MALL between chains).
// DecodePlan: everything the captured step depends on beyond shapes and pointers — the schedule.  plan_decode() fills it once per generate call (before the
// buffers are sized: the arena in c->dec_parts depends on each chain's nsplit) and is the ONLY reader of the development switches for the decode loop; the
// step builders read the plan and StepBufs, and the plan's bytes are the first half of the graph-cache key (generate_impl).
enum { RA_NONE = 0, RA_SMALL, RA_NX, RA_MID, kEarlyChain = 8, kNoOverride = -0x7fffffff };      // RA_*: L2 run-ahead form of a chain (plan_decode)
struct ChainPlan {
    int b0, bg, nsplit;
    int attn_variant, attn_lds_pad, attn_pgrid, attn_no_trim;      // attn_no_trim: A/B, dec_attn2 loads whole edge blocks (Attn2P::no_trim); attn_variant: the decode2.hip variant (fast) / the `fused` form of car_launch_dec_attn_f32_ex (exact)
    int fuse_norm, normx, normx_max, normx_j4, staged_normx;      // the norms: GEMM prologue (<= 8 rows) / on the fly (<= normx_max rows; staged = NORM == 3 allowed) / rmsnorm2 launches
    int runahead, kv_runahead;                       // RA_*; the KV prefixes ride on w2's helpers (MEASURED, OFF)
};
struct DecodePlan {
    int mode, NG, mult, img0[9];                     // chain g = images [img0[g], img0[g+1]), `mult` rows per image ([cond | uncond] under CFG)
    int phase, gsteps, lin_prio, no_graph;           // phase offset between the chains, tokens per captured graph, raised wave priority of the linears / norms, eager launches
    int n_early;                                     // exact mode, three chains: the first n_early steps run as ONE chain, ch[kEarlyChain]
    int f32_resid_cfg, f32_qkv_tiled_from;           // exact-mode tile overrides on top of car_pick_gemm_f32_cfg2's answer (kNoOverride: none)
    ChainPlan ch[9];
};
static int attn_splits(int wg) { int n = 1; while (wg * n < 1024 && n < 16) n *= 2; return n; }      // fast mode: split-KV factor that gives `wg` (sequence, head) pairs 1024 workgroups

// `nsteps`, `skip`: decode steps of this call and the positions CAR_DEBUG_SKIP_STEPS starts late.  Touches no device state.
static void plan_decode(DecodePlan& pl, const car_config& g, int mode, int n_cu, int B, bool use_cfg, int S_max, int nsteps, int skip, bool has_mask) {
    memset(&pl, 0, sizeof(pl));
    const bool fast = mode == CAR_BF16;
    const int D = g.dim, Hn = g.n_head, Fh = g.ffn_hidden, V = g.vocab_size, T = g.cls_token_num;
    const int mult = use_cfg ? 2 : 1, b = mult * B;
    auto num = [](const char* v, int dflt) { return v ? atoi(v) : dflt; };
    // ---- the switches of the development library (all null in the shipped one), each read once
    const char *k_chains = CAR_KNOB("CAR_CHAINS"), *k_one_max = CAR_KNOB("CAR_ONE_LAUNCH_MAX"), *k_variant = CAR_KNOB("CAR_ATTN_VARIANT"), *k_phase = CAR_KNOB("CAR_PHASE_OFFSET"), *k_form = CAR_KNOB("CAR_ATTN_F32_FORM");
    const bool single_chain = CAR_KNOB("CAR_SINGLE_CHAIN"), no_early = CAR_KNOB("CAR_NO_EARLY_CHAIN"), split_small = CAR_KNOB("CAR_ATTN_SPLIT_SMALL"), old_small = CAR_KNOB("CAR_ATTN_OLD_SMALL");
    const bool no_runahead = CAR_KNOB("CAR_NO_RUNAHEAD"), no_small_fuse = CAR_KNOB("CAR_NO_SMALL_FUSE"), no_normx = CAR_KNOB("CAR_NO_NORMX"), kv_runahead = CAR_KNOB("CAR_KV_RUNAHEAD"), no_staged = CAR_KNOB("CAR_NO_STAGED_NORMX");
    const bool attn_no_trim = CAR_KNOB("CAR_ATTN_NO_TRIM");      // A/B: the attention's edge blocks stream all 32 rows (profiles/attn_trim_ab.txt)
    const int k_nsplit = num(CAR_KNOB("CAR_ATTN_NSPLIT"), 0), k_persist = num(CAR_KNOB("CAR_ATTN_PERSIST"), 0), lds_pad = num(CAR_KNOB("CAR_ATTN_LDS_PAD"), 0);      // A/B: shorter attention workgroups / persistent grid
    const int normx_max = num(CAR_KNOB("CAR_NORMX_MAX"), 48), normx_j4 = num(CAR_KNOB("CAR_NORMX_J4"), 0) != 0, k_gsteps = num(CAR_KNOB("CAR_GRAPH_STEPS"), 1);
    pl.mode = mode; pl.mult = mult; pl.lin_prio = num(CAR_KNOB("CAR_LINEAR_PRIO"), 0) != 0;
    pl.no_graph = CAR_KNOB("CAR_NO_GRAPH") != nullptr;      // profiling aid: eager launches (PMC collection cannot follow graph replays)
    pl.f32_resid_cfg = num(CAR_KNOB("CAR_F32_RESID_CFG"), kNoOverride); pl.f32_qkv_tiled_from = num(CAR_KNOB("CAR_F32_QKV_TILED_FROM"), kNoOverride);

    // ---- chains.  Two from 192 sequences up: each chain's GEMMs stream the weights once for <= 128+ rows, and one chain's HBM-bound
    // attention runs beside the other's latency-bound GEMMs (profiles/r02_decode_chain_sweep.txt)
    // (exact mode, round 4: the same cut — its linears are bound by the fp32 matrix pipe and its attention by HBM, so the two chains overlap DIFFERENT resources;
    //  the rows of a chain are computed exactly as in any other batch, so the cut does not touch the mode's batch invariance)
    int NG = b >= 192 ? 2 : 1;
    // exact mode, round 5 (profiles/r05_exact_probe_*.txt, 384 sequences, mean position, ms per step): 1 chain 18.50, 2 chains 18.10, 3 chains 17.42, 4 chains
    // 19.24, 6 chains 21.96.  The attention runs as 12-wave workgroups (decode_f32.hip: 24 of a CU's 32 wave slots), so the other chains' linears are resident
    // beside it; a chain's four linears have to finish while the OTHER chains stream their KV, and with three chains that window is two attentions long.
    if (!fast && b >= 288) NG = 3;
    if (k_chains) { const int v = atoi(k_chains); if (v >= 1 && v <= 8 && B / v >= 2) NG = v; }
    if (single_chain || NG > B) NG = 1;
    pl.NG = NG; for (int gi = 0; gi <= NG; ++gi) pl.img0[gi] = (int)((long)B * gi / NG);
    // ---- decode-loop schedule knobs, all OFF by default in fast mode: the MI355X sweeps of tools/overlap_sweep.py found none of them worth a
    // per cent (profiles/r02_overlap_sweep_v1..v3, DESIGN.md §4 — a linear beside the bandwidth-saturating attention makes no progress whatever
    // the schedule); they stay as A/B switches, and tests/test_parity_gpu.py pins that none of them changes a token.
    //   phase offset : with >= 2 chains, chain g+1 enters the step right after chain g's first wqkv (see enqueue_decode_step_fast)
    //   graph steps  : consecutive tokens captured per graph replay — the chains free-run across them (one fork / join and one phase
    //                  offset per `gsteps` tokens instead of per token); the remainder runs on a single-step graph
    //   linear prio  : s_setprio on the linears / norms
    pl.phase = NG >= 2 && (k_phase ? atoi(k_phase) != 0 : !fast);      // exact mode: the second chain enters half a layer late, so that attention meets linears, not attention
    pl.gsteps = fast && k_gsteps >= 1 && k_gsteps <= 64 ? k_gsteps : 1;
    const int nsplit_exact = (S_max + AF_SPLIT - 1) / AF_SPLIT;
    const bool fused = (long)Hn * b >= 2048 && nsplit_exact <= 8;
    // several chains: 12-wave attention workgroups (two per CU = 24 of its 32 wave slots), so that the other chain's linears find room beside it
    auto plan_exact = [&](ChainPlan& cp) { cp.nsplit = nsplit_exact; cp.attn_variant = fused ? num(k_form, cp.bg < b ? 3 : 1) : 0; };
    for (int gi = 0; gi < NG; ++gi) {
        ChainPlan& cp = pl.ch[gi]; const int bg = mult * (pl.img0[gi + 1] - pl.img0[gi]);
        cp.b0 = mult * pl.img0[gi]; cp.bg = bg;
        if (!fast) { plan_exact(cp); continue; }      // exact mode: a chain is a row range of the shared row-major buffers
        // a handful of sequences (<= 240 (sequence, head) pairs = 12 XL sequences): ONE launch of 16-wave workgroups instead of split-KV + combine —
        // one dependent kernel less per layer.  tools/small_ab.py on MI355X (XL, 1024 tokens, ms per step, same process): 2 rows 1.548 -> 1.406,
        // 8 rows 1.611 -> 1.465, 12 rows 1.887 -> 1.725; at 16 rows the split form wins again (1.890 vs 1.923)  [profiles/r03_small_ab.txt]
        // (round 6: with dec_attn2s — two blocks in flight per wave — the one-launch form wins up to 24 XL sequences: 38.8 -> 38.1 us per layer at 16 rows, 47.5 -> 45.9 at 20,
        //  48.4 -> 46.9 at 24, tools/mid_ab.py with CAR_ONE_LAUNCH_MAX; 480 sixteen-wave workgroups still fit the chip in one round)
        const bool one_launch = (long)bg * Hn <= num(k_one_max, T <= 512 ? 480 : 240) && !split_small;
        cp.nsplit = one_launch ? 1 : attn_splits(bg * Hn);
        if (k_nsplit == 1 || k_nsplit == 2 || k_nsplit == 4 || k_nsplit == 8 || k_nsplit == 16) cp.nsplit = k_nsplit;
        // attention variant (decode2.hip; profiles/r02_kbench_*): 4 waves per (sequence, head) from 128 sequences up, 2 below; 16 in the one-launch small form
        // (round 6: the one-launch form is dec_attn2s_kernel, variant 162 — two blocks in flight per wave, bit-identical to 160; it needs T <= 512 and the jmin table)
        cp.attn_variant = (one_launch && cp.nsplit == 1) ? ((T <= 512 && !old_small) ? 162 : 160) : ((cp.nsplit == 1 && bg < 128) ? 20 : 40);
        cp.attn_variant = num(k_variant, cp.attn_variant); cp.attn_lds_pad = lds_pad; cp.attn_no_trim = attn_no_trim;
        // persistent attention grid: R resident workgroups per CU walk the (sequence, head) items in equal shares
        if (k_persist > 0 && k_persist <= 16 && cp.nsplit == 1) { const long items = (long)bg * Hn, cap = (long)n_cu * k_persist;
            if (items > cap) { const long per = (items + cap - 1) / cap; cp.attn_pgrid = (int)((items + per - 1) / per); }
        }
        // tiny chains (<= 8 rows): the latency-bound regime (BASELINE configs 2, 4, 5).  The two RMSNorms of a layer and the final norm run
        // in the prologue of the GEMM that consumes them (dec_gemm NORM variant), and the attention is ONE launch of 16-wave workgroups
        // (no split-KV partials, no combine kernel): 5 dependent kernels per layer instead of 8.  Measured on MI355X with the layer loop of
        // experiments/small_chain (profiles/r03_small_chain.txt, position 631, us per layer): 2 rows 40.2 -> 35.2, 4 rows 41.6 -> 35.7,
        // 8 rows 47.8 -> 37.4 with 8-wave tiles (one row of the prologue norm per wave); from 12 rows up the fused prologue (every workgroup
        // repeats the norm of all rows) no longer wins (44.1 either way at 12, 50.1 vs 49.4 at 16) and the separate norm kernels stay.
        // The floor of this structure is the kernel boundary itself: 5 EMPTY kernels per layer cost 8.3 us.
        cp.fuse_norm = bg <= 8 && D <= 2048 && !no_small_fuse;
        // chains of up to 48 rows (round 4, experiments/lat_probe: profiles/r04_lat_probe_v5_*): the RMSNorm in front of wqkv / w1|w3 / output is applied ON THE FLY.
        // The RESID linear that produced the residual stream (wo, w2) leaves each row's sum of squares as per-tile partials; the consumer folds them into rstd
        // and normalises the bf16 residual rows it loads as its X operand in registers (dec_gemm NORM == 2).  Against the prologue form (<= 8 rows: a barrier-
        // separated norm in front of the main loop, 3.6-6.0 us of a 6-8 us kernel) and against the separate rmsnorm2 kernels (> 8 rows: two dependent launches of
        // ~6 us per layer) the measured layer goes 37.0 -> 34.4 us at 2 rows, 39.4 -> 35.7 at 8, 66.5 -> 61.6 at 32; at 64 rows it is a draw (83.3 / 82.9: the
        // 960 workgroups of wqkv each repeat the row statistics) and at 128 a loss (120 / 125), so larger chains keep the norm kernels.  The first norm of layer 0
        // (token gather) and of the three control-add layers changes the stream before it is normed: those keep the prologue / kernel form.
        cp.normx_max = normx_max; cp.normx_j4 = normx_j4; cp.staged_normx = !no_staged;
        cp.normx = bg <= normx_max && D % 128 == 0 && D <= 2048 && !no_normx;      // D/32 and D/16 partials per row: multiples of 4, at most 128 (the fold's 16-byte loads)
        // L2 run-ahead (round 6).  The per-XCD L2 survives a kernel boundary (experiments/xk_cache: a region the same XCD read one kernel earlier streams at L2 speed), and
        // kernels that occupy a fraction of the 256 CUs carry HELPER workgroups that touch the weights of the kernels that follow, XCD by XCD (decode2_params.h CAR_PF_FIELDS):
        //   RA_SMALL  chains of one m-block (BASELINE configs 2, 4, 5): attention (40-160 CUs) -> wo + w1|w3 of this layer, wo -> w2 of this layer, w2 -> wqkv of the next layer
        //             (the last layer: the first 16 MB of the vocabulary projection), so that the HBM stream of a layer's 41 MB runs under its latency-bound kernels.
        //             experiments/lat_probe, 2 rows, position 631: 35.1 -> 32.7 us per layer.
        //   RA_NX     ONE chain of 17-normx_max rows (on-the-fly norm: few rmsnorm2 launches to ride on): wo (80-240 workgroups) hosts w1|w3 + w2, w2 hosts the next layer's wqkv;
        //             the rmsnorm2 launches that remain host helpers as in RA_MID
        //   RA_MID    ONE chain of more rows (BASELINE config 3): the rmsnorm2 launches in front of wqkv / w1|w3 / output are 4-48 workgroups; their helpers pull the weights of the
        //             linears behind them into the XCDs' L2s (attention_norm -> wqkv; ffn_norm -> w1|w3 + w2; final norm -> 16 MB of the vocabulary projection)
        if (n_cu >= 128 && !no_runahead) cp.runahead = bg <= 16 ? RA_SMALL : (bg != b ? RA_NONE : (bg <= normx_max ? RA_NX : RA_MID));
        cp.kv_runahead = kv_runahead && cp.attn_variant == 162 && ((bg * Hn) & 7) == 0;
    }
    // ---- exact mode, three chains: the FIRST positions run as ONE chain.  Chains buy overlap of one chain's KV stream with the others' linears at the price of
    // re-streaming the weights per chain and of smaller GEMMs; while the KV prefix is short there is little to overlap (profiles/r05_exact_probe_v5_positions.txt,
    // 384 sequences, ms per step, 1 / 3 chains: position 120 8.47 / 9.25, 220 10.08 / 10.44, 370 13.19 / 12.62, 629 18.50 / 17.45, 1120 28.87 / 27.04).  The
    // cross-over sits where a sequence's KV rows cost ~0.6 of its share of the linears: rows* = 0.087 · P / (8 · dim · n_layer) attended rows (177 for XL).  The
    // host knows the position of every replay, so the loop is two captured graphs; the per-chain (pos, step) scalars are rewritten between them.  Chains are
    // row ranges of the same buffers and every kernel is batch-invariant: the switch does not touch a token.
    if (!fast && NG == 3 && mult == 1 && !k_chains && !no_early) {
        const double P = (double)g.n_layer * (4.0 * D * D + 3.0 * (double)D * Fh) + (double)V * D;
        const int rows_star = (int)(0.087 * P / (8.0 * D * g.n_layer));
        const int attended0 = has_mask ? 24 : T;                       // attended prefix rows at the first decode step (left-padded captions: ~24 of 120 valid on average)
        pl.n_early = std::min(rows_star - attended0 - skip, nsteps); if (pl.n_early < 8) pl.n_early = 0;
        pl.ch[kEarlyChain].bg = b; plan_exact(pl.ch[kEarlyChain]);
    }
}

// What the step builders read besides the plan and the weights: the shared buffers, the call's shapes and each chain's pointers and sampler.
struct FastBufs { bf16_t *xn, *att, *mid, *q; float* logits; float* attn_part; float* ssq; };     // per-chain scratch (XP-packed activations; ssq: row sums of squares of the residual stream as per-tile partials [rows][dim/16])
struct ChainBind { int *pos, *step; FastBufs fb; SampleP sp; };
struct StepBufs {
    void *h, *xn, *qkv, *att, *mid; float* part; float* logits; int* cur;
    int b, SA, n_tok; bool use_ctrl; float cs; const unsigned char* maskb; const int* jmin;      // SA: KV rows per (sequence, head) (exact mode: S_max)
    ChainBind ch[9];                                 // as DecodePlan::ch
};

// bf16 fast path (decode2.hip): 7 kernels per layer — norm -> wqkv(+RoPE, KV write) -> attention -> wo(+residual) ->
// norm -> w1|w3(+SwiGLU) -> w2(+residual); every linear streams the weights once for all rows of the chain.
// `phase_ev` / `phase_dst` (multi-chain capture): right after this chain's FIRST wqkv the event is recorded and `phase_dst` (the next
// chain's stream) is made to wait for it — the next chain enters the step half a layer late, so that its latency-bound linears run
// under this chain's HBM-bound attention and vice versa (chains forked at the same node run in lockstep: both do their linears at the
// same time, then both their attention, and nothing is hidden).
static int enqueue_decode_step_fast(car_ctx* c, const StepBufs& sb, const DecodePlan& pl, int ci, hipStream_t st, hipEvent_t phase_ev, hipStream_t phase_dst) {
    const car_config& g = c->cfg;
    const ChainPlan& cp = pl.ch[ci]; const ChainBind& cb = sb.ch[ci]; const FastBufs& fb = cb.fb;
    const int D = g.dim, Hn = g.n_head, Fh = g.ffn_hidden, li = g.n_layer / 3, V = g.vocab_size, T = g.cls_token_num;
    const int b = cp.bg, b0 = cp.b0, nsplit = cp.nsplit, SA = sb.SA, n_tok = sb.n_tok, prio = pl.lin_prio;
    const size_t kv_layer = (size_t)sb.b * Hn * SA * 64, kv_off = (size_t)b0 * Hn * SA * 64;
    bf16_t* h = (bf16_t*)sb.h + (size_t)b0 * D;
    const bool f8 = g.decode_weight_fp8 != 0;
    int nk = 0, bad_cfg = 0;
    const bool ra_lin = cp.runahead == RA_SMALL || cp.runahead == RA_NX, ra_norm = cp.runahead == RA_NX || cp.runahead == RA_MID;      // helpers ride on the attention / linears, on the rmsnorm2 launches
    auto wimg = [&](const std::string& wname, const void*& ptr, unsigned& bytes, size_t cap = (size_t)24 << 20) {
        auto it = c->w.find(wname + (f8 ? "#pk8" : "#pk"));
        if (it == c->w.end()) { ptr = nullptr; bytes = 0; return; }
        ptr = it->second.p; bytes = (unsigned)std::min(it->second.bytes, cap);
    };
    auto helpers_for = [&](bool on, int main_wgs) -> int {      // helper workgroups beside `main_wgs` workgroups: fill the chip once, multiple of 8 (the helper's XCD arithmetic), at least 32, at most 192
        if (!on || (main_wgs & 7)) return 0;
        const int n = std::min(((c->n_cu - main_wgs) / 8) * 8, 192);
        return n >= 32 ? n : 0;
    };
    auto ctrl_at = [&](int l) { return sb.use_ctrl && l < g.n_layer && l % li == 0 && l / li < 3; };      // a control token is added in front of layer l
    // returns the number of sum-of-squares partials per row the kernel leaves in p.ssq_out (0 if it writes none)
    auto gemm = [&](const std::string& wname, const bf16_t* X, int N, int K, int epi, GemmDP gp_) -> int {
        GemmDP p = gp_;
        p.W = (const bf16_t*)Wp(c, wname + (f8 ? "#pk8" : "#pk")); p.X = X; p.M = b; p.N = N; p.K = K;
        p.wscale = f8 ? (const float*)Wp(c, wname + "#sc") : nullptr; p.f8_mfma = g.decode_weight_fp8 == 2;
        int cfg = car_pick_gemm_cfg(b, N, K, epi);
        // 49-64 rows behind an on-the-fly norm: ALL four m-blocks in one workgroup (J = 4), so the row statistics are folded once per weight tile instead of
        // once per (weight tile, m-block) — 240 workgroups of wqkv instead of 960, each re-reading the same 20 KB of partials (profiles/r04_lat_probe_v5_rows64.txt)
        if (p.ssq_in && b > 48 && b <= 64 && cp.normx_j4) cfg = ((epi == EPI_SWIGLU || N >= 6144) ? 200 : 100) + 40 + 1;
        const int I = cfg / 100, J = (cfg / 10) % 10, Mb = (b + 15) / 16;
        p.w_nt = ((Mb + J - 1) / J == 1 ? 1 : 0) | (prio ? 2 : 0);      // bit 0: non-temporal weight stream, bit 1: raised wave priority
        if (p.pf_wgs > 0) p.pf_wgs = std::min(helpers_for(ra_lin, (N / (16 * I)) * ((Mb + J - 1) / J)), 160);      // (the caller marks the kernels that host helpers)
        if (p.ssq_out) p.ssq_ld = N / (16 * (I >= 2 ? 2 : 1));
        if (car_launch_dec_gemm_cfg_ex(&p, epi, cfg, cp.staged_normx, st)) bad_cfg = cfg;
        ++nk;
        return p.ssq_out ? p.ssq_ld : 0;
    };
    GemmDP z; memset(&z, 0, sizeof(z));
    int ssq_np = 0;                                                   // partials per row currently valid in fb.ssq (0: none)
    bf16_t* hc = h;                                                  // the residual stream; ping-pongs with `halt` when a control token is added
    bf16_t* halt = (bf16_t*)sb.xn + (size_t)b0 * D;                  // (the prefill's xn buffer is idle during decode)
    // a separate rmsnorm2 launch in front of layer l's wqkv (l >= 0: [token gather at layer 0] (+ control add at layers 0, n/3, 2n/3) -> h ; norm -> xn, packed) or of
    // another linear (l < 0); its run-ahead helpers pull the weight images `pf0` (at most `cap0` bytes) and `pf1`
    auto norm_kernel = [&](const std::string& wname, int l, const std::string& pf0, const std::string& pf1, size_t cap0 = (size_t)24 << 20) {
        Norm2P np; memset(&np, 0, sizeof(np));
        np.h_in = h; np.xn = fb.xn; np.w = (const bf16_t*)Wp(c, wname); np.D = D; np.eps = g.norm_eps; np.add = prio ? 2 : 0;
        if (l == 0) { np.emb = (const bf16_t*)Wp(c, "tok_embeddings.weight"); np.idx = sb.cur + b0; np.h_out = h; }
        if (l >= 0 && ctrl_at(l)) {
            np.add |= 1; np.ctrl = (const bf16_t*)c->ctrl[l / li].p + (size_t)b0 * n_tok * D; np.pos = cb.pos; np.T = T; np.n_tok = n_tok; np.cs = sb.cs; np.h_out = h;
        }
        np.pf_wgs = helpers_for(ra_norm, (b + 3) / 4);
        if (np.pf_wgs > 0) { wimg(pf0, np.pf_p0, np.pf_b0, cap0); if (!pf1.empty()) wimg(pf1, np.pf_p1, np.pf_b1); }
        car_launch_rmsnorm2(&np, b, st); ++nk;
    };
    auto normx_fields = [&](GemmDP& q, const std::string& wname) { q.nw = (const bf16_t*)Wp(c, wname); q.neps = g.norm_eps; q.nh_in = hc; q.ssq_in = fb.ssq; q.ssq_np = ssq_np; };
    auto norm_fields = [&](GemmDP& q, const std::string& wname, int l, bool first_of_layer) {
        q.nw = (const bf16_t*)Wp(c, wname); q.neps = g.norm_eps; q.nh_in = hc; q.pos = cb.pos;
        if (first_of_layer && l == 0) { q.nemb = (const bf16_t*)Wp(c, "tok_embeddings.weight"); q.nidx = sb.cur + b0; q.nh_out = h; }
        if (first_of_layer && ctrl_at(l)) {
            q.nadd = 1; q.nctrl = (const bf16_t*)c->ctrl[l / li].p + (size_t)b0 * n_tok * D; q.nT = T; q.n_tok = n_tok; q.ncs = sb.cs;
            q.nh_out = l == 0 ? h : (hc == h ? halt : h);            // never in place: every workgroup re-reads the un-added stream
        }
    };
    // the norm in front of a linear: on the fly (valid partials in fb.ssq), in the GEMM's prologue, or its own launch
    auto norm_for = [&](GemmDP& q, bool nx, const std::string& wname, int l, bool first_of_layer, const std::string& pf0, const std::string& pf1, size_t cap0 = (size_t)24 << 20) {
        if (nx) normx_fields(q, wname);
        else if (cp.fuse_norm) norm_fields(q, wname, l, first_of_layer);
        else norm_kernel(wname, first_of_layer ? l : -1, pf0, pf1, cap0);
    };
    for (int l = 0; l < g.n_layer; ++l) {
        const std::string L = "layers." + std::to_string(l) + ".";
        const size_t kvb = g.kv_cache_fp8 ? 1 : 2;          // bytes per cached element (e4m3 / bf16)
        bf16_t* kc = (bf16_t*)((char*)c->kv.p + ((size_t)(2 * l) * kv_layer + kv_off) * kvb); bf16_t* vc = (bf16_t*)((char*)c->kv.p + ((size_t)(2 * l + 1) * kv_layer + kv_off) * kvb);
        const bool special = l == 0 || ctrl_at(l);      // the stream changes (gather / control add) before this layer's first norm
        const bool nx1 = cp.normx && !special && ssq_np > 0;
        {
            GemmDP q = z; q.qout = fb.q; q.kc = kc; q.vc = vc; q.rope = c->rope; q.pos = cb.pos; q.H = Hn; q.SA = SA; q.dim = D; q.kv8 = g.kv_cache_fp8 ? 1 : 0;
            norm_for(q, nx1, L + "attention_norm.weight", l, true, L + "attention.wqkv.weight", "");
            gemm(L + "attention.wqkv.weight", fb.xn, 3 * D, D, EPI_QKV, q);
            if (!nx1 && cp.fuse_norm && q.nh_out) hc = q.nh_out;
            if (l == 0 && phase_ev) { (void)hipEventRecord(phase_ev, st); (void)hipStreamWaitEvent(phase_dst, phase_ev, 0); }
        }
        {
            Attn2P ap; memset(&ap, 0, sizeof(ap));
            ap.q = fb.q; ap.kc = kc; ap.vc = vc; ap.pos = cb.pos; ap.mask = sb.maskb ? sb.maskb + (size_t)b0 * T : nullptr; ap.jmin = sb.jmin ? sb.jmin + b0 : nullptr;
            ap.out = fb.att; ap.part = fb.attn_part; ap.H = Hn; ap.SA = SA; ap.T = T; ap.dim = D; ap.nsplit = nsplit; ap.out_packed = 1; ap.kv8 = g.kv_cache_fp8 ? 1 : 0; ap.no_trim = cp.attn_no_trim;
            if (cp.attn_pgrid > 0 && nsplit == 1) { ap.n_seq = b; ap.pgrid = cp.attn_pgrid; }
            if (cp.attn_variant == 162) {      // the small-batch kernel hosts the run-ahead for wo and w1|w3
                ap.pf_wgs = helpers_for(ra_lin, b * Hn);
                if (ap.pf_wgs > 0) { wimg(L + "attention.wo.weight", ap.pf_p0, ap.pf_b0); wimg(L + "feed_forward.w13.weight", ap.pf_p1, ap.pf_b1); }
            }
            car_launch_dec_attn2_var(&ap, b, cp.attn_variant, cp.attn_lds_pad, st); nk += nsplit > 1 ? 2 : 1;
        }
        { GemmDP q = z; q.h = hc; if (cp.normx) q.ssq_out = fb.ssq;
          if (cp.runahead == RA_SMALL) { q.pf_wgs = 1; wimg(L + "feed_forward.w2.weight", q.pf_p0, q.pf_b0); }
          else if (cp.runahead == RA_NX) { q.pf_wgs = 1; wimg(L + "feed_forward.w13.weight", q.pf_p0, q.pf_b0); wimg(L + "feed_forward.w2.weight", q.pf_p1, q.pf_b1); }
          ssq_np = gemm(L + "attention.wo.weight", fb.att, D, D, EPI_RESID, q); }
        { GemmDP q = z; q.outp = fb.mid;
          norm_for(q, cp.normx && ssq_np > 0, L + "ffn_norm.weight", l, false, L + "feed_forward.w13.weight", L + "feed_forward.w2.weight");
          gemm(L + "feed_forward.w13.weight", fb.xn, 2 * Fh, D, EPI_SWIGLU, q); }
        {   // w2 leaves the sums of squares for the next layer's first norm (or the final norm) unless that layer adds a control token first
            GemmDP q = z; q.h = hc; if (cp.normx && !ctrl_at(l + 1)) q.ssq_out = fb.ssq;
            if (ra_lin) {
                q.pf_wgs = 1; wimg(l + 1 < g.n_layer ? "layers." + std::to_string(l + 1) + ".attention.wqkv.weight" : std::string("output.weight"), q.pf_p0, q.pf_b0, (size_t)16 << 20);
                // the KV prefixes the next layer's attention will stream — MEASURED, OFF (development switch): the attention shrinks 6.5 -> 4.4 us at 2 rows, but w2 and the two
                // boundaries behind the helpers grow by as much (32.4 vs 32.6 us per layer at position 631, 31.7 vs 32.4 at 200, 36.6 vs 39.7 at 8 rows; only past position
                // ~1000 a gain: 34.8 -> 33.3): every kernel's span is already its own critical path, and a helper load that outlives it is paid at the boundary
                if (l + 1 < g.n_layer && cp.kv_runahead) {
                    q.pf_kc = (const char*)c->kv.p + ((size_t)(2 * (l + 1)) * kv_layer + kv_off) * kvb; q.pf_vc = (const char*)c->kv.p + ((size_t)(2 * (l + 1) + 1) * kv_layer + kv_off) * kvb;
                    q.pf_pos = cb.pos; q.pf_items = b * Hn; q.pf_SA = SA; q.pf_kvb = (int)kvb;
                }
            }
            ssq_np = gemm(L + "feed_forward.w2.weight", fb.mid, D, Fh, EPI_RESID, q);
        }
    }
    { GemmDP q = z; q.outf = fb.logits;
      norm_for(q, cp.normx && ssq_np > 0, "norm.weight", g.n_layer, false, "output.weight", "", (size_t)16 << 20);
      gemm("output.weight", fb.xn, V, D, EPI_LOGITS, q); }
    car_launch_advance(cb.pos, cb.step, st); ++nk;
    SampleP sp = cb.sp; sp.logits = fb.logits; sp.logits_ks = 0; sp.round_bf16 = 0;
    car_launch_sample_greedy(&sp, st); ++nk;
    c->n_dec_kernels = nk;
    if (bad_cfg) FAIL(c, "decode GEMM: tile configuration %d rejected for this model's dimensions (b=%d, dim=%d, ffn=%d, vocab=%d)", bad_cfg, b, D, Fh, V);
    return 0;
}

// Exact mode (decode_f32.hip), round 5: 5 kernels per layer — wqkv(+on-the-fly attention_norm, RoPE, q scale, K/V rows written at *pos) -> attention (fixed
// 512-position splits folded in one launch) -> wo(+residual) -> w1|w3(+on-the-fly ffn_norm, SwiGLU) -> w2(+residual); layer 0 (token gather) and the three
// control-add layers put one `rmsnorm` launch in its add-only form in front.  Every linear runs on the exact fp32 MFMA over the fragment-packed weights; the
// linears behind a norm multiply the RAW residual rows by the image that carries the norm weight in its columns and scale by rstd in the epilogue (round 4
// ran 8 kernels per layer: two rmsnorm launches and the split-KV combine).  Nothing here depends on the batch except the tile shape, which does not change
// an output's arithmetic: a sequence decodes to the same bits alone and in a batch of 384.
static int enqueue_decode_step(car_ctx* c, const StepBufs& sb, const DecodePlan& pl, int ci, hipStream_t st, hipEvent_t phase_ev, hipStream_t phase_dst) {
    // One chain = rows [b0, b0 + b) of the decoded sequences (every buffer is row-major over the sequences, so a chain is a row offset).  With two
    // chains the captured step has two branches: one chain's attention (HBM-bound) runs beside the other's linears (bound by the fp32 matrix pipe) — different
    // resources, unlike the bf16 step whose linears are latency-bound.  `phase_ev` / `phase_dst`: the next chain enters after this chain's first wqkv.
    const car_config& g = c->cfg; const int mode = c->mode; const size_t e = c->esz;
    const ChainPlan& cp = pl.ch[ci]; const ChainBind& cb = sb.ch[ci];
    const int D = g.dim, Hn = g.n_head, Fh = g.ffn_hidden, li = g.n_layer / 3, V = g.vocab_size, T = g.cls_token_num;
    const int b = cp.bg, b0 = cp.b0, nsplit = cp.nsplit, S_max = sb.SA, n_tok = sb.n_tok;
    const size_t kv_layer = (size_t)sb.b * Hn * S_max * 64, kv_off = (size_t)b0 * Hn * S_max * 64;
    int nk = 0, bad = 0;
    auto gemm = [&](const std::string& wname, const void* X, long ldx, int N, int K, int epi, GemmFP q) {
        q.W = (const float*)Wp(c, wname + "#pk32"); q.X = (const float*)X; q.ldx = ldx; q.M = b; q.N = N; q.K = K;
        int cfg = car_pick_gemm_f32_cfg2(b, N, K, epi, sb.b / (b > 0 ? b : 1));
        if (K % 128 == 0 && N % 64 == 0) {      // the shapes the LDS-tiled kernel takes: the A/B overrides of the plan
            if (epi == FEPI_RESID) { if (pl.f32_resid_cfg != kNoOverride && b >= 64) cfg = pl.f32_resid_cfg; }
            else if (N < 4096 && pl.f32_qkv_tiled_from != kNoOverride) cfg = b >= pl.f32_qkv_tiled_from ? 1212 : (b > 16 ? 22 : 21);
        }
        const int J = cfg % 10, Mb = (b + 15) / 16;
        q.w_nt = (cfg < 1000 && (Mb + J - 1) / J == 1 ? 1 : 0) | (pl.lin_prio ? 2 : 0);
        if (!q.W || car_launch_dec_gemm_f32_cfg(&q, epi, cfg, st)) bad = cfg ? cfg : -1;
        ++nk;
    };
    GemmFP z; memset(&z, 0, sizeof(z));
    GemmFP zn = z; zn.normx = 1; zn.neps = g.norm_eps;                  // the linears behind an RMSNorm
    float* h = (float*)sb.h + (size_t)b0 * D; float* att = (float*)sb.att + (size_t)b0 * D;
    float* mid = (float*)sb.mid + (size_t)b0 * Fh; float* logits = sb.logits + (size_t)b0 * V; float* part = sb.part + (size_t)b0 * Hn * nsplit * 66;
    float* qbuf = (float*)sb.qkv + (size_t)b0 * D;                      // [b][H][64] rotated, pre-scaled q (the prefill's qkv buffer is idle during decode)
    for (int l = 0; l < g.n_layer; ++l) {
        const std::string L = "layers." + std::to_string(l) + ".";
        float* kc = (float*)off(c->kv.p, (size_t)(2 * l) * kv_layer + kv_off, e); float* vc = (float*)off(c->kv.p, (size_t)(2 * l + 1) * kv_layer + kv_off, e);
        const bool ctrl_here = sb.use_ctrl && l % li == 0 && l / li < 3;
        if (l == 0 || ctrl_here) {   // token gather (layer 0), control add (layers 0, n/3, 2n/3): the residual stream changes before its norm
            NormP np; memset(&np, 0, sizeof(np));
            np.h_in = h; np.h_out = h; np.xn = nullptr; np.D = D; np.eps = g.norm_eps;
            if (l == 0) { np.emb = Wp(c, "tok_embeddings.weight"); np.idx = sb.cur + b0; }
            if (ctrl_here) { np.add_mode = 1; np.ctrl = off(c->ctrl[l / li].p, (size_t)b0 * n_tok * D, e); np.pos = cb.pos; np.T = T; np.n_tok = n_tok; np.cs = sb.cs; }
            car_launch_rmsnorm(mode, &np, b, st); ++nk;
        }
        { GemmFP q = zn; q.qout = qbuf; q.kc = kc; q.vc = vc; q.rope = c->rope; q.pos = cb.pos; q.H = Hn; q.S_max = S_max; q.dim = D;
          gemm(L + "attention.wqkv.weight", h, D, 3 * D, D, FEPI_QKV, q); }
        if (l == 0 && phase_ev) { (void)hipEventRecord(phase_ev, st); (void)hipStreamWaitEvent(phase_dst, phase_ev, 0); }
        {
            AttnFP ap; memset(&ap, 0, sizeof(ap));
            ap.q = qbuf; ap.kc = kc; ap.vc = vc; ap.pos = cb.pos; ap.mask = sb.maskb ? sb.maskb + (size_t)b0 * T : nullptr; ap.part = part; ap.out = att;
            ap.H = Hn; ap.S_max = S_max; ap.T = T; ap.dim = D; ap.nsplit_max = nsplit;
            car_launch_dec_attn_f32_ex(&ap, b, cp.attn_variant, st); nk += cp.attn_variant ? 1 : 2;      // one fused launch, or the split kernel + combine
        }
        { GemmFP q = z; q.out = h; q.ldo = D; q.R = h; gemm(L + "attention.wo.weight", att, D, D, D, FEPI_RESID, q); }
        { GemmFP q = zn; q.out = mid; q.ldo = Fh; gemm(L + "feed_forward.w13.weight", h, D, 2 * Fh, D, FEPI_SWIGLU, q); }
        { GemmFP q = z; q.out = h; q.ldo = D; q.R = h; gemm(L + "feed_forward.w2.weight", mid, Fh, D, Fh, FEPI_RESID, q); }
    }
    { GemmFP q = zn; q.out = logits; q.ldo = V; gemm("output.weight", h, D, V, D, FEPI_PLAIN, q); }      // final norm on the fly; fp32 logits (exact mode has no bf16 round)
    car_launch_advance(cb.pos, cb.step, st); ++nk;      // pos = T+i+1 consumed next step; step indexes the token being sampled
    SampleP sp = cb.sp; sp.logits = logits; sp.step_ptr = cb.step; car_launch_sample_greedy(&sp, st); ++nk;
    c->n_dec_kernels = nk;
    if (bad) FAIL(c, "exact-mode decode GEMM: tile configuration %d rejected (b=%d, dim=%d, ffn=%d, vocab=%d: N %% 32 and K %% 16 must be 0)", bad, b, D, Fh, V);
    return 0;
}

// host-only view of the edge-block lane predicates of dec_attn2_kernel (decode2_params.h attn2_edge_*; tests/test_attn_trim_cpu.py)
extern "C" int car_debug_attn_edge_mask(int32_t lo, int32_t hi, unsigned char* k_mask, unsigned char* v_mask) {
    if (!k_mask || !v_mask || lo < 0 || hi > 31 || lo > hi) return -1;
    for (int i = 0; i < 4; ++i) for (int l = 0; l < 64; ++l) {
        k_mask[i * 64 + l] = attn2_edge_k_lane(i, l, lo, hi) ? 1 : 0;
        v_mask[i * 64 + l] = attn2_edge_v_lane(l, lo, hi) ? 1 : 0;
    }
    return 0;
}

// ------------------------------------------------------------------------------------- generate
// `rows` (row mode, the *_rows entries): one car_sampling_row per image on the host, or NULL = the plain call, every image sampling with `sp`.
static int generate_impl(car_ctx* c, const void* text_emb, int32_t text_dtype, const int64_t* labels, const int64_t* emb_mask, int32_t B, int32_t n_new,
                         int32_t use_control, const car_sampling* sp, const car_sampling_row* rows, int32_t* out_tokens, const int32_t* forced_tokens,
                         float* logits_out, void* stream_);

extern "C" int car_generate_rows(car_ctx* c, const void* text_emb, int32_t text_dtype, const int64_t* emb_mask, int32_t B, int32_t n_new,
                                 int32_t use_control, const car_sampling* sp, const car_sampling_row* rows, int32_t* out_tokens, const int32_t* forced_tokens,
                                 float* logits_out, void* stream_) {
    if (!c) return -1;
    if (c->cfg.model_type != 0) FAIL(c, "car_generate: context was created for the c2i model; use car_generate_c2i");
    if (!text_emb) FAIL(c, "car_generate: bad arguments");
    if (text_dtype != CAR_DT_F32 && text_dtype != CAR_DT_BF16) FAIL(c, "car_generate: text dtype must be F32 or BF16");
    return generate_impl(c, text_emb, text_dtype, nullptr, emb_mask, B, n_new, use_control, sp, rows, out_tokens, forced_tokens, logits_out, stream_);
}
extern "C" int car_generate(car_ctx* c, const void* text_emb, int32_t text_dtype, const int64_t* emb_mask, int32_t B, int32_t n_new,
                            int32_t use_control, const car_sampling* sp, int32_t* out_tokens, const int32_t* forced_tokens,
                            float* logits_out, void* stream_) {
    return car_generate_rows(c, text_emb, text_dtype, emb_mask, B, n_new, use_control, sp, nullptr, out_tokens, forced_tokens, logits_out, stream_);
}

extern "C" int car_generate_c2i_rows(car_ctx* c, const int64_t* labels, int32_t B, int32_t n_new, int32_t use_control, const car_sampling* sp,
                                     const car_sampling_row* rows, int32_t* out_tokens, const int32_t* forced_tokens, float* logits_out, void* stream_) {
    if (!c) return -1;
    if (c->cfg.model_type != 1) FAIL(c, "car_generate_c2i: context was created for the t2i model; use car_generate");
    if (!labels) FAIL(c, "car_generate_c2i: bad arguments");
    return generate_impl(c, nullptr, CAR_DT_F32, labels, nullptr, B, n_new, use_control, sp, rows, out_tokens, forced_tokens, logits_out, stream_);
}
extern "C" int car_generate_c2i(car_ctx* c, const int64_t* labels, int32_t B, int32_t n_new, int32_t use_control, const car_sampling* sp,
                                int32_t* out_tokens, const int32_t* forced_tokens, float* logits_out, void* stream_) {
    return car_generate_c2i_rows(c, labels, B, n_new, use_control, sp, nullptr, out_tokens, forced_tokens, logits_out, stream_);
}

static int generate_impl(car_ctx* c, const void* text_emb, int32_t text_dtype, const int64_t* labels, const int64_t* emb_mask, int32_t B, int32_t n_new,
                         int32_t use_control, const car_sampling* sp, const car_sampling_row* rows, int32_t* out_tokens, const int32_t* forced_tokens,
                         float* logits_out, void* stream_) {
    if (check_sticky(c)) return -1;
#ifdef CAR_DEV_KNOBS
    // every switch read below (and by the kernels' launchers) counts into car_stats.dev_knobs_active; the counter runs across ALL entry points and is cleared by car_get_stats
    struct KnobLatch { car_ctx* c; int at_entry; ~KnobLatch() { const int d = g_car_knob_hits - at_entry; if (d > c->knob_hits) c->knob_hits = d; } } knob_latch{c, g_car_knob_hits};
#endif
    if (!c->finalized) FAIL(c, "car_generate: call car_finalize_weights first");
    if (!c->has_gpt) FAIL(c, "car_generate: this context holds VQ weights only");
    if (!sp || !out_tokens || B <= 0 || n_new <= 0) FAIL(c, "car_generate: bad arguments");
    const car_config& g = c->cfg;
    const bool c2i = g.model_type == 1;
    RowInfo ri = {sp->cfg_scale > 1.0f, sp->sample_logits != 0};
    if (rows) { if (rows_check(c, c2i ? "car_generate_c2i_rows" : "car_generate_rows", rows, B, g.vocab_size, &ri)) return -1; }
    else if (sp->sample_logits && g.vocab_size > 32768) FAIL(c, "car_generate: stochastic sampling supports vocab_size <= 32768");
    if (g.vocab_size % 4) FAIL(c, "car_generate: vocab_size must be a multiple of 4");
    const int T = g.cls_token_num;
    if (n_new > g.block_size) FAIL(c, "car_generate: max_new_tokens %d exceeds block_size %d (rope table rows, gpt_t2i.py:454)", n_new, g.block_size);
    if (use_control && (c->ctrl_B != B || c->ctrl_ntok < n_new)) FAIL(c, "car_generate: control tokens cached for B=%d n=%d, requested B=%d n_new=%d", c->ctrl_B, c->ctrl_ntok, B, n_new);
    const bool use_cfg = ri.use_cfg;
    const int b = use_cfg ? 2 * B : B;
    // generate.py:87-92: strength ignored when cfg <= 1; absent in gpt.py.  Row mode: every image's strength is folded into its control tokens once (stage C
    // below) and the kernels run at cs = 1 — the decode-loop kernels keep their scalar strength.
    const float cs = (use_cfg && !c2i && !rows) ? sp->control_strength : 1.0f;
    bool row_strength = false;
    if (rows && use_cfg && !c2i && use_control) for (int i = 0; i < B; ++i) row_strength |= rows[i].control_strength != 1.0f;
    const int S_max = (int)rup(T + n_new, 8);                       // gpt_t2i.py:395
    const int SA = c->mode == CAR_BF16 ? (int)rup(S_max, 32) : S_max;   // fast mode: packed KV streams hold whole 32-position blocks (decode2.hip)
    const int D = g.dim, Hn = g.n_head, Fh = g.ffn_hidden, V = g.vocab_size, n_tok = c->ctrl_ntok;
    const int mode = c->mode; const size_t e = c->esz;
    hipStream_t caller = (hipStream_t)stream_, st = c->stream;

    // ---- row layout.  Images are cut into NG groups; the rows of group g are contiguous: [cond rows | uncond rows] under CFG
    // (so every group is a self-contained chain for the decode loop), plain image order otherwise.  NG = 1 reproduces the
    // reference layout [cond 0..B-1 | uncond 0..B-1] (generate.py:158-163).
    const bool fast = mode == CAR_BF16;
    // profiling aid (tools/pmc_workload.py): start the decode loop `skip` positions late so that a handful of steps under
    // counter collection see a long KV prefix.  The skipped cache rows hold zeros / stale rows: tokens are meaningless.
    { int skip = 0; const char* ev = CAR_KNOB("CAR_DEBUG_SKIP_STEPS"); if (ev) { skip = atoi(ev); if (skip < 0 || skip > n_new - 2) skip = 0; } c->dbg_skip = skip; }
    const int nsteps = n_new - 1 - c->dbg_skip;
    DecodePlan pl; plan_decode(pl, g, mode, c->n_cu, B, use_cfg, S_max, nsteps, c->dbg_skip, emb_mask != nullptr);      // the decode loop's schedule (chains included), decided once
    const int NG = pl.NG, mult = pl.mult; const int* img0 = pl.img0;
    std::vector<int> row_img((size_t)b), row_unc((size_t)b);
    for (int gi = 0; gi < NG; ++gi) {
        const int ng = img0[gi + 1] - img0[gi], base = mult * img0[gi];
        for (int j = 0; j < ng; ++j) { row_img[(size_t)base + j] = img0[gi] + j; row_unc[(size_t)base + j] = 0;
                                       if (use_cfg) { row_img[(size_t)base + ng + j] = img0[gi] + j; row_unc[(size_t)base + ng + j] = 1; } }
    }

    // ---- buffers
    const size_t kv_layer = (size_t)b * Hn * SA * 64;
    const size_t kv_cap_before = c->kv.cap;        // ensure() never shrinks: a changed capacity IS a new allocation (the address may repeat)
    const size_t kv_e = (fast && g.kv_cache_fp8) ? 1 : e;        // opt-in e4m3 KV cache: one byte per element
    NEED(c, c->kv, (size_t)g.n_layer * 2 * kv_layer * kv_e);
    const bool kv_fresh = c->kv.cap != kv_cap_before;
    const long rowsP = (long)b * T;                                           // sizes the buffers; the prefill computes b * Tv rows, Tv <= T (the window below)
    NEED(c, c->ws[WS_TEXT], (size_t)b * T * g.caption_dim * e);               // text input (cond | uncond)
    NEED(c, c->ws[WS_H], (size_t)rowsP * D * e);                              // h (prefill)
    NEED(c, c->ws[WS_XN], (size_t)rowsP * D * e);
    NEED(c, c->ws[WS_QKV], (size_t)rowsP * 3 * D * e);
    const AttnBytes ab = attn_bytes(c, b, T, Hn, 64);                         // fused prefill attention: no score / probability tensors
    if (ab.S) NEED(c, c->ws[WS_ATTN_S], ab.S);
    if (ab.P) NEED(c, c->ws[WS_ATTN_P], ab.P);
    NEED(c, c->ws[WS_ATTN_VT], ab.Vt);
    NEED(c, c->ws[WS_MID], (size_t)rowsP * (mode == CAR_BF16 ? Fh : 3 * Fh) * e);  // ffn mid (+ interleaved w13 out in exact mode)
    NEED(c, c->ws[WS_ATT_OUT], (size_t)rowsP * D * e);
    NEED(c, c->ws[WS_LOGITS], (size_t)b * V * 4);                             // fp32
    // exact mode: KV splits with boundaries fixed in ABSOLUTE positions (AF_SPLIT rows each), whatever the batch — the split layout fixes the order in
    // which a row's softmax partial sums are folded, so a sequence decodes to the same bits in a batch of 1 and in a batch of 384 (every other
    // exact-mode kernel sums one fixed-order fp32 chain per output): tests/test_parity_gpu.py::test_exact_mode_is_batch_invariant,
    // bench.py --precision fp32 (row 0 = the XL golden).
    const int nsplit = fast ? attn_splits(b * Hn) : pl.ch[0].nsplit;
    NEED(c, c->ws[WS_PARTS], (size_t)b * Hn * nsplit * 66 * 4);               // split-KV partials
    NEED(c, c->ws[WS_CTRL_MLP], (size_t)B * (use_control ? n_tok : 1) * D * e);   // condition_mlp output
    // device scalars: [16 ints: (pos, step) of up to 8 chains] [cur_tok: b ints] [jmin: b ints] [jmin_min: 4 ints] [SampleDyn, 16-byte aligned]
    NEED(c, c->scal, (size_t)(16 + 2 * b + 4) * 4 + 16 + sizeof(SampleDyn) + 16);
    NEED(c, c->rowimg, (size_t)b * 4);
    NEED(c, c->tok_out, (size_t)B * n_new * 4);
    NEED(c, c->maskb, (size_t)b * T);
    for (int k = 0; k < 3; ++k) if (use_control) NEED(c, c->ctrl[k], (size_t)b * n_tok * D * e);

    fence_in(c, caller);
    HIPCHK(c, hipEventRecord(c->ev_t0, st));
    // The reference zero-fills fresh KVCache buffers every call (gpt_t2i.py:223-225, :391-405); slots that
    // were never written are always masked there and never read here (the attention kernels walk only valid rows), so
    // no per-call memset is needed.  A FRESH allocation is cleared once: the packed V stream is
    // consumed in 32-position blocks whose tail rows meet a zero probability — they must be finite, not uninitialised bits.
    if (kv_fresh) HIPCHK(c, hipMemsetAsync(c->kv.p, 0, c->kv.cap, st));
    // text-pad mask -> uint8 [b, T] (both CFG halves share it, generate.py:188), built on the device: no host round trip
    c->h_rowimg.assign(row_img.begin(), row_img.end());
    HIPCHK(c, hipMemcpyAsync(c->rowimg.p, c->h_rowimg.data(), (size_t)b * 4, hipMemcpyHostToDevice, st));
    car_launch_build_mask(emb_mask, (const int*)c->rowimg.p, (unsigned char*)c->maskb.p, b, T, st);
    int* pos = (int*)c->scal.p; int* step = pos + 1; int* cur = pos + 16; int* jmin = cur + b; int* jmin_min = jmin + b;
    SampleDyn* dyn = (SampleDyn*)(((uintptr_t)(jmin_min + 4) + 15) & ~(uintptr_t)15);
    c->h_dyn.seed = sp->seed; c->h_dyn.temperature = sp->temperature; c->h_dyn.top_k = sp->top_k; c->h_dyn.top_p = sp->top_p;
    HIPCHK(c, hipMemcpyAsync(dyn, &c->h_dyn, sizeof(SampleDyn), hipMemcpyHostToDevice, st));
    // row mode: the whole table in image order; chain g's sampler reads its slice at rows_dev + img0[g].  The values live in device memory, so a call with
    // other per-row values replays the captured graph.
    if (rows && rows_upload(c, rows, B, st)) return -1;
    const SampleRow* rows_dev = rows ? (const SampleRow*)c->rows_dev.p : nullptr;
    if (emb_mask) car_launch_mask_first_valid((const unsigned char*)c->maskb.p, jmin, b, T, st);
    // ---- prefill window (engine_prompt.hip): the prefill runs on the valid tail [t0, T) of the left-padded prompts, t0 a multiple of 16.  Its only host wait is
    // the 4-byte read of a call that brings a mask and no first_valid_hint (development build: CAR_NO_PREFILL_WINDOW=1 keeps all T rows and no wait).
    int Tv = T, t0 = 0;
    if (emb_mask && !c2i && prompt_has_window(T) && (fast || T <= 128) && !CAR_KNOB("CAR_NO_PREFILL_WINDOW") &&
        prompt_window(c, sp->first_valid_hint, jmin, b, jmin_min, T, 16, &t0, &Tv, st)) return -1;
    const unsigned char* pmask = (const unsigned char*)c->maskb.p;             // the prefill's mask: [b][Tv]
    if (t0 > 0) {
        NEED(c, c->maskw, (size_t)b * Tv);
        HIPCHK(c, hipMemcpy2DAsync(c->maskw.p, (size_t)Tv, (const unsigned char*)c->maskb.p + t0, (size_t)T, (size_t)Tv, (size_t)b, hipMemcpyDeviceToDevice, st));
        pmask = (const unsigned char*)c->maskw.p;
    }
    for (int i = 0; i < 8; ++i) { c->h_init[2 * i] = T + c->dbg_skip; c->h_init[2 * i + 1] = c->dbg_skip; }    // (pos, step) per chain: after prefill the first decode step runs at input_pos = T, sampling token index 1 (+ the profiling skip)
    car_launch_set_pos_step(pos, c->h_init[0], c->h_init[1], st);

    // ---- D. text prefix embed: cls_embedding.cap_proj (gpt_t2i.py:435), uncond rows = uncond_embedding (generate.py:157)
    void *h = c->ws[WS_H].p, *xn = c->ws[WS_XN].p, *qkv = c->ws[WS_QKV].p, *mid = c->ws[WS_MID].p, *att = c->ws[WS_ATT_OUT].p;
    float* logits = (float*)c->ws[WS_LOGITS].p;
    if (c2i) {
        // LabelEmbedder (gpt.py:89-96): h[b] = embedding_table[label]; CFG rows use the null class num_classes (generate.py:141).
        // The row -> table-index map is built on the device (no host round trip): an out-of-range label is clamped to the null class and
        // raises a sticky device flag that car_get_stats reports (the reference's nn.Embedding fails asynchronously on a GPU as well).
        c->h_rowunc.assign(row_unc.begin(), row_unc.end());
        NEED(c, c->rowunc, (size_t)b * 4 + 16);
        if (ensure_host_flags(c)) return -1;
        HIPCHK(c, hipMemcpyAsync(c->rowunc.p, c->h_rowunc.data(), (size_t)b * 4, hipMemcpyHostToDevice, st));
        int* didx = cur;       // cur_tok[b] is free until the prefill sampler writes it
        car_launch_label_index(labels, (const int*)c->rowimg.p, (const int*)c->rowunc.p, g.num_classes, didx, c->host_flags, b, st);
        car_launch_gather_rows(mode, Wp(c, "cls_embedding.embedding_table.weight"), didx, h, b, D, st);
    } else prompt_text(c, text_emb, text_dtype, img0, NG, use_cfg, t0, Tv, h, st);
    // ---- C. control tokens of every chain, cached for the whole call
    if (use_control) {
        NEED(c, c->ws[WS_ATTN_S], std::max((size_t)B * n_tok * D * e, ab.S));      // the control MLPs' scratch, idle until the prefill's attention (which may need it larger)
        if (prompt_control_tokens(c, img0, NG, use_cfg, row_strength ? rows_dev : nullptr, st)) return -1;
    }
    // ---- E. prefill over the prefix rows of the window [t0, T) (gpt_t2i.py:446-470): the control token 0 lands on every sequence's last row (add_mode 2), and
    // the rope step writes the rotated K and V rows into the cache
    PromptPass pp = {h, xn, qkv, att, mid, b, Tv, pmask, t0, use_control ? 2 : 0, 0, 0, cs, nullptr};
    if (fast) pp.rope = [&](int l) { car_launch_prefill_rope_kv2(qkv, off(c->kv.p, (size_t)(2 * l) * kv_layer, kv_e), off(c->kv.p, (size_t)(2 * l + 1) * kv_layer, kv_e), c->rope, b, Tv, Hn, D, SA, g.kv_cache_fp8 ? 1 : 0, t0, st); };
    else pp.rope = [&](int l) { car_launch_prefill_rope_kv(mode, qkv, off(c->kv.p, (size_t)(2 * l) * kv_layer, e), off(c->kv.p, (size_t)(2 * l + 1) * kv_layer, e), c->rope, b, Tv, Hn, D, S_max, t0, st); };
    if (prompt_layers(c, pp, st)) FAIL(c, "car_generate: the fused attention kernel rejected the prefill's shape (dim=%d, rows per sequence=%d)", D, Tv);
    // logits for the LAST prefix row only (generate.py:60 samples logits[:, -1])
    { GemmP q = gp(off(xn, (size_t)(Tv - 1) * D, e), (long)Tv * D, Wp(c, "output.weight"), D, logits, V, b, V, D); q.out_f32 = 1; car_launch_gemm(mode, AMODE_PLAIN, &q, st); }
    SampleP spp; memset(&spp, 0, sizeof(spp));
    spp.logits = logits; spp.B = B; spp.V = V; spp.use_cfg = use_cfg; spp.cfg_scale = sp->cfg_scale; spp.cfg_interval = sp->cfg_interval;
    spp.step_ptr = step; spp.n_new = n_new; spp.out_tokens = (int*)c->tok_out.p; spp.cur_tok = cur; spp.forced = forced_tokens; spp.logits_out = logits_out;
    spp.stochastic = ri.any_stochastic; spp.temperature = sp->temperature; spp.top_k = sp->top_k; spp.top_p = sp->top_p; spp.seed = sp->seed; spp.row0 = 0;
    spp.dyn = dyn;     // the sampling scalars live in device memory: changing the seed per call does not invalidate the captured graph
    if (rows) { spp.dyn = nullptr; spp.rows = rows_dev; spp.cfg_scale = 1.0f; spp.cfg_interval = -1; }      // row mode: every block reads its own row of the device table
    auto group_sampler = [&](int gi) {      // the sampler of group gi: its rows are [cond ng | uncond ng] starting at row mult*img0[gi]
        SampleP q = spp; const int i0 = img0[gi], ng = img0[gi + 1] - i0; const size_t rb = (size_t)mult * i0;
        q.B = ng; q.row0 = i0; q.logits = logits + rb * V; q.out_tokens = (int*)c->tok_out.p + (size_t)i0 * n_new; q.cur_tok = cur + rb;
        if (rows) { q.rows = rows_dev + i0; q.row0 = 0; }      // the chain's slice of the table; the Philox counter starts at the image's own rng_stream, not at its slot
        q.forced = forced_tokens ? forced_tokens + (size_t)i0 * n_new : nullptr;
        q.logits_out = logits_out ? logits_out + (size_t)i0 * n_new * V : nullptr;
        return q;
    };
    for (int gi = 0; gi < NG; ++gi) { SampleP q = group_sampler(gi); car_launch_sample_greedy(&q, st); }
    HIPCHK(c, hipEventRecord(c->ev_t1, st));

    // ---- F/G. decode loop: one captured step, replayed n_new-1 times (pos/step/token live on the device)
    StepBufs sb; memset(&sb, 0, sizeof(sb));
    sb.h = h; sb.xn = xn; sb.qkv = qkv; sb.att = att; sb.mid = mid; sb.part = (float*)c->ws[WS_PARTS].p; sb.logits = logits; sb.cur = cur;
    sb.b = b; sb.SA = SA; sb.n_tok = n_tok; sb.use_ctrl = use_control != 0; sb.cs = cs;
    sb.maskb = emb_mask ? (const unsigned char*)c->maskb.p : nullptr; sb.jmin = emb_mask ? jmin : nullptr;      // no text-pad mask: nothing to test per position
    c->stats.graph_used = 0;
    for (int gi = 0; gi < NG; ++gi) {      // scal layout: (pos, step) x 8 chains, then cur_tok[b], then jmin[b]
        ChainBind& cb = sb.ch[gi];
        cb.pos = pos + 2 * gi; cb.step = step + 2 * gi; cb.sp = group_sampler(gi); cb.sp.step_ptr = cb.step;      // (sp.logits: set per launch to the chain's logits)
    }
    { ChainBind& cb = sb.ch[kEarlyChain]; cb.pos = pos; cb.step = step; cb.sp = spp; }      // the early one-chain schedule of exact mode: all rows
    if (fast) {
        // per-chain scratch from one arena: XP-packed xn / att [Mb*16, D], mid [Mb*16, Fh], q [bg, D] (bf16); logits [bg, V],
        // split-KV partials (fp32), sum-of-squares partials.  Every slice is a multiple of 16 bytes.
        auto carve = [&](uintptr_t base) -> size_t {      // lays the chains' slices out from `base`; returns their total size
            size_t o = 0;
            auto take = [&](size_t bytes) { void* p = (void*)(base + o); o += bytes; return p; };
            for (int gi = 0; gi < NG; ++gi) {
                const size_t bg = (size_t)pl.ch[gi].bg, M16 = rup(bg, 16); FastBufs& f = sb.ch[gi].fb;
                f.xn = (bf16_t*)take(M16 * D * 2); f.att = (bf16_t*)take(M16 * D * 2); f.mid = (bf16_t*)take(M16 * Fh * 2); f.q = (bf16_t*)take(rup(bg * D * 2, 16));
                f.logits = (float*)take(bg * V * 4); f.attn_part = (float*)take(rup(bg * Hn * pl.ch[gi].nsplit * 66 * 4, 16)); f.ssq = (float*)take(rup(M16 * (size_t)(D / 16) * 4, 16));
            }
            return o;
        };
        NEED(c, c->dec_parts, carve(0));
        carve((uintptr_t)c->dec_parts.p);
    }
    bool capturing = false; int step_rc = 0;
    const auto step_one = fast ? enqueue_decode_step_fast : enqueue_decode_step;
    auto enqueue_steps = [&](int k, bool early) {      // k consecutive decode steps of every chain of the main schedule, or of the one chain of the early schedule
        const int c0 = early ? kEarlyChain : 0, n = early ? 1 : NG, phase = early ? 0 : pl.phase;
        if (n >= 2 && capturing) {         // the chains are parallel branches of the captured graph
            if (!phase) {
                (void)hipEventRecord(c->ev_fork, st);
                for (int gi = 1; gi < n; ++gi) (void)hipStreamWaitEvent(c->streamx[gi - 1], c->ev_fork, 0);
            }
            for (int gi = 0; gi < n; ++gi) {
                hipStream_t sg = gi == 0 ? st : c->streamx[gi - 1];
                for (int s = 0; s < k; ++s) {
                    const bool hand = phase && s == 0 && gi + 1 < n;      // chain gi+1's stream joins the capture through this event
                    step_rc |= step_one(c, sb, pl, c0 + gi, sg, hand ? c->ev_phase[gi] : nullptr, hand ? c->streamx[gi] : nullptr);
                }
                if (gi > 0) { (void)hipEventRecord(c->ev_joinx[gi - 1], sg); (void)hipStreamWaitEvent(st, c->ev_joinx[gi - 1], 0); }
            }
        } else {
            for (int s = 0; s < k; ++s)
                for (int gi = 0; gi < n; ++gi) step_rc |= step_one(c, sb, pl, c0 + gi, st, nullptr, nullptr);
        }
        c->n_dec_kernels *= n;             // kernel nodes of ONE step over all chains
    };
    if (nsteps > 0) {
        // The graph-cache key: the bytes of the plan and of the shapes and raw pointers that the capture bakes in (n_new: the sampler's row stride and per-chain
        // offsets).  INVARIANT: whatever the step builders read comes from the plan, from a field keyed here, or from the weights — the plan is the schedule and
        // the key, so a switch cannot change the captured kernels without changing the key.
        struct GraphShapes {
            int b, B, S_max, n_new, n_tok, nsplit, use_control, has_mask, cfg_interval, sample_logits, row_mode; float cs, cfg_scale; unsigned long long alloc_gen;
            const void *kv, *h, *xn, *att, *mid, *logits, *ctrl0, *maskb, *parts, *scal, *forced, *logits_out, *rows;
        } gs;
        memset(&gs, 0, sizeof(gs));      // (as plan_decode does for the plan: the padding is part of the key)
        gs.b = b; gs.B = B; gs.S_max = S_max; gs.n_new = n_new; gs.n_tok = n_tok; gs.nsplit = nsplit; gs.use_control = use_control; gs.has_mask = emb_mask ? 1 : 0;
        // sample_logits: the KIND of sampler kernel the step launches (car_launch_sample_greedy: stochastic when any row is).  Row mode: scale, interval and strength
        // live in the device table (the kernels get cs = 1), so they do not distinguish graphs — other per-row values replay the capture
        gs.cfg_interval = spp.cfg_interval; gs.sample_logits = spp.stochastic; gs.cs = cs; gs.cfg_scale = spp.cfg_scale; gs.row_mode = rows ? 1 : 0; gs.rows = rows_dev;
        gs.alloc_gen = g_alloc_gen;
        gs.kv = c->kv.p; gs.h = h; gs.xn = xn; gs.att = att; gs.mid = mid; gs.logits = logits; gs.ctrl0 = c->ctrl[0].p; gs.maskb = c->maskb.p;
        gs.parts = c->dec_parts.p ? c->dec_parts.p : c->ws[WS_PARTS].p; gs.scal = c->scal.p; gs.forced = forced_tokens; gs.logits_out = logits_out;
        std::string key((const char*)&pl, sizeof(pl)); key.append((const char*)&gs, sizeof(gs));
        // capture `k` steps into `ex` unless the cached exec already holds exactly this configuration
        auto get_exec = [&](hipGraphExec_t& ex, std::string& exkey, int k, bool early = false) -> bool {
            const std::string kk = key + "|k" + std::to_string(k) + (early ? "|early" : "");
            if (ex && exkey == kk) return true;
            if (ex) { (void)hipGraphExecDestroy(ex); ex = nullptr; exkey.clear(); }
            hipGraph_t graph = nullptr;
            if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); return false; }
            capturing = true; enqueue_steps(k, early); capturing = false;
            bool ok = hipStreamEndCapture(st, &graph) == hipSuccess && graph != nullptr;
            if (!ok) (void)hipGetLastError();
            // (per-node priorities were tried — attention low, linears high: hipGraphKernelNodeSetAttribute(hipKernelNodeAttributePriority) is
            //  rejected for every kernel node by HIP 7.2, profiles/r02_small_batch.txt)
            if (ok && hipGraphInstantiate(&ex, graph, nullptr, nullptr, 0) != hipSuccess) { ok = false; ex = nullptr; (void)hipGetLastError(); }
            if (graph) (void)hipGraphDestroy(graph);
            if (ok) exkey = kk;
            return ok;
        };
        const int n_early = pl.n_early, gsteps = pl.gsteps, nmain = nsteps - n_early;
        const int nrep = nmain / gsteps, nrem = nmain % gsteps;
        bool graph_ok = !pl.no_graph;
        // the scalars of ALL chains at the switch: (pos, step) after n_early steps
        for (int i = 0; i < 8; ++i) { c->h_init2[2 * i] = c->h_init[0] + n_early; c->h_init2[2 * i + 1] = c->h_init[1] + n_early; }
        if (graph_ok && n_early > 0) graph_ok = get_exec(c->gexec1, c->gkey1, 1, true);      // (exact mode: gexec1 is free, gsteps == 1)
        if (graph_ok && nrep > 0) graph_ok = get_exec(c->gexec, c->gkey, gsteps);
        if (graph_ok && nrem > 0) graph_ok = get_exec(gsteps > 1 ? c->gexec1 : c->gexec, gsteps > 1 ? c->gkey1 : c->gkey, 1);
        if (graph_ok && !step_rc) {
            for (int i = 0; i < n_early; ++i) HIPCHK(c, hipGraphLaunch(c->gexec1, st));
            if (n_early > 0 && nmain > 0) car_launch_set_pos_step(pos, c->h_init2[0], c->h_init2[1], st);
            for (int i = 0; i < nrep; ++i) HIPCHK(c, hipGraphLaunch(c->gexec, st));
            for (int i = 0; i < nrem; ++i) HIPCHK(c, hipGraphLaunch(gsteps > 1 ? c->gexec1 : c->gexec, st));
            c->stats.graph_used = 1;
        } else if (!step_rc) {
            for (int i = 0; i < n_early; ++i) enqueue_steps(1, true);
            if (n_early > 0 && nmain > 0) car_launch_set_pos_step(pos, c->h_init2[0], c->h_init2[1], st);
            for (int i = 0; i < nmain; ++i) enqueue_steps(1, false);
        }
    }
    if (step_rc) { fence_out(c, caller); return -1; }        // c->err was set by the step builder
    HIPCHK(c, hipEventRecord(c->ev_t2, st));
    HIPCHK(c, hipMemcpyAsync(out_tokens, c->tok_out.p, (size_t)B * n_new * 4, hipMemcpyDeviceToDevice, st));
    fence_out(c, caller);
    HIPCHK(c, hipGetLastError());
    // stats inputs (algorithmic bytes are computed in car_get_stats, which synchronises anyway: DESIGN.md §4 / SURVEY.md §8d)
    {
        c->stats.decode_steps = nsteps;
        c->stats.decode_kernels_per_step = c->n_dec_kernels;
        const double we = (mode == CAR_BF16 && g.decode_weight_fp8) ? 1.0 : (double)e;      // fp8 decode weights: 1 B/param (+ fp32 row scales)
        c->st_wbytes = ((double)g.n_layer * ((double)3 * D * D + (double)D * D + 3.0 * (double)Fh * D) + (double)V * D) * we
                       + ((double)g.n_layer * 2.0 * D + D) * (double)e
                       + ((mode == CAR_BF16 && g.decode_weight_fp8) ? 4.0 * ((double)g.n_layer * (5.0 * D + 2.0 * Fh) + V) : 0.0);
        c->st_b = b; c->st_T = T; c->st_nsteps = nsteps; c->st_has_mask = emb_mask ? 1 : 0; c->st_jmin = jmin;
    }
    return 0;
}
