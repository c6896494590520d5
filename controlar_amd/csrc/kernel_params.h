// kernel_params.h — parameter blocks of the kernels in ops.hip / attn.hip, shared with their callers (engine_*.hip): ONE definition each
// (the engine used to keep hand-synchronised copies).  decode2.hip's blocks live in decode2_params.h.
#pragma once
#include "car_common.h"

// ------------------------------------------------------------------ RMSNorm with optional token gather and control add
// reference: gpt_t2i.py:193-198 (norm), :445 (tok_embeddings gather), :463/:466 (control add)
//   row r:  v = gather ? emb[idx[r]] : h_in[r]
//           parts: v = rnd(v + rnd(sum_s parts[s][r]))   (residual add of a dec_linear output, decode fast path)
//           add_mode 1 (decode):  v = rnd(v + rnd(cs * ctrl[r, *pos - T + 1]))
//           add_mode 2 (prefill): same with control token 0, only on rows r % T == T-1 (ctrl batch = r / T)
//           add_mode 3 (score):   same with control token j = r % T - row0 on every row with j >= 0 (sequences of T rows: a window of the prefix, then
//                                 the image tokens; row0 = the last prefix row; ctrl batch = r / T) — all positions of car_score's one pass
//           h_out[r] = v (if h_out);  xn[r] = rnd(rnd(v * rsqrt(mean(v^2)+eps)) * w)
struct NormP {
    const void* h_in; const void* emb; const int* idx; void* h_out; void* xn; const void* w;
    const void* ctrl; const int* pos; int add_mode; int T; int n_tok; float cs;
    int D; float eps;
    const float* parts; int parts_ks; long parts_stride;   // residual branch as fp32 split-K partials [ks][rows][D] of dec_linear
    int row0;                                              // add_mode 3
};

// ------------------------------------------------------------------ fused vocabulary projection + cross-entropy (score.hip; car_score)
// Output row r (an image position) takes its X row(s) from
//     xrow(r, u) = (r / rows_per_seq) * seq_stride + row_off + r % rows_per_seq + u * unc_off        (u = 1: the unconditional row of a CFG pair)
// logit[r][n] = x[xrow(r, 0)] . w[n]  (rounded to bf16 if round_bf16), and with `paired`
//     logit[r][n] = s == 1 ? c : u + (c - u) * s,   s = scale ? scale[r] : (cfg_interval > -1 && r % rows_per_seq - 1 > cfg_interval ? 1 : cfg_scale)
// The kernel leaves per row and per vocabulary part (max, sum of exp(logit - max), the target's logit or 0) in `part` [nparts][R][4]; score_fold_kernel
// folds the parts in index order: nll[r] = max + log(sum) - logit[r][targets[r]].  logits (optional) [R][V] fp32 takes the same accumulators.
struct ScoreP {
    const void* x; const void* w; const int* targets; const float* scale;
    float* part; float* logits;
    long ldx, seq_stride, row_off, unc_off;
    int R, V, D, rows_per_seq;
    int paired, round_bf16, cfg_interval; float cfg_scale;
    int nsplit, tiles_per_split;                           // vocabulary tiles (128 columns) per grid.y slice
};

struct SampleDyn { unsigned long long seed; float temperature; int top_k; float top_p; int pad; };
// The device image of car_sampling_row (include/controlar_hip.h): one entry per image of a row-mode call, uploaded as the caller wrote it.
struct SampleRow {
    float cfg_scale; int cfg_interval; float temperature; int top_k; float top_p; int sample_logits;
    unsigned long long seed; float control_strength; unsigned rng_stream;
};
static_assert(sizeof(SampleRow) == 40, "SampleRow mirrors car_sampling_row");

// ------------------------------------------------------------------ CFG mix + greedy argmax (generate.py:90,105; :59-74 greedy branch)
// logits fp32 [b, V] (cond rows [0,B), uncond rows [B,2B)).  One block per image.
//   mixed = use_mix ? u + (c - u) * scale : c;  token = lowest index of the maximum (torch.topk tie rule)
// writes: out_tokens[i*n_new + step], cur_tok[i] (and cur_tok[B+i] under CFG) = forced ? forced[i*n_new+step] : token,
// optional logits_out[(i*n_new + step)*V + :] = mixed.
struct SampleP {
    const float* logits; int B, V, use_cfg; float cfg_scale; int cfg_interval;
    const int* step_ptr; int n_new; int* out_tokens; int* cur_tok; const int* forced; float* logits_out;
    int logits_ks; long logits_stride; int round_bf16;   // logits given as split-K partials [ks][b][V]; bf16 rounding of the sum (gpt_t2i.py:470)
    int stochastic; float temperature; int top_k; float top_p; unsigned long long seed; int row0;   // sample_logits=True path (generate.py:59-74)
    const struct SampleDyn* dyn;    // when set, (seed, temperature, top_k, top_p) are read from device memory: a captured graph stays valid across calls
    const struct SampleRow* rows;   // row mode (device pointer, one entry per image of this launch): block i takes cfg_scale, cfg_interval, temperature, top_k, top_p,
                                    // seed and greedy-or-stochastic from rows[i], and draws at the Philox counter (row0 + rows[i].rng_stream, step) instead of (row0 + i, step)
    int mix_step0;                  // added to *step_ptr in the cfg_interval test only (car_sample_logits: the device step is 0, the caller's step arrives here)
};

struct FlashP {
    const bf16_t* q; const bf16_t* k; const bf16_t* vt; bf16_t* o;
    long q_sb, q_st, k_sb, k_st;      // batch / token strides in elements; head h starts at column h*64
    long vt_sb; int vt_ld;            // V^T [b][h*64 + d][vt_ld] (keys zero padded to a multiple of 32)
    long o_sb, o_st;
    int Tq, Tk, H;
    float scale;
    int mode;                         // 0 none | 1 causal + pad mask: key j allowed iff j <= i and (mask[b][j] or j == i) | 2 bias + key mask (T5)
    const unsigned char* mask;        // [b][Tk]
    const float* bias;                // [H][Tq][Tk]
};

// ------------------------------------------------------------------ LineArt extractor (lineart.hip; condition/lineart.py:26-86)
// One implicit-GEMM convolution launch: GEMM rows = the Hg x Wg grid of ONE image (blockIdx.z), row (gy, gx) reads input pixel
// (gy*stride + dy[t], gx*stride + dx[t]) for tap t — reflected at the border (reflect = 1) or zero outside it — and lands at output pixel
// (gy*os + py, gx*os + px): os = 2 with a parity (py, px) is one phase of a transposed convolution.  k = t*Cin + ci, weights [N][Kp].
struct LaConvP {
    const void* in; const void* w; float* raw; float* part; int* cnt;
    long in_img, raw_img;             // per-image element strides of `in` / `raw`
    int Hi, Wi, Cin, N, K, Kp;
    int Hg, Wg, Hout, Wout;
    int stride, os, py, px, reflect, ntaps;
    int tile0, tiles_img;             // first InstanceNorm partial slot of this launch; partial slots per image
    signed char dy[49], dx[49];
};

// ------------------------------------------------------------------ HED extractor (hed.hip; condition/hed.py:17-81)
// One 3x3 / stride 1 / zero-padded convolution launch as an implicit GEMM: rows = the H x W grid of ONE image (blockIdx.z), k = tap*Cin + ci,
// weights [N][Kp].  pool = 1: the stored input map is Hi x Wi and the conv reads it through a 2x2 / stride-2 max-pool (H = Hi/2, W = Wi/2, floor).
// part != NULL: the block's 1x1 side projection is taken in the epilogue — fp32 partial per 64-channel block at part[img*part_img + nblk*H*W + pixel].
struct HedConvP {
    const void* in; const void* w; const float* bias; void* out;
    const void* proj; float* part;
    long in_img, out_img, part_img;   // per-image element strides
    int Hi, Wi, H, W;
    int Cin, N, K, Kp, pool;
};

// Fusion of the five side maps (level l is (H >> l) x (W >> l), nblk[l] channel-block partials + bias): bilinear up-sampling, mean, sigmoid, x255.
struct HedFuseP {
    const float* part[5]; const float* bias[5];
    long part_img[5]; int nblk[5];
    float* out; void* control;        // fp32 [nimg][H*W]; T [nimg][3][H*W]
    int H, W;
};

// ------------------------------------------------------------------ DPT depth estimator (dpt.hip; transformers modeling_dpt.py neck + head)
// One 3x3 / zero-padded (pad 1) convolution launch as an implicit GEMM: rows = the H x W output grid of ONE image (blockIdx.z), k = tap*Cin + ci
// (Cin a multiple of 32), weights [N][9*Cin], N a multiple of 4 (partial 64-channel tiles are masked).  stride 1: H = Hi, W = Wi; stride 2:
// H = (Hi-1)/2 + 1, likewise W.  relu_in: the gather reads max(x, 0) (the pre-activation of a residual conv unit).  Epilogue, in this order:
// + bias (optional), + res1, + res2 (optional NHWC maps of the output's shape), ReLU (relu_out), round to T, store (out may be NULL with proj).
// proj != NULL (N <= 64): the T-rounded channels are reduced against proj[N] in fp32, + proj_bias[0], ReLU -> map[img*map_img + pixel] (fp32).
struct DptConvP {
    const void* in; const void* w; const float* bias; void* out;
    const void* res1; const void* res2;
    const void* proj; const float* proj_bias; float* map;
    long in_img, out_img, res1_img, res2_img, map_img;   // per-image element strides
    int Hi, Wi, H, W;
    int Cin, N, K, stride, relu_in, relu_out;
};

// ------------------------------------------------------------------ Pillow-exact 8-bit resampler (resample.hip; ImagingResample for modes L / RGB)
// One pass over uint8 rows of `row_bytes` = width * C interleaved bytes; a thread owns 4 consecutive bytes of one output row.
//   pass 0 (horizontal): output row r is source row src_y0 + r; byte e = x*C + c sums source pixels bounds[2x] .. +bounds[2x+1] of channel c with kk[x][*]
//   pass 1 (vertical):   output row r sums source rows bounds[2r] .. +bounds[2r+1] with kk[r][*]; `src` starts at image row src_y0
//   pass 2 (copy):       output row r is source row r
// Each sum is (1 << 21) + sum(pixel * k) in int32, shifted right by 22 (arithmetic) and clamped to 0..255.
// final = 0: the bytes go to `tmp` (row pitch tmp_pitch, a multiple of 4; the pad bytes are written as 0).  final = 1: to out (dense [B][rows][row_bytes])
// and / or control (T [B][3][rows][Wo] = 2*(v/255 - 0.5), C = 1 replicated) and / or fout (fp32 [B][C][rows][Wo]: norm 0 raw, norm 1 = 2*(v/255 - 0.5)).
struct ResampleP {
    const unsigned char* src; long src_img; int src_pitch, src_y0, src_aligned;   // src_aligned: base, pitch and image stride are multiples of 4
    const int* kk; const int* bounds; int ksize;
    int B, C, rows, row_bytes, nq;                                                // nq = quads per output row
    unsigned char* tmp; long tmp_img; int tmp_pitch;
    unsigned char* out; void* control; float* fout; int norm, Wo, final;
};

// ------------------------------------------------------------------ CLIP score (clip.hip; evaluations/t2i/evaluation.py:129-176)
// clip_pixels_to_patches: the tail of CLIP's preprocessor on the uint8 [B][Hr][Wr][3] output of the bicubic resize.  Pixel (y, x) of the n_px x n_px
// centre crop is source pixel (top + y, left + x); its value is v = ((u / 255) - mean[c]) / std[c], every step rounded to fp32 once (correctly rounded
// divisions, no contraction).  v goes to patches[(b*g*g + (y/patch)*g + x/patch)][c*patch*patch + (y%patch)*patch + x%patch] (row pitch Kp, the columns
// [3*patch*patch, Kp) written as 0) in the element type, and to pixel_values [B][3][n_px][n_px] fp32 when that is given.
struct ClipPatchP {
    const unsigned char* src; void* patches; float* pixel_values;
    int B, Hr, Wr, top, left, n_px, patch, g, Kp;
    float mean[3], std[3];
};
