/*
 * controlar_hip.h — C ABI of libcontrolar_hip.so: the MI355X (gfx950) implementation of
 * ControlAR's conditional-decoding hot path
 *     DINOv2 control encoder -> LlamaGen AR decode with per-token control fusion -> VQGAN decoder.
 *
 * The reference (hustvl/ControlAR) has no FFI/plugin layer: its seams are Python callables
 * (SURVEY.md §8b).  Each entry point below replaces one of those callables; the ctypes binding
 * that a reference maintainer would add is shown in INTEGRATION.md and shipped in
 * controlar_amd/_lib.py.  No torch types cross this boundary: plain pointers, sizes, ints.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; car_last_error(ctx) gives the text
 *     (reference raises Python exceptions / asserts: generate.py:173,185-186; gpt_t2i.py:229).
 *   - all data pointers are DEVICE pointers unless stated; the caller (PyTorch) owns inputs and
 *     outputs; the library owns packed weights, KV caches, control-token buffers, hipGraphs and
 *     workspaces (SURVEY.md §8b "Ownership").
 *   - work is enqueued on the hipStream_t passed as `stream` (void* so the header needs no HIP
 *     include); functions that return values to the HOST say so and synchronise that stream.
 *   - a context is re-entrant per ctx but not thread-safe within one ctx.
 */
#ifndef CONTROLAR_HIP_H
#define CONTROLAR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAR_ABI_VERSION 2      /* 2: car_stats.dev_knobs_active, car_check_errors, car_sampling.first_valid_hint (round 4-5) */

/* arithmetic mode of a context */
enum { CAR_F32 = 0,   /* "exact" mode: fp32 weights/activations/FMA — parity contract vs the fp32 CPU reference */
       CAR_BF16 = 1   /* fast mode: bf16 storage, fp32 accumulate, the reference's bf16 rounding points */ };

/* element types accepted by car_load_tensor / image inputs */
enum { CAR_DT_F32 = 0, CAR_DT_BF16 = 1, CAR_DT_I32 = 2, CAR_DT_I64 = 3, CAR_DT_U8 = 4 };

/* resize in front of the encoder — reference: autoregressive/models/dinov2_adapter.py:16-24 */
enum { CAR_RESIZE_NEAREST = 0,          /* condition_type in {'canny','seg'} */
       CAR_RESIZE_BICUBIC_AC = 1 };     /* everything else: bicubic, align_corners=True */

typedef struct car_config {
    int32_t abi_version;      /* = CAR_ABI_VERSION */
    int32_t mode;             /* CAR_F32 | CAR_BF16 */
    /* LlamaGen transformer — reference: autoregressive/models/gpt_t2i.py:31-60 ModelArgs */
    int32_t dim, n_layer, n_head, ffn_hidden, vocab_size;
    int32_t cls_token_num;    /* text prefix length T (120) */
    int32_t block_size;       /* rope grid = sqrt(block_size)  (gpt_t2i.py:351-353) */
    int32_t caption_dim;      /* 2048 */
    float   norm_eps;         /* 1e-5 */
    float   rope_base;        /* 10000 */
    /* control encoder — HF Dinov2Config as built by dinov2_adapter.py:13 */
    int32_t vit_hidden, vit_layers, vit_heads, vit_mlp, vit_patch, vit_pos_grid;
    float   vit_ln_eps;       /* 1e-6 */
    int32_t resize_mode;      /* CAR_RESIZE_* */
    /* VQGAN decoder — reference: tokenizer/tokenizer_image/vq_model.py:12-24,129-169 */
    int32_t codebook_size, codebook_dim, z_channels, vq_ch, vq_num_res_blocks;
    int32_t vq_n_mult;        /* number of entries used in vq_ch_mult (5 for VQ-16) */
    int32_t vq_ch_mult[8];
    float   gn_eps;           /* 1e-6 */
    int32_t vit_variant;      /* 0 = HF Dinov2Model (t2i; LayerScale, patch-14 resize)   1 = HF ViTModel (c2i: gpt.py:319, vit_adapter.py:11-15) */
    int32_t model_type;       /* 0 = t2i (gpt_t2i.py)   1 = c2i (gpt.py: class-label prefix of length 1) */
    int32_t num_classes;      /* c2i: LabelEmbedder rows = num_classes + 1, CFG null class = num_classes (gpt.py:66-96) */
    int32_t stream_priority;  /* priority of the context's internal HIP streams: 0 default, 1 lowest, 2 highest (overlapping a
                                 compute-bound context with a latency-bound one on the same GPU) */
    int32_t decode_weight_fp8; /* CAR_BF16 only: the five decode linears (wqkv, wo, w1|w3, w2, output) stream OCP e4m3fn weights with
                                  per-output-row fp32 scales (BASELINE config 5).  1 = weight-only: bytes widened to bf16 in registers, bf16 MFMA.
                                  2 = W8A8: activations quantised to e4m3 (unit scale, clamped to +-448) in registers and multiplied on the
                                  fp8 MFMA (v_mfma_f32_16x16x32_fp8_fp8).  The reference has no fp8 path: tolerance-graded only. */
    int32_t kv_cache_fp8;     /* CAR_BF16 only, opt-in (0 = bf16 KV cache: the default and the parity path).  1 = the KV cache holds OCP e4m3fn bytes, unit scale:
                                  rotated K and V are rounded to e4m3 when they are stored, widened to bf16 in registers in front of the same bf16 MFMAs; the
                                  prefill's own attention reads the unrounded rows.  Halves the dominant HBM stream of large batches and doubles the sequences
                                  that fit.  The reference has no such mode: tolerance-graded against the oracle running the same model (kv_fp8=True). */
    int32_t vq_split_bf16;    /* CAR_F32 only, opt-in (0 = the default: every GEMM-shaped layer of car_vq_decode on the exact fp32 MFMA).  1 = the decoder's convolutions
                                  (3x3, 1x1) and the AttnBlock's two batched GEMMs take each fp32 operand as two bf16 numbers, hi = bf16(x) and lo = bf16(x - hi), and
                                  a product as three bf16 MFMAs accumulating in fp32 (hi*hi + hi*lo + lo*hi; relative product error about 2^-16) wherever a layer's
                                  K and channel count are multiples of 32; a layer that is not runs exact fp32 as with 0.  Activations, GroupNorm, softmax, the codebook
                                  lookup and conv_out stay fp32; car_vq_encode and the transformer never use it.  Stands for the fp32 convolutions of
                                  tokenizer/tokenizer_image/vq_model.py:53-56,129-195.  The reference has no such arithmetic: held to the exact decoder's own tolerance
                                  against the reference's pixels, max <= 2e-3 and mean <= 1e-4 (tests/test_vq_split_gpu.py; profiles/vq_split_parity_measured.jsonl) */
    int32_t reserved[1];
} car_config;

/* sampling parameters — reference: generate.py:59-74 sample(), :134 generate() kwargs */
typedef struct car_sampling {
    float    cfg_scale;        /* > 1 doubles the batch (cond | uncond)           generate.py:156-164 */
    int32_t  cfg_interval;     /* -1 = always mix                                  generate.py:121-122 */
    float    temperature;      /* logits / max(T,1e-5)                             generate.py:60 */
    int32_t  top_k;            /* 0 = off                                          generate.py:33-38 */
    float    top_p;            /* 1 = off                                          generate.py:40-55 */
    int32_t  sample_logits;    /* 0 = greedy topk(probs,1): ties -> lowest index   generate.py:71-73 */
    uint64_t seed;             /* counter-based RNG seed when sample_logits != 0 */
    float    control_strength; /* ignored (=1) when cfg_scale <= 1                 generate.py:87-92 */
    int32_t  first_valid_hint; /* 0 = unknown.  Otherwise 1 + a LOWER bound of the first attendable position over all prompts of the call (left-padded captions,
                                  sample_t2i.py:146-160): T - longest valid length, known to a caller that built the mask on the host.  With it car_generate sizes the
                                  prefill window without reading the device mask back — no host wait, the call only enqueues (every per-call scalar is a kernel argument;
                                  capturing the CALLER's stream around the call is not a tested configuration: the work runs on the library's own stream).  Too
                                  small a value only costs time; a value beyond the true minimum would drop valid prompt rows: it is checked on the device and
                                  raises the sticky error flag (car_check_errors). */
    int32_t  reserved[3];
} car_sampling;

/* sampling parameters of ONE image of a batch: the per-request form of the fields above, for the *_rows entry points below (40 bytes).  Every image carries
 * its own parameters and its own RNG stream, so its result is a function of its own row alone: it does not change with the slot it occupies, with the
 * requests beside it, or with the rank a shard of the batch runs on — in the CAR_F32 mode bit for bit (that mode is batch-invariant by construction). */
typedef struct car_sampling_row {
    float    cfg_scale;        /* the rows of one call are all > 1 or all <= 1: the CFG batch doubling is call-wide */
    int32_t  cfg_interval;
    float    temperature;
    int32_t  top_k;            /* >= 0 */
    float    top_p;            /* in (0, 1] */
    int32_t  sample_logits;    /* greedy and stochastic rows may share a call */
    uint64_t seed;
    float    control_strength; /* ignored (= 1) when the call is not under CFG, and in c2i */
    uint32_t rng_stream;       /* first word of this image's Philox counter: (rng_stream, step).  The plain entry points use the image's index in the batch; a
                                  request that is to be replayed, re-batched or moved to another rank keeps one value (0 is fine: the seed tells requests apart) */
} car_sampling_row;

typedef struct car_ctx car_ctx;

/* lifecycle */
int  car_create(car_ctx** out, const car_config* cfg);
void car_destroy(car_ctx* ctx);
const char* car_last_error(const car_ctx* ctx);   /* also valid with ctx == NULL after a failed car_create */
int  car_abi_version(void);
const char* car_build_id(void);                   /* hash of the library sources: packed-weight cache files are valid for ONE build */

/*
 * Weight loading — keyed by the reference state_dict names (SURVEY.md §8b "Weight contract"):
 * gpt_t2i.Transformer / gpt.Transformer names (incl. HF Dinov2 / ViT under "adapter.model.", 4.x and 5.x key spellings)
 * and VQModel names (decoder.*, post_quant_conv.*, quantize.embedding.weight; encoder.* + quant_conv.* enable car_vq_encode).
 * `ptr` may be a host or device pointer; dtype CAR_DT_F32 or CAR_DT_BF16; shape row-major.
 * Reference tensors that inference never reads (condition_embeddings.weight, *.mask_token, pooler.*, condition_norm.weight,
 * quantize.codebook_used) are accepted and ignored.  Tensors are packed as they arrive (MFMA-fragment images of the decode
 * linears, w1|w3 interleave, implicit-GEMM conv layouts, optional e4m3 quantisation);
 * car_finalize_weights checks that every tensor the loaded model halves need has arrived.
 */
int car_load_tensor(car_ctx* ctx, const char* name, const void* ptr, const int64_t* shape, int32_t ndim, int32_t dtype);
int car_finalize_weights(car_ctx* ctx);

/*
 * Packed-weight cache — the start-up cost of sample_t2i.py:64-83 / demo/model.py:66-75 (checkpoints re-read and re-loaded on every
 * start, in the demo on every request).  car_export_packed writes every weight image of a FINALISED context (row-major
 * operands, MFMA-fragment / e4m3 decode images, scales, conv layouts, host tables) to `path`; car_import_packed restores them
 * by plain copies into a context created with the same car_config and finalises it.  The file is only valid for this
 * library build (magic + car_config are checked); keying it on the checkpoint content is the caller's job
 * (controlar_amd/checkpoint.py).
 */
int car_export_packed(car_ctx* ctx, const char* path);
int car_import_packed(car_ctx* ctx, const char* path);

/*
 * Control encoder + adapter MLP — replaces model.adapter(condition) + model.adapter_mlp(...)
 * (generate.py:136-138; dinov2_adapter.py:26-29).  img: [B,3,H,W] in [-1,1], dtype F32/BF16.
 * out (optional, may be NULL): [B,(H/16)(W/16),dim] in the context's element type; the result is
 * always kept inside the context for the next car_generate call.
 */
int car_encode_control(car_ctx* ctx, const void* img, int32_t img_dtype, int32_t B, int32_t H, int32_t W,
                       void* out, void* stream);

/*
 * generate() — replaces autoregressive/models/generate.py:134-204 (t2i branch).
 *   text_emb  [B,T,caption_dim] (F32/BF16 per text_dtype), emb_mask [B,T] int64 (may be NULL),
 *   n_new     = max_new_tokens <= block_size (RoPE is indexed linearly on the sqrt(block_size)-wide grid exactly as the
 *               reference does, gpt_t2i.py:454 — also for non-square token grids, sample_t2i_MR.py:73-78,182-185),
 *   use_control != 0 consumes the control tokens of the preceding car_encode_control (same B, >= n_new tokens),
 *   out_tokens [B,n_new] int32 (device).
 * Debug/teacher-forcing extras (tests): forced_tokens [B,n_new] int32 or NULL
 * (token fed back at step i is forced[i]); logits_out [B,n_new,vocab] fp32 or NULL (post-CFG logits
 * handed to sample()).
 * Host waits: none inside the token loop.  With a text-pad mask the call reads ONE int (the earliest attendable text position of the batch) back from
 * the device before it enqueues the prefill, so that the prefill runs on the valid tail of the left-padded prefix only (result-preserving: pad rows
 * influence nothing that is returned; exact-mode tokens unchanged) — it therefore waits for the producers of emb_mask on `stream`.
 */
int car_generate(car_ctx* ctx, const void* text_emb, int32_t text_dtype, const int64_t* emb_mask,
                 int32_t B, int32_t n_new, int32_t use_control, const car_sampling* sp,
                 int32_t* out_tokens, const int32_t* forced_tokens, float* logits_out, void* stream);

/*
 * score() — the per-token negative log-likelihood of GIVEN image tokens under a prompt and a control map, in one parallel pass: the `targets` branch of
 * Transformer.forward (gpt_t2i.py:420-431,456-459,472-481) with generate()'s inference conventions.  Inputs mean what they mean to car_generate
 * (text_emb, emb_mask: left-padded, folded into the causal mask, fully padded rows attend to themselves; use_control consumes the preceding
 * car_encode_control; the prefill window on the valid tail, with the same single host read unless first_valid_hint is given).
 *   tokens     [B,n_new] int32 (device): the sequence to score
 *   nll_out    [B,n_new] fp32: logsumexp(l_i) - l_i[tokens[:,i]], where l_i is the fp32 logits row generate() hands to sample() at step i after feeding
 *              back tokens[:, :i] — after the CFG mix uncond + (cond - uncond) * cfg_scale when cfg_scale > 1, with cfg_interval dropping the mix from
 *              step cfg_interval + 2 on as the token loop does, before temperature / top-k / top-p
 *   logits_out optional [B,n_new,vocab] fp32: the same l_i (the very accumulators nll_out was reduced from)
 * Of `sp` only cfg_scale, cfg_interval, control_strength (ignored when cfg_scale <= 1, generate.py:87-92) and first_valid_hint are read.  No KV cache is
 * written and nothing a later car_generate depends on is changed.  Images are scored in fixed chunks (engine_score.hip): a sequence scored alone returns
 * the bits of its slice of a batch, in both modes.  Deterministic (no atomics).  A token id outside [0, vocab) cannot fail this call (no host
 * read-back): it is read as token 0 and raises the sticky error flag, reported by the next entry on the context or by car_check_errors, as for the
 * class labels of the c2i model.  c2i contexts are refused.
 */
int car_score(car_ctx* ctx, const void* text_emb, int32_t text_dtype, const int64_t* emb_mask,
              int32_t B, int32_t n_new, int32_t use_control, const car_sampling* sp,
              const int32_t* tokens, float* nll_out, float* logits_out, void* stream);

/*
 * Canny control extraction — replaces CannyDetector.__call__ = cv2.Canny(img, low, high) (condition/canny.py:6-14; callers
 * sample_t2i.py:123-125, sample_t2i_MR.py:139, demo 'Canny' preprocessor).  img: uint8 [B,H,W,3] (device).  edges_out: uint8 [B,H,W]
 * in {0,255} or NULL; control_out: [B,3,H,W] in the context's element type, = 2*(edges/255 - 0.5) replicated over 3 channels
 * (sample_t2i.py:125,141), or NULL.  Integer arithmetic of opencv-python 4.9 (Sobel 3x3, L1 magnitude, fixed-point direction test,
 * hysteresis); works on any context (no weights needed).  Synchronises `stream` internally (hysteresis fixed point).
 */
int car_canny(car_ctx* ctx, const uint8_t* img_hwc, int32_t B, int32_t H, int32_t W, float low_threshold, float high_threshold,
              uint8_t* edges_out, void* control_out, void* stream);

/*
 * Image resize — replaces PIL's Image.resize(size, resample, box) on 8-bit images in front of every extractor (sample_t2i_MR.py:37-49,
 * dataset/augmentation.py:8-26 center_crop_arr, sample_t2i.py:135 DPTImageProcessor, demo/model.py:127,221, condition/utils.py:28-38 resize_image).
 * img_hwc: uint8 [B,H,W,C] (device), interleaved as car_canny takes it, C = 1 (mode L) or 3 (mode RGB).  filter: Pillow's own codes, the CAR_FILTER_*
 * values below.  box: four floats x0, y0, x1, y1 on the HOST (the source region, 0 <= x0 < x1 <= W, 0 <= y0 < y1 <= H, fractions allowed) or NULL = the
 * whole image.  out_hwc: uint8 [B,Ho,Wo,C] or NULL.  control_out: [B,3,Ho,Wo] in the context's element type, = 2*(x/255 - 0.5), C = 1 replicated over
 * the three channels, ready for car_encode_control, or NULL.  float_out: fp32 [B,C,Ho,Wo] or NULL; norm 0: the raw value (float)x, what car_hed and
 * car_lineart take; norm 1: (x/255 - 0.5)/0.5, the pixel_values car_depth takes (the same bits as 2*(x/255 - 0.5)).  Not all three NULL.  Both float
 * tensors are evaluated in fp32 with a correctly rounded division and rounded once.
 * The arithmetic is Pillow's ImagingResample (checked against Pillow 12.2.0): per axis a table of fixed-point taps (22 fractional bits) computed on
 * the host in double, a horizontal pass into a uint8 intermediate — that rounding is part of the result — then a vertical pass, int32 sums; an
 * axis whose size stays and whose box spans it is skipped, and with both skipped the result is a copy.  Integer throughout, so out_hwc is
 * bit-identical to Pillow's for every filter, size and box.  One table pair serves the whole batch; the last pair stays in the context, keyed by
 * (input size, box edges, output size, filter) per axis, and is uploaded on the stream when the key changes.  Works on any context (no weights
 * needed), deterministic, batch-invariant, no host synchronisation.  Refused, with the context left usable: all outputs NULL; C other than 1 or 3
 * (for 4 the message points at HWC3); a non-positive size or a side above 65536; NEAREST (Pillow takes another code path for it) or an unknown
 * filter; an empty box or one outside the image.  Out of scope: modes F, I and RGBA, NEAREST, and reducing_gap.
 */
enum { CAR_FILTER_LANCZOS = 1, CAR_FILTER_BILINEAR = 2, CAR_FILTER_BICUBIC = 3, CAR_FILTER_BOX = 4, CAR_FILTER_HAMMING = 5 };
int car_resize(car_ctx* ctx, const uint8_t* img_hwc, int32_t B, int32_t H, int32_t W, int32_t C,
               int32_t Ho, int32_t Wo, int32_t filter, const float* box /* x0,y0,x1,y1 or NULL = whole image */,
               uint8_t* out_hwc, void* control_out, float* float_out, int32_t norm, void* stream);

/*
 * Control-consistency metrics — replace the scoring of evaluations/hed_ssim.py, lineart_ssim.py, canny_f1score.py, depth_rmse.py and the accumulators of
 * autoregressive/test/metric.py (torchmetrics / sklearn on saved PNGs) on tensors that are already on the device.  All four entries work on any
 * context (no weights needed), are deterministic (no atomics: per-block partials folded per image in a fixed order), batch-invariant per image, and do
 * not synchronise with the host.  Element types are the CAR_DT_* codes; metric inputs are CAR_DT_F32 or CAR_DT_U8.  Results are fp64: every sum is
 * accumulated in fp64 on the device.  A refused call leaves the context usable.
 *
 * Multi-scale SSIM — torchmetrics' MultiScaleStructuralSimilarityIndexMeasure(data_range=1.0) with its defaults (11 x 11 Gaussian window, sigma 1.5,
 * k1 0.01, k2 0.03, betas 0.0448 0.2856 0.3001 0.2363 0.1333, relu normalisation).  pred, target: [B,C,H,W], each fp32 or uint8; the value of an
 * element is clip(v * scale, 0, 1) with that input's scale (1 for maps in 0..1, 1/255 for raw 0..255 maps, as the scripts divide and clip).  out: fp64
 * [B], the per-image value; scales_out: fp64 [B,5,2], per scale the means of the ssim and of the contrast-sensitivity map after relu, or NULL.  Both sides
 * must be at least 176 (torchmetrics refuses side / 16 <= 10).  Six launches: one per scale, which stages a halo tile of both images in LDS, filters the
 * five maps separably from there, reduces ssim and cs to one pair per tile and writes the 2 x 2-pooled images of the next scale; and one fold.
 */
int car_ms_ssim(car_ctx* ctx, const void* pred, int32_t pred_dtype, const void* target, int32_t target_dtype,
                int32_t B, int32_t C, int32_t H, int32_t W, double pred_scale, double target_scale,
                double* out, double* scales_out, void* stream);
/*
 * Binary F1 of two maps [B,H,W], each fp32 or uint8.  An element is positive by its map's rule: 0 = (v == value) (canny_f1score.py: == 255), 1 =
 * (v > value) (metric.py's F1score: > 128).  counts_out: int64 [B,3] = TP, FP, FN per image (FP: pred positive, target not), or NULL; f1_out: fp64 [B] =
 * 2 TP / (2 TP + FP + FN), 0 where the denominator is 0 (what torchmetrics and sklearn return), or NULL; not both NULL.  Integer partials: exact.
 */
int car_f1(car_ctx* ctx, const void* pred, int32_t pred_dtype, int32_t pred_rule, float pred_value,
           const void* target, int32_t target_dtype, int32_t target_rule, float target_value,
           int32_t B, int32_t H, int32_t W, int64_t* counts_out, double* f1_out, void* stream);
/*
 * RMSE per image: out[b] = sqrt(mean((pred * s - label)^2)), pred fp32 [B,H,W], label fp32 or uint8 [B,H,W], out fp64 [B].  scale_to_max 0: s = 1
 * (metric.py's RMSE); 1: s = 255 / max(pred[b]) (depth_rmse.py:59), the maximum from a reduction of its own.  An image whose pred is zero everywhere
 * gives NaN under scale_to_max, as the script does.
 */
int car_rmse(car_ctx* ctx, const float* pred, const void* label, int32_t label_dtype, int32_t B, int32_t H, int32_t W,
             int32_t scale_to_max, double* out, void* stream);
/*
 * The pixel quantiser of torchvision's save_image(normalize=True, value_range=(-1, 1)) as the reference writes its samples
 * (autoregressive/test/test_t2i.py:233-234): x fp32 [B,3,H,W] -> floor(clamp((clamp(x, -1, 1) + 1) / 2 * 255 + 0.5, 0, 255)), every step rounded to
 * fp32 as torch rounds it.  out_hwc: uint8 [B,H,W,3], what car_canny and car_resize take, or NULL; float_out: fp32 [B,3,H,W] with the same values
 * (raw 0..255), what car_hed and car_lineart take, or NULL; not both NULL.
 */
int car_pixels_to_u8(car_ctx* ctx, const float* x_nchw, int32_t B, int32_t H, int32_t W, uint8_t* out_hwc, float* float_out, void* stream);

/*
 * Reconstruction quality — what judges the pixel decoder and the tokenizer's round trip: the LPIPS distance the reference trains its tokenizer
 * against (tokenizer/tokenizer_image/lpips.py:83-96, vq_loss.py:93-95,124-125) and the PSNR and pixel quantiser of its tokenizer evaluation
 * (tokenizer/tokenizer_image/reconstruction_vq_ddp.py:128-155).  Deterministic (no atomics), batch-invariant per pair / image, no host synchronisation;
 * results are fp64.  A refused call leaves the context usable.
 *
 * car_lpips — LPIPS.forward in inference (dropout is the identity).  a_nchw, b_nchw: fp32 [B,3,H,W] in [-1,1] (device).  out: fp64 [B], the distance of
 * pair i; layers_out: fp64 [B,5], the five per-layer terms whose sum in the order 0..4 it is, or NULL.  Per image (x - shift) / scale (a subtraction
 * and a true division in fp32), the VGG-16 trunk (torchvision features[0:30], taps relu1_2 ... relu5_3) on the kernels of car_hed, per tap and pixel
 * x / (sqrt(sum_c x_c^2) + 1e-10) for both images, the 1x1 lin of the squared difference, the mean over H x W.  The context's mode sets the trunk's
 * arithmetic: bf16 operands and stored taps with fp32 accumulation, or fp32 throughout; the head is fp32 per pixel in both, every spatial sum and what
 * follows fp64.  The head takes the difference of the normalised features directly: identical inputs give exactly 0.0 in every layer, and
 * car_lpips(a, b) and car_lpips(b, a) are bit-equal.  Both sides at least 16 (four 2x2 pools), H * W at most 2^26.  Weights through car_load_tensor
 * under "lpips." + key, then car_finalize_weights (which names a missing tensor of a partly loaded family): the trunk as the LPIPS module spells it
 * (net.slice{1..5}.{0,2,5,7,10,12,14,17,19,21,24,26,28}.{weight,bias}) or as torchvision does (features.N.{weight,bias}; the LPIPS checkpoint holds
 * the lin layers only), lin{0..4}.model.1.weight [1,C,1,1], and optionally scaling_layer.shift / .scale [1,3,1,1] (otherwise (-.030, -.088, -.188)
 * and (.458, .448, .450)).  They travel in the packed cache and may sit next to any other model.
 */
int car_lpips(car_ctx* ctx, const float* a_nchw, const float* b_nchw, int32_t B, int32_t H, int32_t W,
              double* out, double* layers_out, void* stream);
/*
 * PSNR per image: out[i] = 10 log10(data_range^2 / mse), mse the fp64 mean of (a - b)^2 over the n elements of image i (skimage's
 * peak_signal_noise_ratio with an explicit data_range); equal images give +inf.  a, b: [B, n], each fp32 or uint8 (CAR_DT_*), read through its map,
 * every step rounded to fp32 once: 0 = v, 1 = v / 255 (the script's sample.astype(np.float32) / 255.), 2 = (v + 1) / 2 (its rgb_gt).  Any context.
 */
enum { CAR_PSNR_RAW = 0, CAR_PSNR_DIV255 = 1, CAR_PSNR_HALF = 2 };
int car_psnr(car_ctx* ctx, const void* a, int32_t a_dtype, int32_t a_map, const void* b, int32_t b_dtype, int32_t b_map,
             int32_t B, int64_t n, double data_range, double* out, void* stream);
/*
 * The tokenizer script's quantiser, torch.clamp(127.5 * x + 128.0, 0, 255).to(torch.uint8) (reconstruction_vq_ddp.py:144, val_ddp.py:138): a product
 * and a sum, each rounded to fp32, a clamp, a truncation — not save_image's rule (car_pixels_to_u8).  x: fp32 [n]; out: uint8 [n], same order.  Any context.
 */
int car_recon_to_u8(car_ctx* ctx, const float* x, int64_t n, uint8_t* out, void* stream);
/* host-only helpers (tests): the name car_load_tensor stores an "lpips." tensor under (0, or -1 for a name outside the network); the pairs one chunk of
 * car_lpips holds at H x W in a mode (its workspace rule), or -1. */
int car_debug_lpips_canonical_name(const char* name, char* out, int32_t cap);
int car_debug_lpips_chunk_pairs(int32_t mode, int32_t H, int32_t W);

/*
 * Sample quality — the statistics half of evaluations/c2i/evaluator.py (everything from compute_statistics down): the moments behind FID and sFID,
 * improved precision / recall, the Inception Score.  Inputs are activations [N, D] already on the device; the Inception tower that produces them
 * is not part of the library, and the Fréchet distance itself (one D^3 matrix square root per evaluation) is host code
 * (controlar_amd.metrics.frechet_distance).  No weights, any context; the context's mode changes no bit.  Deterministic: fixed summation orders, no
 * floating-point atomics.  A refused call leaves the context usable.
 *
 * Moments (compute_statistics, :186-189) as a running fp64 state the caller owns: car_fid_state_bytes(D) bytes of device memory (0 for a D outside
 * 1..16384), all zero = empty; fp64 [1 + 2D + D*D] = n | c [D] | sum(x - c) [D] | sum (x - c)(x - c)^T [D][D].  c is fixed by the first update as
 * that batch's column mean rounded to fp32; products accumulate on v_mfma_f64_16x16x4_f64 as one k-ordered chain over all updates.
 * car_fid_accumulate adds acts fp32 [n, D] (n >= 1).  car_fid_finalize writes mu fp64 [D] = np.mean(axis=0) and sigma fp64 [D, D] =
 * np.cov(rowvar=False) (ddof 1; exactly symmetric, written in full); it reads n back, so it waits for the stream, and refuses a state of fewer
 * than 2 rows.
 */
int64_t car_fid_state_bytes(int32_t D);
int car_fid_accumulate(car_ctx* ctx, const float* acts, int64_t n, int32_t D, void* state, void* stream);
int car_fid_finalize(car_ctx* ctx, const void* state, int32_t D, double* mu, double* sigma, void* stream);
/*
 * Precision and recall (ManifoldEstimator.manifold_radii / evaluate_pr over DistanceBlock, :260-293, :337-442, nhood_sizes = (k,), no percentile
 * clamp).  Squared distances are computed per (row batch x column batch) block in fp16 and, where a block's fp16 result is not all finite, again in
 * fp32 for that whole block (a device flag per block; no host round trip).  The fp16 arithmetic, which TensorFlow leaves to its backend, is defined
 * as: features rounded to fp16 (nearest even), D padded with zeros to a multiple of 32; nu, nv = fl16 of the fp32 sum of the fp16-rounded squares;
 * mm = fl16 of the v_mfma_f32_16x16x32_f16 product (exact products, fp32 accumulation); d = max(fl16(fl16(nu - fl16(2 mm)) + nv), 0), widened to
 * fp32.  The fp32 block: the same expression with one fp32 rounding per operation on v_mfma_f32_16x16x4_f32.  Nothing of size N x N is written.
 * car_manifold_radii: radii[i] = the (k+1)-th smallest of row i's N distances, its own included (0 <= k <= 7, k + 1 <= N).
 * car_manifold_pr: status1[i] = any_j d_ij <= r2[j], status2[j] = any_i d_ij <= r1[i] (uint8 0 / 1; d over rows of f1 and rows of f2),
 * pr = (mean status2, mean status1) = (precision, recall) when set 1 is the reference batch, as compute_prec_recall passes it.
 * row_batch, col_batch: the script's 10000 / 10000; they decide which distances share a fallback and nothing else.
 * car_debug_pairwise_distances (tests): one block's distances, out fp32 [n, m], and *used_fp32 (device int32) = 1 if the block fell back.
 */
int car_manifold_radii(car_ctx* ctx, const float* feats, int64_t N, int32_t D, int32_t k, int64_t row_batch, int64_t col_batch, float* radii, void* stream);
int car_manifold_pr(car_ctx* ctx, const float* f1, const float* r1, int64_t N1, const float* f2, const float* r2, int64_t N2, int32_t D,
                    int64_t row_batch, int64_t col_batch, uint8_t* status1, uint8_t* status2, double* pr, void* stream);
int car_debug_pairwise_distances(car_ctx* ctx, const float* U, int64_t n, const float* V, int64_t m, int32_t D, float* out, int32_t* used_fp32, void* stream);
/*
 * Inception Score (compute_inception_score, :191-204): p = softmax(acts . w) in fp32 (w fp32 [D, C], no bias: _create_softmax_graph), everything
 * behind p in fp64; per split of split_size rows exp(mean_rows sum_c p (log p - log mean_rows p)).  out fp64 [1 + ceil(N / split_size)]: the mean of
 * the splits, then every split.  A probability of exactly 0 gives NaN, as in the script.
 */
int car_inception_score(car_ctx* ctx, const float* acts, int64_t N, int32_t D, const float* w, int32_t C, int64_t split_size, double* out, void* stream);

/*
 * LineArt control extraction — replaces LineArt.forward (condition/lineart.py:26-86, default constructor: 3 residual blocks, sigmoid; callers
 * sample_t2i.py:110-113,129-132, sample_t2i_MR.py, autoregressive/test/test_t2i.py:177).  img_nchw: fp32 [B,3,H,W] (device), raw 0..255 values as the
 * reference receives them.  out: fp32 [B,1,Ho,Wo] in (0,1) or NULL; control_out: [B,3,Ho,Wo] in the context's element type, = 1 - 2*out replicated over
 * 3 channels (1 - y, *255, 2*(x/255 - 0.5) of sample_t2i.py:131-132,141), ready for car_encode_control, or NULL.  The output size is the network's own:
 * Ho = 4*ceil(ceil(H/2)/2), likewise Wo (30 x 44 in -> 32 x 44 out).  H or W below 5 is an error (the reference raises there).  The context's mode sets
 * the arithmetic: bf16 operands / fp32 accumulation and InstanceNorm statistics / bf16 activations, or fp32 throughout.  Weights: the 24 tensors of
 * LineArt().state_dict() through car_load_tensor under "lineart." + key (model0.1.weight ... model4.1.bias), then car_finalize_weights; a context may
 * hold them alone or next to a GPT / VQ / T5 model.  Deterministic (no atomics), batch-invariant per image, no host synchronisation.
 */
int car_lineart(car_ctx* ctx, const float* img_nchw, int32_t B, int32_t H, int32_t W,
                float* out, void* control_out, void* stream);

/*
 * HED edge extraction — replaces HEDdetector.__call__ (condition/hed.py:17-81: ControlNetHED_Apache2, bilinear up-sampling of the five side outputs,
 * mean, sigmoid, x255; callers sample_t2i.py:108-109,126-128, sample_t2i_MR.py, autoregressive/test/test_t2i.py:172-173, test_c2i.py,
 * evaluations/hed_ssim.py).  img_nchw: fp32 [B,3,H,W] (device), raw 0..255 values as the reference receives them.  out: fp32 [B,H,W] in 0..255 or NULL;
 * control_out: [B,3,H,W] in the context's element type, = 2*(out/255 - 0.5) replicated over 3 channels (sample_t2i.py:128,141), ready for
 * car_encode_control, or NULL; not both NULL.  H or W below 16 is an error (four 2x2 pools leave nothing; the reference raises there).  The context's
 * mode sets the arithmetic: bf16 operands and activations with fp32 accumulation, or fp32 throughout; side outputs, up-sampling and the sigmoid are
 * fp32 in both.  Weights: the 37 tensors of ControlNetHED_Apache2().state_dict() through car_load_tensor under "hed." + key (norm,
 * block1.convs.0.weight ... block5.projection.bias), then car_finalize_weights; a context may hold them alone or next to a GPT / VQ / T5 / LineArt
 * model.  Deterministic (no atomics), batch-invariant per image, no host synchronisation.
 */
int car_hed(car_ctx* ctx, const float* img_nchw, int32_t B, int32_t H, int32_t W,
            float* out, void* control_out, void* stream);

/*
 * DPT depth estimation — replaces DPTForDepthEstimation(pixel_values).predicted_depth and the scaling behind it (sample_t2i.py:33,114-116,133-139;
 * demo/model.py:192-284): a plain ViT backbone, the readout-"project" reassemble stage, the four-level fusion stage and the three-conv head of
 * transformers' modeling_dpt.py.  Configure once, load every tensor of DPTForDepthEstimation.state_dict() through car_load_tensor under
 * "depth." + key (depth.dpt.embeddings.cls_token, depth.dpt.encoder.layer.N.attention.attention.query.weight, depth.neck.reassemble_stage.*,
 * depth.neck.convs.N.weight, depth.neck.fusion_stage.layers.N.*, depth.head.head.{0,2,4}.*), then car_finalize_weights (which names the first
 * missing tensor).  depth.dpt.layernorm.* and depth.dpt.pooler.* never reach the depth map: they are accepted and ignored.  Any other "depth.*"
 * name is refused.  A context may hold these tensors alone or next to any other model; they travel in the packed cache (the importing context is
 * configured with the same car_dpt_config first).
 *
 * The family is the shipped one and nothing else: non-hybrid ViT with patch 16, qkv bias, erf-GELU, readout_type "project", reassemble factors
 * (4, 2, 1, 1/2), no batch norm in the fusion residual units, no add_projection, head_in_index -1.  car_depth_configure refuses what lies outside
 * it (sizes that are not multiples of 32, fewer or more than four taps, taps out of order or out of range, and in bf16 mode a head width other
 * than 64, which the fused attention kernel requires).
 */
typedef struct car_dpt_config {
    int32_t hidden;           /* 1024 (dpt_large) */
    int32_t layers;           /* 24 */
    int32_t heads;            /* 16 */
    int32_t mlp;              /* intermediate_size, 4096 */
    int32_t pos_grid;         /* image_size / 16 of the checkpoint: 24 */
    int32_t out_indices[4];   /* backbone_out_indices: 5, 11, 17, 23 */
    int32_t neck_hidden[4];   /* neck_hidden_sizes: 256, 512, 1024, 1024 */
    int32_t fusion_hidden;    /* 256 */
    float   ln_eps;           /* layer_norm_eps, 1e-12 */
    int32_t reserved[8];      /* zero */
} car_dpt_config;
int car_depth_configure(car_ctx* ctx, const car_dpt_config* cfg);
/*
 * pixel_values: fp32 [B,3,H,W] (device), exactly what the HF model receives after the image processor's rescale and normalise.  H == W, a
 * multiple of 32, at least 32: the reference itself raises on a non-square image (its reassemble stage takes sqrt of the token count), and an odd
 * token grid is out of scope; everything else is an error.  out: fp32 [B,H,W] = predicted_depth (>= 0) or NULL.  control_out: [B,3,H,W] in the
 * context's element type, = 2*(d/max_b - 0.5) replicated over 3 channels, ready for car_encode_control, or NULL; not both NULL.  max_b is the
 * maximum of image b alone: the reference takes .max() over a tensor that holds one image, and per image keeps the batch-invariance promise.  The
 * value is computed in fp32 (correctly rounded division) and rounded once to the element type.  An image whose map is zero everywhere writes -1
 * (the reference would write NaN).  The position embeddings are resized bilinearly (align_corners = False) in fp32 to the token grid of the call,
 * once per grid.  The context's mode sets the arithmetic: bf16 operands and activations with fp32 accumulation, or fp32 throughout; the final map
 * is fp32 in both.  Deterministic (no atomics), batch-invariant per image, no host synchronisation.
 */
int car_depth(car_ctx* ctx, const float* pixel_values, int32_t B, int32_t H, int32_t W,
              float* out, void* control_out, void* stream);

/*
 * Caption encoder — replaces T5Embedder.get_text_embeddings' model call (language/t5.py:185-201:
 * self.model(input_ids, attention_mask)['last_hidden_state'], HF T5EncoderModel built at language/t5.py:58-79; callers
 * sample_t2i.py:99-118, demo/model.py).  The tokenizer stays on the host side of the boundary (sentencepiece, CPU string work).
 * Configure once, load the encoder's tensors through car_load_tensor under the names "t5." + the HF state-dict key
 * (shared.weight, encoder.block.N.layer.0.SelfAttention.{q,k,v,o}.weight, ...relative_attention_bias.weight (block 0),
 * encoder.block.N.layer.0.layer_norm.weight, encoder.block.N.layer.1.DenseReluDense.{wi_0,wi_1,wo}.weight,
 * encoder.block.N.layer.1.layer_norm.weight, encoder.final_layer_norm.weight; encoder.embed_tokens.weight is the tied alias of
 * shared.weight and is ignored), then car_finalize_weights.  A context may hold the T5 encoder alone or next to a GPT / VQ model.
 */
typedef struct car_t5_config {
    int32_t vocab_size;       /* 32128 */
    int32_t d_model;          /* 2048 (Flan-T5-XL) */
    int32_t d_kv;             /* 64 */
    int32_t num_heads;        /* 32 */
    int32_t d_ff;             /* 5120 */
    int32_t num_layers;       /* 24 */
    int32_t rel_buckets;      /* relative_attention_num_buckets, 32 */
    int32_t rel_max_distance; /* relative_attention_max_distance, 128 */
    float   ln_eps;           /* layer_norm_epsilon, 1e-6 */
    int32_t reserved[7];
} car_t5_config;
int car_t5_configure(car_ctx* ctx, const car_t5_config* cfg);
/*
 * input_ids, attention_mask: int64 [B,T] (device or host; attention_mask may be NULL = all ones).  out: [B,T,d_model] in the
 * context's element type (device) = last_hidden_state (final_layer_norm applied; dropout is identity in eval).  Rows at padded
 * positions are computed exactly as HF computes them (only KEYS are masked).  feature_type "gated-gelu" (gelu_new) only — the
 * family the reference loads (flan-t5-xl, t5-v1_1-xxl).
 */
int car_t5_encode(car_ctx* ctx, const int64_t* input_ids, const int64_t* attention_mask, int32_t B, int32_t T, void* out, void* stream);

/*
 * CLIP score — replaces compute_clip_score (evaluations/t2i/evaluation.py:129-176: OpenAI clip.load, preprocess, encode_image, encode_text,
 * F.cosine_similarity, mean) on tensors that are already on the device.  The model is CLIP as HF transformers' CLIPModel evaluates it: a ViT with a
 * bias-free patch convolution, class token, learned positions, pre_layrnorm, pre-norm layers (LayerNorm, q/k/v/out projections with bias, scale
 * head_dim^-0.5, quick-GELU MLP), post_layernorm on the class row and visual_projection; a text transformer over token + position embeddings with the
 * same layer under a causal mask (no padding mask), final_layer_norm, the row at the first position of the largest token id and text_projection.
 * Configure once, load the tensors through car_load_tensor under "clip." + the HF state-dict key (text_model.embeddings.token_embedding.weight,
 * text_model.encoder.layers.N.self_attn.q_proj.weight, vision_model.pre_layrnorm.weight, visual_projection.weight, ...; logit_scale and *.position_ids
 * are accepted and ignored; any other "clip.*" name is refused), then car_finalize_weights, which names the first missing tensor.  A context may hold
 * CLIP alone or next to any other model; the tensors travel in the packed cache (the importing context is configured with the same car_clip_config
 * first).  car_clip_configure refuses a head width other than 64 in either tower (the fused attention kernel's; ViT-g/14's 88 is out of scope), an
 * image side that is no multiple of the patch, widths and MLP widths that are no multiples of 32 (the GEMMs' K step), and a context length above 128;
 * the context is left usable.
 */
typedef struct car_clip_config {
    int32_t vision_width;     /* 768 (ViT-B/32) */
    int32_t vision_layers;    /* 12 */
    int32_t vision_heads;     /* 12 */
    int32_t vision_mlp;       /* 3072 */
    int32_t image_size;       /* n_px, 224 */
    int32_t patch;            /* 32 */
    int32_t text_width;       /* 512 */
    int32_t text_layers;      /* 12 */
    int32_t text_heads;       /* 8 */
    int32_t text_mlp;         /* 2048 */
    int32_t vocab_size;       /* 49408 */
    int32_t context_length;   /* 77 */
    int32_t proj_dim;         /* 512 */
    float   ln_eps;           /* 1e-5 */
    int32_t reserved[10];     /* zero */
} car_clip_config;
int car_clip_configure(car_ctx* ctx, const car_clip_config* cfg);
/*
 * img_hwc_u8: uint8 [B,H,W,3] (device), e.g. the car_pixels_to_u8 output or the evaluation-resolution image.  In this order: with requant != 0 every
 * byte u goes through the script's ToTensor / Normalize(0.5, 0.5) / tensor2pil round trip, trunc(((u/255 - 0.5)/0.5 + 1) * 127.5) in fp32 (not the
 * identity: 63 of the 256 values change; the input is not modified, the library works on a copy); the short side is resized to image_size with Pillow's
 * BICUBIC (car_resize's arithmetic), the long side to int(image_size * long / short); the image_size x image_size centre is cropped with torchvision's
 * CenterCrop offset rule (round half to even); u/255, then (x - mean)/std with CLIP's constants, each step rounded to fp32 once; the tower.
 * out_emb: fp32 [B,proj_dim] (in CAR_BF16 mode the values are bf16-representable) or NULL; pixel_values_out: fp32 [B,3,image_size,image_size], what the
 * tower received before the rounding to the element type, or NULL; not both NULL.
 */
int car_clip_encode_image(car_ctx* ctx, const uint8_t* img_hwc_u8, int32_t B, int32_t H, int32_t W, int32_t requant,
                          float* out_emb, float* pixel_values_out, void* stream);
/* ids: int64 [B,T] (device), T <= context_length.  out_emb: fp32 [B,proj_dim].  An id outside [0, vocab) cannot fail this call (no host read-back): it
 * is read as token 0 and raises the sticky error flag, as car_score treats a bad token. */
int car_clip_encode_text(car_ctx* ctx, const int64_t* ids, int32_t B, int32_t T, float* out_emb, void* stream);
/* out_scores: fp32 [B] = F.cosine_similarity(img_emb, txt_emb, dim=1, eps=1e-8) of fp32 [B,proj_dim] inputs: each vector divided by max(its norm, eps), then
 * the dot product; fp32, one wave per pair, a fixed shuffle tree.  out_mean: fp64 [1] = the mean of the first n_mean scores (1 <= n_mean <= B), folded
 * by one block in a fixed order, or NULL.  Works on any context with a CLIP configuration.
 * All three entries are deterministic (no atomics), batch-invariant per row (fixed chunks of at most 16384 activation rows; no kernel lets a row depend on its chunk-mates), do
 * not synchronise with the host and leave the context usable after a refusal. */
int car_clip_score(car_ctx* ctx, const float* img_emb, const float* txt_emb, int32_t B, int32_t n_mean,
                   float* out_scores, double* out_mean, void* stream);

/*
 * generate() for the class-conditional model — replaces generate.py:134-204 (c2i branch :139-154) over
 * autoregressive/models/gpt.py.  labels [B] int64 (device).  Prefix length is 1; no pad mask; control_strength
 * does not exist on this path.  NOTE: in the reference snapshot this branch only runs with cfg_scale <= 1
 * (generate.py:88 passes control_strength, which gpt.py's forward does not accept); cfg_scale > 1 is
 * accepted here with the semantics generate.py:140-146 spells out (null class = num_classes).
 * Label range: labels live on the device and the entry never waits for the host, so a label outside [0, num_classes] cannot fail THIS call.
 * The device clamps it to the null class and raises a sticky error flag (host-mapped memory); the flag fails — with car_last_error naming this
 * entry — the next call on the context that runs after the offending kernel has executed: car_generate*, car_encode_control, car_vq_decode /
 * car_vq_encode, car_get_stats, or car_check_errors (which waits for the context's stream first: call it to validate the tokens right away).
 * The reporting call clears the flag.  (The reference's nn.Embedding fails asynchronously on a GPU as well.)
 */
int car_generate_c2i(car_ctx* ctx, const int64_t* labels, int32_t B, int32_t n_new, int32_t use_control, const car_sampling* sp,
                     int32_t* out_tokens, const int32_t* forced_tokens, float* logits_out, void* stream);

/*
 * sample() — autoregressive/models/generate.py:59-74 (with top_k_top_p_filtering :17-56) on caller-provided logits:
 * logits fp32 [rows, V] with rows = B, or 2B under CFG (cond rows then uncond rows, mixed as generate.py:105);
 * greedy (sample_logits = 0) or temperature / top-k / top-p / multinomial with a Philox counter RNG keyed by
 * (seed, image row, step).  out int32 [B] (device).  The same kernels run inside car_generate's token loop.  `step` is the index of the token being
 * sampled, as in that loop: with cfg_interval > -1 the mix is dropped where step - 1 > cfg_interval (generate.py:121-122).
 */
int car_sample_logits(car_ctx* ctx, const float* logits, int32_t B, int32_t V, const car_sampling* sp, int32_t step,
                      int32_t* out, void* stream);

/*
 * Per-request sampling parameters inside one batch: the four entries above with a row table behind `sp`.  rows: a HOST array of B car_sampling_row, one per
 * image, copied before the call returns.  With rows != NULL only the call-wide field of `sp` is read (first_valid_hint); with rows == NULL each is the
 * entry it is named after.  Image i mixes with its own cfg_scale and cfg_interval, filters with its own temperature / top_k / top_p, is greedy or stochastic
 * by its own sample_logits, and draws from Philox keyed by its own seed at counter (rng_stream, step); car_sample_logits_rows draws at
 * (step * 65536 + rng_stream, 0), as the plain entry does with the image index.  control_strength of image i scales its control tokens once, in the
 * element type, right after the condition layers (c' = rnd(cs_i * c), the product the plain call forms inside its kernels), and the passes then run at
 * strength 1; it is ignored where the plain call ignores it.  forced_tokens and logits_out work as in the plain calls; logits_out holds each image's own
 * mixed logits.  car_score_rows reads cfg_scale, cfg_interval and control_strength of each row.  The table lives in device memory that the captured decode
 * graph references: a second call with other values replays the graph.
 * Refused on the host, with the context left usable: rows that disagree about cfg_scale > 1 (the CFG batch doubling is call-wide, and u + (c - u) * 1 is
 * not c in fp32, so a row at scale 1 inside a CFG batch could not reproduce its plain call); top_k < 0; top_p outside (0, 1]; vocab_size > 32768 when any
 * row is stochastic.
 */
int car_generate_rows(car_ctx* ctx, const void* text_emb, int32_t text_dtype, const int64_t* emb_mask,
                      int32_t B, int32_t n_new, int32_t use_control, const car_sampling* sp, const car_sampling_row* rows,
                      int32_t* out_tokens, const int32_t* forced_tokens, float* logits_out, void* stream);
int car_generate_c2i_rows(car_ctx* ctx, const int64_t* labels, int32_t B, int32_t n_new, int32_t use_control, const car_sampling* sp,
                          const car_sampling_row* rows, int32_t* out_tokens, const int32_t* forced_tokens, float* logits_out, void* stream);
int car_score_rows(car_ctx* ctx, const void* text_emb, int32_t text_dtype, const int64_t* emb_mask,
                   int32_t B, int32_t n_new, int32_t use_control, const car_sampling* sp, const car_sampling_row* rows,
                   const int32_t* tokens, float* nll_out, float* logits_out, void* stream);
int car_sample_logits_rows(car_ctx* ctx, const float* logits, int32_t B, int32_t V, const car_sampling* sp, const car_sampling_row* rows,
                           int32_t step, int32_t* out, void* stream);

/*
 * VQModel.decode_code(code_b, [B,C,h,w], channel_first=True) — tokenizer/tokenizer_image/vq_model.py:53-56.
 * tokens [B,h*w] int32 -> out fp32 NCHW [B,3,16h,16w].
 */
int car_vq_decode(car_ctx* ctx, const int32_t* tokens, int32_t B, int32_t h, int32_t w, float* out_nchw, void* stream);

/*
 * VQModel.encode(x)[2][2] — tokenizer/tokenizer_image/vq_model.py:41-46 (Encoder :62-126, quant_conv :39, VectorQuantizer
 * arg-min :216-232): image fp32 NCHW [B,3,H,W] in [-1,1] -> min_encoding_indices int32 [B,(H/16)(W/16)] (device).
 * Needs the `encoder.*` and `quant_conv.*` tensors (the step on the other side of the tokenizer).
 */
int car_vq_encode(car_ctx* ctx, const float* img_nchw, int32_t B, int32_t H, int32_t W, int32_t* out_tokens, void* stream);

/* Introspection used by tests and bench.py */
typedef struct car_stats {
    double  decode_ms;          /* HIP-event time of the last car_generate's decode loop (n_new-1 steps) */
    double  prefill_ms;         /* prefill + control-token MLPs */
    int64_t decode_steps;
    int64_t decode_algo_bytes;  /* algorithmic HBM bytes of that loop (weights once/step + valid KV), DESIGN.md §4 */
    int32_t decode_kernels_per_step;
    int32_t graph_used;
    int32_t dev_knobs_active;   /* number of CAR_* environment variables set in this process: the library's A/B and profiling switches.  A
                                   measurement is only the benchmark when this is 0 — bench.py refuses to run otherwise */
    int32_t reserved[5];
} car_stats;
int car_get_stats(car_ctx* ctx, car_stats* out);

/* Waits for the work enqueued on the context, then reports (non-zero + car_last_error) and clears sticky device-side errors — see car_generate_c2i. */
int car_check_errors(car_ctx* ctx);

/* Host-only: the MFMA-fragment image of a decode linear W[N,K] (bf16 bits): chunk (rb,kb) = 64 lanes x 8 values, lane l holds
 * W[16rb + (l&15)][32kb + 8(l>>4) .. +8]; chunks ordered [rb][kb].  N % 16 == 0, K % 32 == 0. */
int car_debug_pack_decode_weight(const float* w, int32_t N, int32_t K, uint16_t* out);

/* Host-only: the coefficient table car_resize builds for one axis: input size, box edges in0 < in1 within [0, in_size], output size, filter.
 * *ksize_out = taps per output index; kk [out_size][ksize] fixed-point taps (22 fractional bits, zero past the bound); bounds [out_size][2] =
 * (first source index, number of taps).  max_kk: the capacity of kk in elements; non-zero when it is too small or an argument is refused. */
int car_debug_resample_coeffs(int32_t in_size, double in0, double in1, int32_t out_size, int32_t filter,
                              int32_t* ksize_out, int32_t* kk /* [out_size*ksize] */, int32_t* bounds /* [out_size*2] */, int64_t max_kk);

/* Host-only: the 256-entry table of car_clip_encode_image's requant step: out[u] = trunc(clamp(((u/255 - 0.5)/0.5 + 1) * 127.5, 0, 255)) in fp32. */
int car_debug_clip_requant_table(unsigned char* out /* [256] */);

/* Host-only: fp32 -> OCP e4m3fn bytes with the library's rounding (round-to-nearest-even, saturating at 448). */
int car_debug_f32_to_e4m3(const float* in, unsigned char* out, int64_t n);

/* Host-only: the operand split of car_config.vq_split_bf16 on n values: hi[i] = round-to-nearest-even bf16 bits of x[i], lo[i] = RNE bf16 bits of
 * x[i] - float(hi[i]); where hi[i] is not finite (inf, NaN, or a value that rounds to inf) lo[i] is zero. */
int car_debug_split_bf16(const float* x, int64_t n, uint16_t* hi, uint16_t* lo);

/* Runs the fused vocabulary projection + cross-entropy kernel behind car_score alone (tests).  x [R,D] and w [V,D] in the context's element type, targets
 * int32, all on the device; D a multiple of 32 (CAR_BF16) or 16 (CAR_F32), V of 4.  nll[r] = logsumexp_n(x[r] . w[n]) - x[r] . w[targets[r]]; logits
 * (or NULL) takes the fp32 rows.  With pair_scale [R/2] (R even) rows [0,R/2) are conditional and rows [R/2,R) their unconditional twins, row r scores
 * u + (c - u) * pair_scale[r] (a scale of exactly 1 takes c as it is), and targets, nll and logits have R/2 rows.  round_bf16 != 0 rounds every product
 * row to bf16 first, as the CAR_BF16 model pass does.  Works on any context (no weights needed). */
int car_debug_score_rows(car_ctx* ctx, const void* x, const void* w, const int32_t* targets, const float* pair_scale,
                         int32_t R, int32_t V, int32_t D, int32_t round_bf16, float* nll, float* logits, void* stream);

/* Host-only: the lane predicates of the bf16 decode attention's edge blocks.  [lo, hi] (0 <= lo <= hi <= 31) is the range of attended rows inside one
 * 32-position block of the packed KV cache; k_mask[i*64 + l] / v_mask[i*64 + l] = 1 if lane l of the block's i-th 1-KiB K / V load (i = 0..3) is issued,
 * 0 if the lane holds no attended row and gets zeros instead.  Non-zero on a range outside those bounds. */
int car_debug_attn_edge_mask(int32_t lo, int32_t hi, unsigned char* k_mask /* [4*64] */, unsigned char* v_mask /* [4*64] */);

/* Host-only: the prefill window of car_generate (grain 16) and car_score (grain 32) over a prompt of T positions whose first valid (unpadded) position over
 * the batch is first_valid: the pass computes rows [t0, T), Tv = T - t0 of them.  t0 is the largest multiple of grain that is <= min(clamp(first_valid, 0, T),
 * T - 8); t0 = 0 unless T > 8 and T is a multiple of 8.  Non-zero on T <= 0 or a grain that is not a positive multiple of 8. */
int car_debug_prompt_window(int32_t T, int32_t first_valid, int32_t grain, int32_t* t0, int32_t* Tv);

/* Copies the cached control tokens of layer-group k (0..2) [b,n_tok,dim] as fp32 to a HOST buffer (tests). */
int car_debug_control_tokens(car_ctx* ctx, int32_t k, float* host_out, int64_t max_elems);

#ifdef __cplusplus
}
#endif
#endif /* CONTROLAR_HIP_H */
