// engine_attn.hip — the batched multi-head attention of the host side (attn_bytes / attn_run): what car_encode_control, car_depth, both CLIP towers,
// car_t5_encode and the prompt pass of car_generate and car_score (engine_prompt.hip) share.
// (one of the translation units behind include/controlar_hip.h; shared declarations: engine_internal.h)
#include "engine_internal.h"

// fused attention (attn.hip) is the fast-mode path for 64-wide heads, and then no score / probability tensor exists
AttnBytes attn_bytes(const car_ctx* c, int nb, int T, int H, int hd) {
    const size_t Tpad = rup(T, 32); const bool fused = use_flash(c, hd);
    AttnBytes b;
    b.S = fused ? 0 : (size_t)nb * H * T * T * 4;
    b.P = fused ? 0 : (size_t)nb * H * T * Tpad * c->esz;
    b.Vt = (size_t)nb * H * hd * Tpad * c->esz;
    return b;
}

// V^T into ws[WS_ATTN_VT], then flash64 (use_flash), else S = scale * Q K^T (fp32, ws[WS_ATTN_S]) -> the softmax of the mask kind (P, ws[WS_ATTN_P]) -> out = P V.
// Non-zero: the fused kernel was chosen and car_launch_flash64 refused the shape; nothing further was launched (S and P were never sized: there is no
// falling back).  No caller can see that: flash64 (attn.hip, car_launch_flash64) wants token and sequence strides in multiples of 8 elements, 16-byte
// aligned q, k and V^T, 8-byte aligned out, vt_ld a multiple of 32 that covers Tk, and Tq == Tk under the causal mask.  use_flash means hd == 64, so every
// width here (H*64, ld = H*64 or 3*H*64, T*ld) is a multiple of 64 elements; q, k, out and V^T are DevBuf bases (hipMalloc: 256 bytes) plus plane offsets
// of rows * width elements or, in the packed layout, one width; vt_ld = rup(T, 32); Tq = Tk = T.
int attn_run(car_ctx* c, const AttnCall& a, hipStream_t st) {
    const int mode = c->mode, T = a.T, H = a.H, hd = a.hd, nb = a.nb, D = H * hd, Tpad = (int)rup(T, 32);
    float* S = (float*)c->ws[WS_ATTN_S].p; void* P = c->ws[WS_ATTN_P].p; void* vT = c->ws[WS_ATTN_VT].p;
    car_launch_transpose_pad(mode, a.v, a.ld, (long)T * a.ld, vT, nb, T, Tpad, D, st);
    if (use_flash(c, hd)) {
        FlashP f; memset(&f, 0, sizeof(f));
        f.q = (const bf16_t*)a.q; f.k = (const bf16_t*)a.k; f.vt = (const bf16_t*)vT; f.o = (bf16_t*)a.out;
        f.q_sb = f.k_sb = (long)T * a.ld; f.q_st = f.k_st = a.ld; f.vt_sb = (long)D * Tpad; f.vt_ld = Tpad; f.o_sb = (long)T * D; f.o_st = D;
        f.Tq = f.Tk = T; f.H = H; f.scale = a.scale; f.mode = a.kind; f.mask = a.mask; f.bias = a.bias;
        return car_launch_flash64(&f, nb, st);
    }
    {   // S[b,h] = (Q K^T) * scale, fp32
        GemmP q = gp(a.q, a.ld, a.k, a.ld, S, T, T, T, hd);
        q.alpha = a.scale; q.out_f32 = 1; q.nb0 = nb; q.nb1 = H;
        q.sA0 = (long)T * a.ld; q.sA1 = hd; q.sW0 = (long)T * a.ld; q.sW1 = hd; q.sC0 = (long)H * T * T; q.sC1 = (long)T * T;
        car_launch_gemm(mode, AMODE_PLAIN, &q, st);
    }
    const long rows = (long)nb * H * T;
    if (a.kind == ATTN_T5) car_launch_t5_softmax(mode, S, T, P, Tpad, rows, T, a.bias, a.mask, T, H, st);
    else if (a.kind == ATTN_CAUSAL) car_launch_softmax_at(mode, S, T, P, Tpad, rows, T, 1, a.mask, T, H, a.col0, st);
    else car_launch_softmax(mode, S, T, P, Tpad, rows, T, 0, nullptr, 0, 0, st);
    {   // out[b, t, h*hd + d] = P[b,h] @ V[b,h]
        GemmP q = gp(P, Tpad, vT, Tpad, a.out, D, T, hd, Tpad);
        q.nb0 = nb; q.nb1 = H;
        q.sA0 = (long)H * T * Tpad; q.sA1 = (long)T * Tpad; q.sW0 = (long)D * Tpad; q.sW1 = (long)hd * Tpad; q.sC0 = (long)T * D; q.sC1 = hd;
        car_launch_gemm(mode, AMODE_PLAIN, &q, st);
    }
    return 0;
}
