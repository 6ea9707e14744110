/* Backward of the varlen, block-diagonal attention over a cu_lens-packed batch (libesme_hip.so, gfx950): what LoRA fine-tuning needs
 * of the attention kernel.  Base weights stay frozen, so this is the one piece of a training step torch has no stand-in for.
 *
 * Definition.  Per sequence (rows [cu[s], cu[s+1]) of the packed batch) and head, with S = Q K^T * softmax_scale, P = softmax_j(S),
 * O = P V and an incoming gradient dO:
 *     D_i = sum_c dO_ic O_ic,   dV = P^T dO,   dP = dO V^T,   dS = P o (dP - D),   dQ = softmax_scale * dS K,   dK = softmax_scale * dS^T Q.
 *
 * The forward saves no softmax statistics; the backward computes them itself.  Three launches, no floating-point atomics:
 *   1. per (sequence, head, 64 query rows): all key tiles twice -> the exact row maximum (log2 units) and the row sum; D in fp32;
 *   2. per (sequence, head, 64 key rows): every query tile -> dK, dV;
 *   3. per (sequence, head, 64 query rows): every key tile -> dQ.
 * The two gradient kernels run seven matrix products per tile pair (S, dP, dV, dK; S, dP, dQ) instead of the five of a backward that
 * adds dQ with atomics, and the statistics kernel forms the scores twice more: the price of results that are bit-equal from run to
 * run and of a sequence's gradients not depending on its neighbours in the batch.
 *
 * Arithmetic: bf16 MFMA operands (16x16x32), fp32 accumulators; the softmax in fp32 log2 units; P and dS are rounded to bf16 where
 * they become MFMA operands (the flash-attention convention); statistics and D stay fp32; every output is rounded to bf16 once.
 */
#ifndef ESME_HIP_ATTN_BWD_H
#define ESME_HIP_ATTN_BWD_H

#include "esme_hip.h"   /* ESME_OK / ESME_ERR_*, esme_hip_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

/* Rows inside one sequence are addressed with unsigned 32-bit element offsets: max_len times each of the four row strides must
 * stay below this many elements, else ESME_ERR_UNSUPPORTED. */
#define ESME_HIP_ATTN_BWD_MAX_SEQ_ELEMS 4294967296LL

/* Workspace of one esme_hip_attn_varlen_bwd call, in bytes:  3 * H * T * sizeof(float)
 * -- per head and packed row the row maximum (log2 units), the row sum and D.  It needs no initialisation and carries nothing from
 * one call to the next.  Negative sizes or H <= 0: ESME_ERR_ARG (negative return). */
int64_t esme_hip_attn_varlen_bwd_workspace_bytes(int B, int64_t T, int H);

/* q, k, v: (T, H, d) bf16 views with ONE row stride ld_qkv -- exactly the operands the forward kernel consumed (post-rotary, q NOT
 * prescaled).  o: the forward's output, d_o: its gradient, (T, H * d) bf16 with their own row strides.  dq, dk, dv: (T, H, d) bf16
 * with one shared row stride ld_dqkv (they may be the three column blocks of one (T, 3E) buffer); they must not overlap the inputs.
 * Every operand 16-byte aligned, every row stride % 8 == 0 and >= H * d (else ESME_ERR_ARG).
 * d in {32, 64}; any other head dim: ESME_ERR_UNSUPPORTED.
 * cu_lens: int32 (B + 1) on the device; T < 2^31; any B (more than 65 535 sequences run as several launches); max_len >= the longest
 * sequence (rows past max_len are not processed); H <= 65 535; ESME_HIP_ATTN_BWD_MAX_SEQ_ELEMS above.
 * Rows of dq / dk / dv that belong to no sequence are not written; an empty sequence writes nothing; no row outside
 * [cu[s], cu[s+1]) is read for sequence s.
 * workspace: esme_hip_attn_varlen_bwd_workspace_bytes(B, T, H) bytes, 16-byte aligned.  B == 0 or T == 0 is a no-op. */
int esme_hip_attn_varlen_bwd(const void* q, const void* k, const void* v, int64_t ld_qkv, const void* o, int64_t ld_o,
                             const void* d_o, int64_t ld_do, const int32_t* cu_lens, int B, int64_t T, int H, int d, int max_len,
                             float softmax_scale, void* dq, void* dk, void* dv, int64_t ld_dqkv, void* workspace, int64_t ws_bytes,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
