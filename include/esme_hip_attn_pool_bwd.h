/* Backward of attention pooling over a cu_lens-packed batch (libesme_hip.so, gfx950): what fine-tuning a task head
 * (AttentionPool, LearnedAttentionPool, LearnedAggregation, BinaryLearnedAggregation) needs of esme_hip_attn_pool.
 *
 * Definition.  The forward (esme_hip.h) is a function of the embedding x (T, E) and the folded queries U (J = n_cls * heads, E) fp32,
 * which carry log2(e) / sqrt(d).  For sequence s, class token c, head h, j = c * heads + h, d = E / heads:
 *     sigma_tj = U_j . x_t,   p_tj = 2^sigma_tj / sum_{t' in s} 2^sigma_t'j,   out[s, c, h d + i] = sum_{t in s} p_tj x_t[h d + i].
 * Given dO (B, n_cls, E):
 *     dP_tj     = sum_i dO[s, c, h d + i] x_t[h d + i]
 *     Delta_sj  = sum_{t in s} p_tj dP_tj
 *     dsigma_tj = ln 2 * p_tj * (dP_tj - Delta_sj)
 *     dU_j      = sum_s sum_{t in s} dsigma_tj x_t
 *     dX_t[e]   = sum_j dsigma_tj U_j[e] + sum_c p_{t,(c, h(e))} dO[s, c, e].
 * The gradients of the class tokens and of the key weight follow from dU through the fold (a (C, H, d) x (H, d, E) contraction),
 * which is the caller's; the key bias cancels in the softmax and has gradient zero.
 *
 * Three launches, no atomics.  Work items are the forward's: chunks of 64 rows that start at each sequence's own first row.
 *   1. per chunk: sigma, dP, and with the chunk's own maximum the chunk's sum of 2^(sigma - max) and of 2^(sigma - max) dP;
 *   2. per chunk and 256 columns of E: the sequence's maximum, sum and Delta from its chunks in chunk order (Delta in fp32 from the
 *      recomputed p and dP, never from the rounded forward output), then p, dsigma, the chunk's rows of dX (one rounding to the
 *      output dtype) and the chunk's partial of dU;
 *   3. dU = the partials summed in slot order.
 * Every reduction has a fixed order: dX and dU are bit-equal from run to run, and a sequence's rows of dX are bit-equal whether it is
 * run alone or packed among others.  dU sums over the sequences, so it is reproducible from run to run only.
 */
#ifndef ESME_HIP_ATTN_POOL_BWD_H
#define ESME_HIP_ATTN_POOL_BWD_H

#include "esme_hip.h"   /* ESME_OK / ESME_ERR_*, esme_hip_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of one esme_hip_attn_pool_bwd call, in bytes, with slots = B + floor(T / 64) + 1 and J = n_cls * heads:
 *     slots * (2 + 3 J + 2 * 64 J + J E) * 4
 * -- per slot: {sequence, rows} (int32), per j {max, sum, Delta part}, sigma and dP of the chunk's 64 rows, and the chunk's partial
 * of dU, J x E fp32 (the one large term: slots * J * E * 4 bytes).  No T x E fp32 object exists.  It needs no initialisation and
 * carries nothing from one call to the next.  Geometry errors are the forward's and come back as a negative code: E % 8, E % heads,
 * negative or zero sizes ESME_ERR_ARG; n_cls * heads > 512 ESME_ERR_UNSUPPORTED. */
int64_t esme_hip_attn_pool_bwd_workspace_bytes(int B, int64_t T, int E, int heads, int n_cls);

/* x: (T, E) bf16, or fp32 when dtype_f32, row stride ldx -- the embedding the forward consumed.  U: (J, E) fp32 contiguous, the
 * forward's.  d_out: (B, n_cls, E) in x's dtype, row stride ldg >= n_cls * E per sequence.  dx: (T, E) in x's dtype, row stride lddx,
 * or NULL when the embedding gradient is not wanted (a frozen backbone): the work that feeds only dx is then skipped and dU is
 * bit-equal to the run with dx.  dU: (J, E) fp32 contiguous.  dx and dU must not overlap the inputs.
 * x, U, dx and the workspace 16-byte aligned; ldx and lddx multiples of 8 (bf16) or 4 (fp32) and >= E (else ESME_ERR_ARG).
 * cu_lens: int32 (B + 1) on the device.  Rows of dx that belong to no sequence are not written; an empty sequence contributes
 * nothing; no row outside [cu[s], cu[s+1]) is read for sequence s.  dU is always written (zeros when no sequence has a row).
 * workspace: esme_hip_attn_pool_bwd_workspace_bytes(B, T, E, heads, n_cls) bytes.  B == 0: dU = 0, nothing else is touched. */
int esme_hip_attn_pool_bwd(const void* x, int64_t ldx, const int32_t* cu_lens, int B, int64_t T, int E, int heads, int n_cls,
                           const float* U, const void* d_out, int64_t ldg, void* dx, int64_t lddx, float* dU, void* workspace,
                           int64_t ws_bytes, int dtype_f32, void* stream);

#ifdef __cplusplus
}
#endif
#endif
