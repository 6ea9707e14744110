/* Fused linear layer + cross-entropy over packed rows (libesme_hip.so, gfx950): the loss of a per-residue classifier and of the
 * masked-LM head's last projection, and its gradients, without materialising the (T, C) logits.
 *
 * Definition.  x (T, E) bf16, W (C, E) bf16, b (C) bf16 or null, labels y (T) int32 / int64, class weights cw (C) fp32 or null (ones):
 *     z_t   = W x_t + b                       lse_t = log sum_c exp z_tc
 *     l_t   = cw[y_t] (lse_t - z_{t, y_t})    for a KEPT row, 0 otherwise
 *     L     = sum_t l_t                       D = sum over kept rows of cw[y_t]
 *     loss  = L (sum)  or  L / D (mean; 0 when D == 0)
 * A row is kept when y_t != ignore_index and 0 <= y_t < C: a label outside [0, C) is an ignored row and never indexes anything.
 * With D == 0 the mean is 0 and every gradient is zero (torch returns NaN there): nothing on the host can look at D without a
 * synchronisation, and a NaN would reach the fp32 master weights of the optimiser.
 *
 * Backward, with the upstream gradient g as a DEVICE scalar and s = 1 (sum) or 1 / D (mean; 0 when D == 0):
 *     G_tc = g s cw[y_t] (exp(z_tc - lse_t) - [c == y_t])   on kept rows, 0 elsewhere
 *     dX = G W (bf16, every row written),   dW = G^T X,   db = sum_t G_t.
 * The logits are recomputed from x.  G is rounded to bf16 where it becomes an MFMA operand (dX and dW) and db sums the same rounded
 * values.  dW / db: rows in chunks of ESME_HIP_LINEAR_XENT_CHUNK (dW) and ESME_HIP_LINEAR_XENT_TILE (db), fp32 partials, added in
 * ascending chunk order, rounded once.  L and D: per-tile partials in row order, then one launch that adds them in a fixed order.
 * No atomics anywhere: every output is bit-equal from run to run, and l_t, lse_t and row t of dX depend on row t alone.
 * A non-finite value in row t of x makes lse_t, l_t (kept rows), row t of dX, L, the loss and dW non-finite and touches no other row.
 */
#ifndef ESME_HIP_LINEAR_XENT_H
#define ESME_HIP_LINEAR_XENT_H

#include "esme_hip.h"   /* ESME_OK / ESME_ERR_*, esme_hip_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

/* Rows per workgroup tile: the unit of the L / D / db partials (part of the summation order). */
#define ESME_HIP_LINEAR_XENT_TILE 64
/* Rows per chunk of the dW contraction (part of the summation order). */
#define ESME_HIP_LINEAR_XENT_CHUNK 512
/* Largest number of classes: one 64-wide MFMA column tile (classes C .. 63 are padding inside the kernel only). */
#define ESME_HIP_LINEAR_XENT_MAX_C 64

/* Workspace of the forward in bytes: 2 floats per tile.  T == 0: 0.  T < 0: ESME_ERR_ARG; T >= 2^31: ESME_ERR_UNSUPPORTED. */
int64_t esme_hip_linear_xent_fwd_workspace_bytes(int64_t T);
/* Workspace of the backward in bytes, O(T C + chunks C E): the transposed padded weight (E, 64) bf16, G^T (C, T rounded up to the
 * tile) bf16, the db partials (tiles, 64) fp32 and the dW partials (chunks, C, E) fp32.  Needs no initialisation.
 * Bad sizes: ESME_ERR_ARG; E % 8 != 0, C > ESME_HIP_LINEAR_XENT_MAX_C, T >= 2^31: ESME_ERR_UNSUPPORTED (negative returns). */
int64_t esme_hip_linear_xent_bwd_workspace_bytes(int64_t T, int E, int C);

/* x: rows [0, T) of E bf16 with row stride ld_x (>= E, % 8 == 0); w: (C, E) bf16 with row stride ld_w; bias: C bf16 or null;
 * labels: T int64 (labels_i64 != 0) or int32; class_weight: C fp32 or null; mean: 0 sum, 1 weighted mean.
 * Outputs, all fp32 and all written: loss_rows (T), lse (T), sums[0] = L, sums[1] = D, sums[2] = the loss (sums: 4 floats).
 * Every pointer 16-byte aligned.  T == 0: OK with sums = 0 (x, labels, loss_rows, lse, workspace may then be null). */
int esme_hip_linear_xent_fwd(const void* x, int64_t ld_x, const void* w, int64_t ld_w, const void* bias, const void* labels, int labels_i64,
                             int64_t ignore_index, const float* class_weight, int64_t T, int E, int C, int mean, float* loss_rows, float* lse,
                             float* sums, void* workspace, int64_t ws_bytes, void* stream);

/* lse, sums: what the forward wrote on the same operands.  grad: the upstream gradient, one fp32 on the device.
 * want_dx: d_x (T, E) bf16 with row stride ld_dx, every row written (zeros on rows that are not kept).
 * want_dw: d_w (C, E) and d_b (C; may be null when bias is null), contiguous, bf16 or (out_f32) fp32, every element written.
 * T == 0: OK with d_w = d_b = 0. */
int esme_hip_linear_xent_bwd(const void* x, int64_t ld_x, const void* w, int64_t ld_w, const void* bias, const void* labels, int labels_i64,
                             int64_t ignore_index, const float* class_weight, int64_t T, int E, int C, int mean, const float* lse,
                             const float* sums, const float* grad, int want_dx, void* d_x, int64_t ld_dx, int want_dw, void* d_w, void* d_b,
                             int out_f32, void* workspace, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
