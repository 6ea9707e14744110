/* Fused AdamW with fp32 master weights over a LIST of tensors (libesme_hip.so, gfx950): what bf16 fine-tuning needs after the
 * backward pass.  A bf16 weight of magnitude 0.05 has an ulp of 2.4e-4; an AdamW update at lr = 1e-5 is under half of it and rounds
 * away, so the step is taken on an fp32 master copy, with fp32 moments, and the bf16 parameter is written from the master.
 *
 * The tensor list.  Every entry point works on a table that the caller fills on the host and uploads (one stream-ordered copy) before
 * the call; the same bytes are handed over twice, as `table_host` (validated before any launch, never dereferenced by a kernel) and
 * `table_dev` (read by the kernels).  Layout, esme_hip_optim_table_bytes(n_tensors, n_groups) bytes in all:
 *     esme_optim_row_t   rows[n_tensors]
 *     esme_optim_group_t groups[n_groups]
 *     int64_t            prefix[n_tensors + 1]       prefix[0] = 0, prefix[r + 1] = prefix[r] + ceil(rows[r].numel / ESME_OPTIM_CHUNK)
 * Work is cut into chunks of ESME_OPTIM_CHUNK elements; workgroup c finds its tensor in `prefix` (the last r with prefix[r] <= c).
 * The launch count of every entry point is independent of n_tensors, and the partition depends on the list of numels alone.
 *
 * Arithmetic of esme_hip_optim_adamw_step, per element, all fp32 (fma = one rounding; sqrt and the divide correctly rounded):
 *     g  = float(grad) * s                                   s = *scale, a device float: clip coefficient x 1 / accumulated micro-batches
 *     m  = fma(beta1, m, one_minus_beta1 * g)
 *     v  = fma(beta2, v, (one_minus_beta2 * g) * g)
 *     w  = fma(-step_size, m / fma(sqrt(v), inv_sqrt_bc2, eps), master * decay)
 *     master, exp_avg, exp_avg_sq <- w, m, v
 *     param <- bf16 round-to-nearest-even(w)                 (an fp32 parameter IS its master: `master` is ignored, nothing else is stored)
 * with the host's float64 scalars rounded once to fp32: decay = 1 - lr * weight_decay (decoupled decay), step_size = lr / bc1,
 * inv_sqrt_bc2 = 1 / sqrt(bc2), bc1 = 1 - beta1^t, bc2 = 1 - beta2^t for the TENSOR's own step count t.  That is
 *     w = master (1 - lr wd) - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps).
 *
 * Addresses need the alignment of their element only (a parameter may be a view at an odd element offset).  A tensor whose five
 * arrays are all 16-byte aligned moves 16 bytes per lane and array; any other tensor, and the last numel % 8 elements, go element by
 * element through the same arithmetic, so no result bit depends on an address.  No element outside [0, numel) of any array is read
 * or written.  No atomics: results are bit-equal from run to run.
 */
#ifndef ESME_HIP_OPTIM_H
#define ESME_HIP_OPTIM_H

#include "esme_hip.h"   /* ESME_OK / ESME_ERR_*, esme_hip_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

#define ESME_OPTIM_CHUNK 8192          /* elements of one chunk = of one workgroup */

#define ESME_OPTIM_PARAM_F32 1         /* row flag: the parameter is fp32 and is its own master */
#define ESME_OPTIM_GRAD_F32  2         /* row flag: `grad` is fp32 (else bf16) */
#define ESME_OPTIM_ACC_INIT  4         /* row flag, esme_hip_optim_grad_accumulate only: the accumulator is overwritten, not added to */

typedef struct esme_optim_row_t {      /* 64 bytes */
    void*   param;                     /* bf16, or fp32 with ESME_OPTIM_PARAM_F32 */
    void*   grad;                      /* bf16, or fp32 with ESME_OPTIM_GRAD_F32 */
    void*   master;                    /* fp32; esme_hip_optim_grad_accumulate: the fp32 accumulator */
    void*   exp_avg;                   /* fp32 */
    void*   exp_avg_sq;                /* fp32 */
    int64_t numel;                     /* >= 0 */
    int32_t flags;
    int32_t group;                     /* index into groups[] */
    float   step_size;                 /* lr / bc1 */
    float   inv_sqrt_bc2;              /* 1 / sqrt(bc2) */
} esme_optim_row_t;

typedef struct esme_optim_group_t {    /* 32 bytes */
    float lr, beta1, beta2, eps, weight_decay;
    float decay;                       /* 1 - lr * weight_decay */
    float one_minus_beta1, one_minus_beta2;
} esme_optim_group_t;

/* ESME_OPTIM_CHUNK, for a binding that cannot read the macro. */
int esme_hip_optim_chunk_elems(void);

/* Bytes of the table: 64 * n_tensors + 32 * n_groups + 8 * (n_tensors + 1); n_tensors < 0 or n_groups < 0: ESME_ERR_ARG. */
int64_t esme_hip_optim_table_bytes(int n_tensors, int n_groups);

/* Workspace of esme_hip_optim_grad_sqnorm for a list of total_chunks = prefix[n_tensors] chunks: 4 * max(total_chunks, 4) bytes (one fp32
 * partial per chunk).  It needs no initialisation.  total_chunks < 0 or >= 2^31: ESME_ERR_ARG. */
int64_t esme_hip_optim_workspace_bytes(int64_t total_chunks);

/* What every entry point below checks on table_host before it launches anything (ESME_ERR_ARG): table_host and table_dev non-NULL and
 * 8-byte aligned; n_tensors >= 0, n_groups >= 0; per row numel >= 0, no unknown flag, and where numel > 0 the arrays the entry point
 * uses non-NULL and aligned to their element; prefix as defined above, prefix[n_tensors] < 2^31.  stream: a hipStream_t (NULL: the
 * default stream).  Nothing synchronises with the host. */

/* The fused step.  Uses param, grad, master (bf16 parameters), exp_avg, exp_avg_sq of every row and rows[r].group < n_groups (which
 * must then be >= 1).  scale: device float, 4-byte aligned, read by the kernel.  One launch; none when the list has no chunk. */
int esme_hip_optim_adamw_step(const void* table_host, const void* table_dev, int n_tensors, int n_groups, const void* scale, void* stream);

/* Global L2 norm of the list's gradients, for clipping.  Uses `grad` of every row.  Launch 1: every chunk sums float(g)^2 in fp32 -- a
 * lane adds its elements in index order (element i of a chunk belongs to lane (i / 8) % 256), then the fixed butterfly over the 64 lanes
 * and the 4 waves in order -- and writes its partial to the workspace.  Launch 2: one workgroup adds the partials in float64, lane t
 * those with index = t mod 256 in order, then the same tree.  With S the sum:
 *     out[0] = norm = float(sqrt(S) * grad_scale)            (the norm of the gradients as the step will see them before clipping)
 *     out[1] = coef = min(1, max_norm / (norm + 1e-6))       (torch's clip_grad_norm_; a NaN norm gives NaN, an infinite one 0, as
 *                                                             there with error_if_nonfinite=False); max_norm <= 0: coef = 1
 *     out[2] = coef * grad_scale                             (the `scale` of esme_hip_optim_adamw_step)
 * out: 3 device floats, 4-byte aligned.  workspace: esme_hip_optim_workspace_bytes(prefix[n_tensors]) bytes, 4-byte aligned; a smaller
 * ws_bytes is ESME_ERR_ARG.  grad_scale must be finite and > 0. */
int esme_hip_optim_grad_sqnorm(const void* table_host, const void* table_dev, int n_tensors, int n_groups, float max_norm, float grad_scale,
                               void* workspace, int64_t ws_bytes, void* out, void* stream);

/* fp32 accumulator += gradient over the list: master[i] = (ESME_OPTIM_ACC_INIT ? 0 : master[i]) + float(grad[i]), one rounding.  Uses
 * `grad` and `master` of every row.  One launch. */
int esme_hip_optim_grad_accumulate(const void* table_host, const void* table_dev, int n_tensors, int n_groups, void* stream);

#ifdef __cplusplus
}
#endif
#endif
