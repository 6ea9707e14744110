/* Backward of the token-embedding lookup esme_hip_embed (libesme_hip.so, gfx950): the gradient of the embedding table, what
 * masked-LM training (continued pretraining) needs beyond full fine-tuning.
 *
 * Definition.  With the packed rows' ids tok[t] and the gradient dX (T, E) of the lookup's output,
 *     dE[v, :] = sum over { t : tok[t] == v } of dX[t, :]        for v = 0 .. V-1, v not in {mask_idx, pad_idx},
 *     dE[v, :] = 0                                               for v in {mask_idx, pad_idx}.
 * mask_idx / pad_idx follow the forward's convention (-1: none): the forward writes a zero row for these ids, so their table rows
 * have no influence on the output.  An id outside [0, V) contributes nothing (the forward writes a zero row there too).
 *
 * A reduction with extreme fan-in (50 000 packed rows onto 33 table rows).  Two launches, no atomics:
 *   1. per (chunk of ESME_HIP_EMBED_BWD_ROWS rows, 8 columns): one lane walks the chunk's rows in ascending order and adds each into
 *      its own fp32 accumulators acc[V][8] in LDS; the chunk's (V, E) fp32 partial goes to the workspace;
 *   2. per (v, column): the chunks' partials in ascending chunk order, rounded to bf16 once.
 * The summation order is a function of (T, E, V) alone, so dE is bit-equal from run to run and from device to device.
 */
#ifndef ESME_HIP_EMBED_BWD_H
#define ESME_HIP_EMBED_BWD_H

#include "esme_hip.h"   /* ESME_OK / ESME_ERR_*, esme_hip_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

/* Rows per chunk of the first launch (part of the summation order, hence of the result's bits). */
#define ESME_HIP_EMBED_BWD_ROWS 256
/* Largest table the kernel serves: the fp32 accumulators of a workgroup are V * 2 KiB of LDS. */
#define ESME_HIP_EMBED_BWD_MAX_V 64

/* Workspace of one esme_hip_embed_bwd call, in bytes:  ceil(T / ESME_HIP_EMBED_BWD_ROWS) * V * E * sizeof(float)  -- the chunks'
 * partials.  It needs no initialisation and carries nothing from one call to the next.  T == 0: 0.
 * T < 0, E <= 0, V <= 0: ESME_ERR_ARG; E % 8 != 0, V > ESME_HIP_EMBED_BWD_MAX_V, T >= 2^31: ESME_ERR_UNSUPPORTED (negative returns). */
int64_t esme_hip_embed_bwd_workspace_bytes(int64_t T, int E, int V);

/* d_x: (T, E) bf16 with unit column stride and row stride ld_dx (% 8 == 0, >= E), 16-byte aligned.  tokens: int64 (T) on the device.
 * d_table: (V, E) bf16, contiguous, 16-byte aligned: EVERY element is written (a row whose id does not occur or is excluded becomes
 * zeros; the memory may arrive uninitialised).  workspace: esme_hip_embed_bwd_workspace_bytes(T, E, V) bytes, 16-byte aligned (may be
 * null when that is 0).  T == 0 writes zeros.  Nothing outside the rows [0, T) of d_x and tokens is read.
 * Sizes as for the workspace query (ESME_ERR_ARG / ESME_ERR_UNSUPPORTED). */
int esme_hip_embed_bwd(const void* d_x, int64_t ld_dx, const int64_t* tokens, int64_t T, int E, int V, int mask_idx, int pad_idx,
                       void* d_table, void* workspace, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
