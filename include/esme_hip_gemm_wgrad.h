/* Weight gradient of a projection y = x W^T + b over a packed batch (libesme_hip.so, gfx950): what full fine-tuning needs beside
 * the forward GEMM (esme_hip.h), which already serves dX = dY W.
 *
 * Definition.  dy (M, N) bf16 with row stride ld_dy, x (M, K) bf16 with row stride ld_x:
 *     dW[n, k] = sum_t dy[t, n] * x[t, k]        (N, K), row stride ld_dw, bf16, or fp32 when out_f32
 *     db[n]    = sum_t dy[t, n]                  (N) contiguous, dW's dtype; db == NULL skips it and changes no bit of dW.
 * The contraction runs over the row index t of BOTH operands.  128-column tiles of dy and x are staged in LDS as they lie in memory
 * ([row t][column], 64 rows at a time) and both operands of the 16x16x32 bf16 MFMA are gathered from them with the transposing LDS
 * read (ds_read_b64_tr_b16); no transposed copy of dy or x exists in global memory.  The rows past the last one of a 64-row stage are
 * zero-filled in LDS (the transposing read needs every lane: pad, don't mask).  Products are exact, accumulation is fp32, every output
 * element is rounded once.  db comes from the dy tiles the call streams anyway (one more MFMA against a tile of ones in the
 * workgroups of the first K-tile column): the terms are exact bf16 values added in fp32.
 *
 * No floating-point atomics.  One workgroup owns a 128 x 128 tile of dW.  When the tiles alone are few (the out-projection of
 * ESM2-650M has 100), the rows are cut into chunks: with tiles = ceil(N / 128) * ceil(K / 128),
 *     c      = the smallest c in 1 .. min(64, max(1, floor(2048 / tiles)), ceil(M / 256)) that maximises
 *              tiles * c / (512 * ceil(tiles * c / 512))      (rounds of 512 workgroups, the last one as full as possible)
 *     rows   = ceil(M / c) rounded up to a multiple of 64           (rows of a chunk; at least 64)
 *     chunks = max(1, ceil(M / rows)).
 * The partition is a function of (M, N, K) only -- never of the device -- so results are bit-equal from run to run and from box to
 * box.  With chunks == 1 the tile kernel writes dW (and db) itself and no workspace is needed; otherwise every chunk writes its fp32
 * partial to the workspace and a second launch sums the partials in chunk order and rounds once.
 */
#ifndef ESME_HIP_GEMM_WGRAD_H
#define ESME_HIP_GEMM_WGRAD_H

#include "esme_hip.h"   /* ESME_OK / ESME_ERR_*, esme_hip_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of one esme_hip_gemm_wgrad call, in bytes: 0 when chunks == 1, else chunks * (N * K + N) * 4 (the partials of dW, then
 * those of db, fp32).  It needs no initialisation and carries nothing from one call to the next.  Errors come back as a negative
 * code: M < 0, M >= 2^31, N <= 0 or K <= 0 ESME_ERR_ARG; N % 64 or K % 64 ESME_ERR_UNSUPPORTED. */
int64_t esme_hip_gemm_wgrad_workspace_bytes(int64_t M, int N, int K);

/* dy: (M, N) bf16, row stride ld_dy >= N.  x: (M, K) bf16, row stride ld_x >= K.  dw: (N, K) bf16 (fp32 when out_f32), row stride
 * ld_dw >= K, in elements of its dtype.  db: (N) contiguous in dw's dtype, or NULL.  Every pointer 16-byte aligned, every row stride
 * a multiple of 8 and at least its width (else ESME_ERR_ARG).  N % 64 == 0 and K % 64 == 0 (else ESME_ERR_UNSUPPORTED: the kernel
 * works on 64-column wave tiles).  0 <= M < 2^31; row offsets are 64-bit, so M * ld may exceed 2^31 elements.  M == 0 writes exact
 * zeros (dy and x may then be NULL).  dw and db must not overlap dy, x or the workspace.  No row >= M and no column outside N / K is
 * read; of dw only the N x K elements are written (not the gap up to ld_dw), of db its N.
 * workspace: esme_hip_gemm_wgrad_workspace_bytes(M, N, K) bytes, 16-byte aligned; may be NULL when that is 0.  A smaller ws_bytes is
 * ESME_ERR_ARG.  stream: a hipStream_t (NULL: the default stream). */
int esme_hip_gemm_wgrad(const void* dy, int64_t ld_dy, const void* x, int64_t ld_x, int64_t M, int N, int K, void* dw, int64_t ld_dw,
                        void* db, int out_f32, void* workspace, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
