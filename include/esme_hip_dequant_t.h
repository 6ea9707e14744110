/* Transposing expansion of the weight-only storage formats of esme_hip.h (libesme_hip.so, gfx950): W^T as bf16, straight from the
 * codes.  Training adapters over a quantised base needs dX = dY W, which the GEMM kernel computes against a row-major (K, N) copy of
 * W^T; keeping such a copy per projection would cost four times what the 4-bit codes cost, so it is expanded into a scratch buffer
 * every time it is used.
 *
 * Definition.  For codes / absmax (scale) exactly as esme_hip_dequantize_4bit / _8bit take them,
 *     out[k * ldo + n] == the bf16 value those entries (with col_scale == NULL) write to [n * ld + k],       0 <= n < N, 0 <= k < K,
 * bit for bit: the same fp32 expression (codebook[code] * absmax, resp. (code * scale) / 127) and the same one rounding to bfloat16.
 *
 * One workgroup owns a 128 (n) x 64 (k) tile: it reads the codes as the plain kernels do (4-byte words, 8-byte for int8: 8 elements
 * of one weight row per lane, lanes along k), decodes in registers, transposes through LDS and writes `out` in 16-byte stores, 256
 * contiguous bytes per output row and tile.  No atomics, no workspace; the result does not depend on the device or the grid.
 */
#ifndef ESME_HIP_DEQUANT_T_H
#define ESME_HIP_DEQUANT_T_H

#include "esme_hip.h"   /* ESME_OK / ESME_ERR_*, esme_hip_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

/* codes: (N, K / 2) uint8, 4-byte aligned (a row slice of a larger packed tensor is fine: K / 2 is a multiple of 32).
 * absmax: (N, K / 64) float.  codebook: 16 HOST floats in [-1, 1].  out: (K, N) bf16, row stride ldo.
 * N >= 0 (N == 0: ESME_OK, nothing written), K > 0; K % 64 != 0 is ESME_ERR_UNSUPPORTED.  ldo >= N, ldo % 8 == 0, out 16-byte
 * aligned (else ESME_ERR_ARG).  N need not be a multiple of the tile: nothing outside out[0:K, 0:N] is written, in particular not
 * the columns N .. ldo - 1, and no code / absmax row >= N is read.  All checks run before any launch. */
int esme_hip_dequantize_4bit_t(const void* codes, const float* absmax, int64_t N, int K, const float* codebook, void* out, int64_t ldo,
                               void* stream);

/* codes: (N, K) int8, 8-byte aligned.  scale: (N) float.  out: (K, N) bf16, row stride ldo.  As above with K % 8 != 0
 * ESME_ERR_UNSUPPORTED (K need not be a multiple of the tile either). */
int esme_hip_dequantize_8bit_t(const void* codes, const float* scale, int64_t N, int K, void* out, int64_t ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif
