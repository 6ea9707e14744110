/* Backward of the per-sequence mean esme_hip_segment_mean (libesme_hip.so, gfx950): the gradient that a mean-pooling head
 * (PartitionMeanPool, ClsHead) hands back to the packed rows of the backbone.
 *
 * Definition.  With cu_lens (B + 1) the sequences' row offsets and dY (B, E) the gradient of the means,
 *     dX[t, :] = round(float(dY[s, :]) / float(cu_lens[s + 1] - cu_lens[s]))      for cu_lens[s] <= t < cu_lens[s + 1],
 *     dX[t, :] = 0                                                                for every other row t of [0, T):
 * the rows before cu_lens[0], the rows from cu_lens[B] on, and all of them when B == 0.  The division is IEEE fp32 and the
 * quotient is rounded ONCE to dY's type (bf16: to nearest even; fp32: it is the quotient).  An empty sequence owns no row and
 * contributes nothing.
 *
 * One launch, no atomics, no host read of cu_lens: a workgroup owns ESME_HIP_SEGMENT_MEAN_BWD_ROWS consecutive rows of dX, finds
 * each row's sequence by bisection of cu_lens on the device, and writes the rows in 16-byte pieces.  B is not a grid dimension,
 * so any B (beyond 65 535 too) takes the same single launch.  Every element of the rows [0, T) of dX is written exactly once; the
 * memory may arrive uninitialised.
 */
#ifndef ESME_HIP_SEGMENT_MEAN_BWD_H
#define ESME_HIP_SEGMENT_MEAN_BWD_H

#include "esme_hip.h"   /* ESME_OK / ESME_ERR_*, esme_hip_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

/* Rows of dX per workgroup (no influence on the result). */
#define ESME_HIP_SEGMENT_MEAN_BWD_ROWS 32

/* d_y: (B, E) with unit column stride and row stride ld_dy; d_x: (T, E) with unit column stride and row stride ld_dx; both bf16
 * (dtype_f32 == 0) or both fp32 (dtype_f32 != 0), 16-byte aligned, row strides >= E and multiples of 8 (bf16) / 4 (fp32) elements.
 * cu_lens: int32 (B + 1) on the device, ascending.  Whatever cu_lens holds, nothing outside the rows [0, T) of d_x is written and
 * nothing outside the rows [0, B) of d_y is read (a row that bisection assigns to a sequence of non-positive length becomes zeros).
 * T == 0 does nothing; B == 0 writes zeros (d_y and cu_lens may then be null).
 * B < 0, T < 0, E <= 0, a null pointer, a bad stride or alignment: ESME_ERR_ARG; E % 8 != 0, T >= 2^31: ESME_ERR_UNSUPPORTED. */
int esme_hip_segment_mean_bwd(const void* d_y, int64_t ld_dy, const int32_t* cu_lens, int B, int64_t T, int E,
                              void* d_x, int64_t ld_dx, int dtype_f32, void* stream);

#ifdef __cplusplus
}
#endif
#endif
