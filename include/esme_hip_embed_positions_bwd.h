/* Backward of the learned-position half of esme_hip_embed_positions (libesme_hip.so, gfx950): the gradient of the position table of
 * ESM-1b / ESM-1v, what training the table alone (the run that made the 4 096-position checkpoints) and masked-LM training of these
 * models need.
 *
 * Definition.  The packed forward adds table row (in-sequence position + pos_offset) to every row of a sequence, so with the gradient
 * dX (T, E) of the lookup's output and the sequences' offsets cu_lens (B + 1),
 *     dP[r, :] = sum over { b : len_b > r - pos_offset >= 0 } of dX[cu_lens[b] + (r - pos_offset), :]     for pos_offset <= r < pos_offset + max_len,
 *     dP[r, :] = 0                                                                                        for every other r in [0, P),
 * len_b = cu_lens[b + 1] - cu_lens[b].  The transpose of esme_hip_embed_positions as the packed forward calls it (pos_idx = the
 * in-sequence position, pos_offset = padding_idx + 1 = 2).
 *
 * A reduction ACROSS sequences with a fan-in of at most B per table row.  One launch, no workspace, no atomics: a work item is
 * (table row, 8 columns) and belongs to one lane, which walks the sequences b = 0 .. B-1 in ASCENDING order and adds the row of each
 * sequence that is long enough into fp32 accumulators, rounded to bf16 once at the end.  The accumulators start at +0.0 and a
 * sequence too short for the row enters NOTHING (the add is skipped, not made with a zero); so a row reached only by -0.0 values
 * is +0.0, as 0.0f + -0.0f is.  The summation order is a function of cu_lens alone, so dP is bit-equal from run to run and from
 * device to device.
 */
#ifndef ESME_HIP_EMBED_POSITIONS_BWD_H
#define ESME_HIP_EMBED_POSITIONS_BWD_H

#include "esme_hip.h"   /* ESME_OK / ESME_ERR_*, esme_hip_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

/* d_x: (T, E) bf16 with unit column stride and row stride ld (% 8 == 0, >= E), 16-byte aligned.  cu_lens: int32 (B + 1) on the device,
 * non-decreasing, cu_lens[B] <= T.  d_pos: (P, E) bf16, contiguous, 16-byte aligned: EVERY element is written (rows below pos_offset,
 * rows from pos_offset + max_len on and rows no sequence reaches become exact zeros; the memory may arrive uninitialised).
 * max_len bounds the rows that are summed, not the sequences: a sequence longer than max_len contributes its first max_len rows.
 * B == 0 or T == 0 writes zeros (d_x and cu_lens may then be null).  Nothing outside the rows [0, T) of d_x and the B + 1 entries of
 * cu_lens is read: a row index cu_lens[b] + p outside [0, T) is skipped.
 * ESME_ERR_UNSUPPORTED (-2): E % 8 != 0, T >= 2^31.  ESME_ERR_ARG (-1): B < 0, T < 0, E <= 0, P <= 0, pos_offset < 0, max_len < 0,
 * max_len + pos_offset > P, a null or misaligned pointer, a bad row stride. */
int esme_hip_embed_positions_bwd(const void* d_x, int64_t ld, const int32_t* cu_lens, int B, int64_t T, int E, int P, int pos_offset,
                                 int max_len, void* d_pos, void* stream);

#ifdef __cplusplus
}
#endif
#endif
