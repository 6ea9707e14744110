/* The contact regression's features at chosen residue pairs, without materialising the maps (libesme_hip.so, gfx950).
 *
 * A contact regression (esme_hip_contacts.h) is trained on a list of residue pairs, not on whole maps.  With everything as defined in
 * esme_hip_contacts.h -- P the softmax over all S keys, f = trim_front, A = P without the trimmed rows and columns, r the row sums of
 * A + A^T, t their total -- the feature of pair p = (s, i, j) and head h of one layer is
 *     feat[p, col0 + h] = N^(h)_ij = P_{f+i,f+j} + P_{f+j,f+i} - r_i r_j / t        (i == j: 2 P_ii - r_i^2 / t;  i > j allowed),
 * with i, j counted from the first kept row of sequence s.  One call per layer with col0 = l * H fills the (P, L H) design matrix in
 * place, in the layer-major column order of the regression weights.  No S x S object, dense or per head, exists in device memory.
 *
 * Arithmetic: the call runs the three statistics passes of esme_hip_contact_layer unchanged (row maximum and row sum on the bf16 MFMA
 * with fp32 accumulators, r, t) and then one gather pass: per pair and head the two scores q_{f+i} . k_{f+j} and q_{f+j} . k_{f+i} as
 * fp32 fused multiply-adds of the exact bf16 products (eight elements per lane in index order, then a butterfly over the d / 8 lanes
 * of the head), normalised with the stored maximum and row sum in log2 units (exp2), minus r_i r_j / t.  No atomics, every reduction
 * in a fixed order: a pair's row does not depend on P, on its position in the list or on the other sequences of the batch, and
 * (s, i, j) and (s, j, i) give bit-identical rows.
 */
#ifndef ESME_HIP_CONTACT_FEATURES_H
#define ESME_HIP_CONTACT_FEATURES_H

#include "esme_hip_contacts.h"   /* ESME_HIP_CONTACT_MAX_SEQ_ELEMS; ESME_OK / ESME_ERR_*, esme_hip_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of one esme_hip_contact_features call, in bytes:  (3 * H * T + H * B) * sizeof(float)  (the statistics of
 * esme_hip_contact_layer).  It needs no initialisation and carries nothing from one call to the next.  Negative sizes or H <= 0:
 * ESME_ERR_ARG (negative return). */
int64_t esme_hip_contact_features_workspace_bytes(int B, int64_t T, int H);

/* q, k, ld_qk, cu_lens, B, T, H, d, max_len, softmax_scale, q_prescaled, trim_front, trim_back, workspace: as esme_hip_contact_layer --
 * the same operands, alignment (16-byte aligned q, k and workspace, ld_qk % 8 == 0, ld_qk >= H * d), sizes (d in {16, 32, 64, 128},
 * T < 2^31, H <= 65 535, max_len > 0, ESME_HIP_CONTACT_MAX_SEQ_ELEMS), error codes, and any B (more than 65 535 sequences run as
 * several launches).  workspace: esme_hip_contact_features_workspace_bytes(B, T, H) bytes.
 * pairs: int32 (P, 3) rows (s, i, j) on the device, contiguous; 0 <= P < 2^31.  A pair is in range when 0 <= s < B and
 * 0 <= i, j < S_s - trim_front - trim_back (and below max_len - trim_front - trim_back: rows past max_len have no statistics).  The
 * list is not validated on the host (no synchronisation): a pair out of range is skipped without reading q, k or the workspace for
 * it, and its H outputs are set to a quiet NaN.
 * feat: float on the device, row stride ld_feat >= col0 + H elements, col0 >= 0; the call writes feat[p * ld_feat + col0 + h] for
 * h = 0 .. H - 1 and touches no other column.
 * P == 0, B == 0 or T == 0 is a no-op. */
int esme_hip_contact_features(const void* q, const void* k, int64_t ld_qk, const int32_t* cu_lens, int B, int64_t T, int H, int d,
                              int max_len, float softmax_scale, int q_prescaled, int trim_front, int trim_back, const int32_t* pairs,
                              int64_t P, float* feat, int64_t ld_feat, int col0, void* workspace, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
