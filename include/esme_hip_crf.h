/* Linear-chain conditional random field over packed sequences (libesme_hip.so, gfx950): the log-partition function by the forward
 * algorithm, its gradients by the backward algorithm (posterior marginals), and Viterbi decoding.
 *
 * Definition.  emissions e (T, C) fp32, transitions A (C, C) fp32 with A[i][j] the score of moving from label i to label j
 * (pytorch-crf's orientation), start (C) and end (C) fp32, cu_lens (B + 1) int32, tags (T) int32, 1 <= C <= 64.  Row t takes one role:
 *     0 <= tags[t] < C                 the row is in its sequence's chain and constrained to that label,
 *     tags[t] == ESME_HIP_CRF_FREE     the row is in the chain and every label is allowed,
 *     any other value (ESME_HIP_CRF_SKIP is the named one)   the row is not in the chain: the chain links the previous chain row
 *                                      of the same sequence to the next one (how <cls> / <eos> rows drop out).
 * For sequence b with chain rows t_1 < ... < t_n:
 *     log Z_b = log sum over the label paths y consistent with the constraints of
 *               exp(start[y_1] + sum_k e[t_k][y_k] + sum_{k > 1} A[y_{k-1}][y_k] + end[y_n]),
 * and log Z_b = 0 with zero gradients for an empty chain.  The CRF loss of a (partly) labelled sequence is
 * log Z(every chain row free) - log Z(labelled rows constrained): a fully labelled sequence makes the second term the gold path's
 * score, an unlabelled residue is marginalised over.
 *
 * Forward.  alpha_1[j] = start[j] + e[t_1][j];  alpha_k[j] = e[t_k][j] + log sum_i exp(alpha_{k-1}[i] + A[i][j]), fp32 in the log
 * domain: per target label j the maximum over the predecessors i is exact and the sum of exp(. - max) runs in ascending i.  A constrained
 * row sets the other labels' alpha to -inf.  log Z_b = log sum_j exp(alpha_n[j] + end[j]), the same way.
 * Backward.  beta_n[i] = end[i];  beta_k[i] = log sum_j exp(A[i][j] + e[t_{k+1}][j] + beta_{k+1}[j]) over the labels j that row
 * t_{k+1} allows.  d_e[t_k][c] = grad_b exp(alpha_k[c] + beta_k[c] - log Z_b); d_transitions[i][j] = sum_b grad_b sum_k
 * exp(alpha_k[i] + A[i][j] + e[t_{k+1}][j] + beta_{k+1}[j] - log Z_b); d_start / d_end = sum_b of the first / last chain row's d_e.
 * The sums over sequences: sequence b belongs to part b % P with P = min(B, ESME_HIP_CRF_PARTS) (a function of B alone); a part adds
 * its sequences in ascending b in fp32, and the parts are added in ascending order.  No atomics: every output is bit-equal from run
 * to run, and log Z_b, the d_e rows, the path and the score of a sequence depend on that sequence's rows alone.
 * Decode.  Max-plus Viterbi under the same constraints.  Ties: the lowest predecessor index wins at every step, and the lowest final
 * label.  The score is the best path's score, 0 for an empty chain.
 * Non-finite emissions.  A NaN, or a +inf, emission on a chain row makes log Z_b, the d_e chain rows and the decoded score of ITS
 * sequence NaN, whichever label it sits at and whatever the row's constraint, and through the sums over sequences
 * d_transitions, d_start and d_end.  It touches no other sequence's rows.  (-inf emissions forbid a label, as -inf transitions do.)
 */
#ifndef ESME_HIP_CRF_H
#define ESME_HIP_CRF_H

#include "esme_hip.h"   /* ESME_OK / ESME_ERR_*, esme_hip_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

/* tags[t]: the row is in the chain, every label allowed. */
#define ESME_HIP_CRF_FREE -1
/* tags[t]: the row is not in the chain (any value below -1 or at least C acts the same). */
#define ESME_HIP_CRF_SKIP -2
/* Largest number of labels: one lane of a wavefront per label. */
#define ESME_HIP_CRF_MAX_C 64
/* Largest number of parts of the sums over sequences (part of the summation order): P = min(B, ESME_HIP_CRF_PARTS). */
#define ESME_HIP_CRF_PARTS 1024

/* Workspace of the backward in bytes: P (C C + 2 C) floats, P = min(B, ESME_HIP_CRF_PARTS).  Needs no initialisation.  B == 0: 0.
 * B, T < 0: ESME_ERR_ARG; C outside 1 .. 64 or T >= 2^31: ESME_ERR_UNSUPPORTED (negative returns). */
int64_t esme_hip_crf_bwd_workspace_bytes(int64_t B, int64_t T, int C);
/* Workspace of the decoder in bytes: the back-pointers, one byte per (row, label), rounded up to 16.  Needs no initialisation. */
int64_t esme_hip_crf_decode_workspace_bytes(int64_t T, int C);

/* emissions: rows [0, T) of C fp32 with row stride ld_e (>= C); transitions (C, C), start (C), end (C) fp32 contiguous; cu_lens
 * (B + 1) int32, ascending, cu_lens[0] >= 0, cu_lens[B] <= T; tags (T) int32.  Outputs, all written: logz (B) fp32; alpha (T, C) fp32
 * contiguous, the forward variables of chain rows and zeros on every other row.  Every pointer 16-byte aligned.
 * B == 0 or T == 0: OK (T == 0 with B > 0 writes logz = 0; emissions, tags and alpha may then be null).  With B == 0 no row belongs
 * to a sequence and the three entry points write NO row of alpha, d_emissions or path (the binding zeroes / fills them); the
 * parameter gradients are still written, as zeros. */
int esme_hip_crf_fwd(const float* emissions, int64_t ld_e, const float* transitions, const float* start, const float* end,
                     const int32_t* cu_lens, const int32_t* tags, int64_t B, int64_t T, int C, float* logz, float* alpha, void* stream);

/* alpha, logz: what the forward wrote on the same operands.  grad (B) fp32: the upstream gradient of logz, on the device.
 * d_emissions: rows [0, T) of C fp32 with row stride ld_de (>= C), every row written (zeros outside chains).
 * want_params: d_transitions (C, C), d_start (C), d_end (C) fp32 contiguous, every element written (zeros when B == 0). */
int esme_hip_crf_bwd(const float* emissions, int64_t ld_e, const float* transitions, const float* start, const float* end,
                     const int32_t* cu_lens, const int32_t* tags, int64_t B, int64_t T, int C, const float* alpha, const float* logz,
                     const float* grad, float* d_emissions, int64_t ld_de, int want_params, float* d_transitions, float* d_start,
                     float* d_end, void* workspace, int64_t ws_bytes, void* stream);

/* path (T): int64 (path_i64 != 0) or int32, the best label of every chain row and `fill` on the rows outside chains; score (B) fp32.
 * workspace: esme_hip_crf_decode_workspace_bytes(T, C) bytes. */
int esme_hip_crf_decode(const float* emissions, int64_t ld_e, const float* transitions, const float* start, const float* end,
                        const int32_t* cu_lens, const int32_t* tags, int64_t B, int64_t T, int C, void* path, int path_i64, int64_t fill,
                        float* score, void* workspace, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
