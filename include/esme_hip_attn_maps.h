/* Attention maps of chosen heads of one layer, written out (libesme_hip.so, gfx950).
 *
 * fair-esm's need_head_weights=True and Hugging Face's output_attentions=True return the softmax weights of every head; the
 * reference package cannot (flash_attn_varlen_func gives none back), and the contact entry points of this library reduce the maps
 * as they are produced, so that no S x S object is ever stored.  This entry point is for the user who wants the maps themselves:
 * one head of one layer of one protein, a head average, or a feature the contact head does not have.
 *
 * Definition.  One packed sequence of S rows, head h:
 *     P^(h)_ij = softmax_j((q_i . k_j) * softmax_scale) over ALL S keys.
 * Rows and columns of bos / eos are included; nothing is trimmed (the caller slices).  q and k are the bf16 operands that layer's
 * attention kernel consumes (post-rotary; ESM-C: post-q/k-LayerNorm).
 *
 * Output.  head_list names the n_heads heads to produce, in that order.
 *   head_weights == NULL:  map j of the call (head head_list[j]) of sequence s is the row-major S_s x S_s block at
 *                          map + map_off[s] + (slot0 + j) * S_s^2   (elements, 64-bit).
 *   head_weights != NULL:  ONE block per sequence, at slot slot0, holding sum_j head_weights[j] * P^(head_list[j]); the heads are
 *                          summed in list order in fp32 (acc = fma(w_j, P_j, acc) from acc = 0).
 * A model that wants n_out blocks per layer calls the entry once per selected layer with slot0 = i * n_out for its i-th selected
 * layer and map_off[s] = (sum of L_sel * n_out * S_t^2 over the sequences t before s): a sequence's blocks are then one
 * (L_sel, n_out, S_s, S_s) tensor.  Every element of every block the call owns is written (the output needs no initialisation);
 * nothing else is.  An empty sequence owns nothing.
 *
 * Arithmetic: scores on the bf16 MFMA (16x16x32) with fp32 accumulators; the softmax in fp32 in log2 units (exp2) with the exact
 * row maximum and row sum over all keys (never a tile-local maximum); P = exp2(s - m) * (1 / l) is rounded once: fp32 output stores
 * it as it is, bf16 output its round-to-nearest-even image (weighted mode: the fp32 head sum is rounded once).
 * Two launches per call: attn_map_stats_kernel (per sequence, listed head and 64 query rows: all key tiles twice -> m, l in the
 * workspace) and attn_map_write_kernel (per sequence, block and 64 x 64 tile: the scores again, normalised and stored).
 * No floating-point atomics, every reduction has a fixed order and every index is relative to the sequence's own first row: a
 * sequence's maps are bit-identical alone and packed, from run to run, and for any head_list that contains the head.  No row outside
 * [cu_lens[s], cu_lens[s + 1]) is read for sequence s.
 */
#ifndef ESME_HIP_ATTN_MAPS_H
#define ESME_HIP_ATTN_MAPS_H

#include "esme_hip_contacts.h"   /* ESME_OK / ESME_ERR_*, ESME_HIP_CONTACT_MAX_SEQ_ELEMS */

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of one esme_hip_attn_maps call, in bytes:  2 * n_heads * T * sizeof(float)
 * -- per listed head and packed row the row maximum (log2 units) and the row sum.  It needs no initialisation and carries nothing
 * from one call to the next.  Negative sizes or n_heads <= 0: ESME_ERR_ARG (negative return). */
int64_t esme_hip_attn_maps_workspace_bytes(int B, int64_t T, int n_heads);

/* q, k: (T, H, d) bf16 views with ONE row stride ld_qk (column blocks of the fused (T, 3E) projection).  16-byte aligned q and k,
 * ld_qk % 8 == 0, ld_qk >= H * d (else ESME_ERR_ARG).  d in {16, 32, 64, 128} (else ESME_ERR_UNSUPPORTED); a padded layout passes
 * its physical d (pad lanes zero) and the softmax_scale of the logical head dim.
 * q_prescaled != 0: q already carries softmax_scale * log2(e); softmax_scale is then ignored.
 * cu_lens: int32 (B + 1) on the device; T < 2^31; any B (more than 65 535 sequences run as several launches); max_len >= the longest
 * sequence (rows past max_len are not processed) and max_len * ld_qk < ESME_HIP_CONTACT_MAX_SEQ_ELEMS (else ESME_ERR_UNSUPPORTED).
 * head_list: int32 (n_heads) on the device, each in [0, H); NOT validated here (the caller does).  0 < n_heads <= 65 535.
 * head_weights: NULL, or float (n_heads) on the device (see above).
 * map: float (out_bf16 == 0, 4-byte aligned) or bf16 (out_bf16 != 0, 2-byte aligned) on the device; map_off: int64 (B) on the
 * device, in elements; slot0 >= 0.
 * workspace: esme_hip_attn_maps_workspace_bytes(B, T, n_heads) bytes, 16-byte aligned.  All checks run before any launch.
 * B == 0 or T == 0 is a no-op. */
int esme_hip_attn_maps(const void* q, const void* k, int64_t ld_qk, const int32_t* cu_lens, int B, int64_t T, int H, int d,
                       int max_len, float softmax_scale, int q_prescaled, const int32_t* head_list, int n_heads,
                       const float* head_weights, void* map, int out_bf16, const int64_t* map_off, int64_t slot0,
                       void* workspace, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
