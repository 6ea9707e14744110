/* Residue-contact logits from the attention maps, without materialising the maps (libesme_hip.so, gfx950).
 *
 * ESM-2's contact head (Rao et al. 2021) is a logistic regression over the symmetrised, APC-corrected attention maps of all
 * layers and heads.  The reference package dropped it with its move to flash_attn_varlen_func, which returns no attention
 * weights; the original implementation stores an (L H, S, S) fp32 tensor per protein.  Everything the head needs from one map is
 * linear in that map apart from one rank-1 term, so the maps are reduced into ONE (n x n) logit map per protein as they are produced.
 *
 * Definition.  One packed sequence of S rows; f = trim_front, e = trim_back, n = max(S - f - e, 0).  Per head h of the layer:
 *     P = softmax_j((q_i . k_j) * softmax_scale) over ALL S keys (the trimmed rows stay in the softmax),
 *     A = P[f : S - e, f : S - e],   Y = A + A^T,   r_i = sum_j Y_ij,   t = sum_i r_i,   N = Y - r r^T / t,
 *     map += sum_h w[h] N^(h)        (the call with init != 0 writes bias + sum_h ... instead of adding).
 * A model calls esme_hip_contact_layer once per layer, in layer order, with that layer's H regression weights; the map then holds
 * the logits, and sigmoid(map) the contact probabilities.  A sequence with n = 0 produces nothing.
 *
 * Arithmetic: scores on the bf16 MFMA (16x16x32) with fp32 accumulators, softmax in fp32 in log2 units (exp2), P never rounded to
 * bf16; regression weights, r, t and the map are fp32.  No floating-point atomics: heads are summed in index order, layers in call
 * order; a sequence's map does not depend on its neighbours in the batch (bit-identical alone and packed), and it is exactly
 * symmetric (every unordered tile pair is computed once and both halves are written from the same registers).
 * No per-head or per-layer S x S object exists in device memory.
 */
#ifndef ESME_HIP_CONTACTS_H
#define ESME_HIP_CONTACTS_H

#include "esme_hip.h"   /* ESME_OK / ESME_ERR_*, esme_hip_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

/* Rows inside one sequence are addressed with unsigned 32-bit element offsets: max_len * ld_qk must stay below this many elements,
 * else ESME_ERR_UNSUPPORTED. */
#define ESME_HIP_CONTACT_MAX_SEQ_ELEMS 4294967296LL

/* Workspace of one esme_hip_contact_layer call, in bytes:  (3 * H * T + H * B) * sizeof(float)
 * -- per head and packed row the row maximum (log2 units), the row sum and r; per head and sequence t.  O(H T); it needs no
 * initialisation and carries nothing from one call to the next.  Negative sizes or H <= 0: ESME_ERR_ARG (negative return). */
int64_t esme_hip_contact_workspace_bytes(int B, int64_t T, int H);

/* q, k: (T, H, d) bf16 views with ONE row stride ld_qk (column blocks of the fused (T, 3E) projection) -- exactly the operands
 * the attention kernel of that layer consumes (post-rotary; ESM-C: post-q/k-LayerNorm).  Alignment as the attention entry points:
 * 16-byte aligned q and k, ld_qk % 8 == 0, ld_qk >= H * d (else ESME_ERR_ARG).  d in {16, 32, 64, 128} (else ESME_ERR_UNSUPPORTED);
 * a padded layout passes its physical d (pad lanes zero) and the softmax_scale of the logical head dim.
 * q_prescaled != 0: q already carries softmax_scale * log2(e) (esme_attn_opts_t.q_prescaled); softmax_scale is then ignored.
 * cu_lens: int32 (B + 1) on the device; T < 2^31; any B (more than 65 535 sequences run as several launches); max_len >= the longest
 * sequence (rows past max_len are not processed); H <= 65 535; ESME_HIP_CONTACT_MAX_SEQ_ELEMS above.
 * trim_front / trim_back: rows dropped at either end of every sequence (prepend_bos / append_eos), each 0 or more.
 * w: float (H) on the device, this layer's regression weights.  bias and init: init != 0 writes bias + the layer's sum (the map
 * needs no initialisation), init == 0 adds the layer's sum to the map.
 * map: float on the device; sequence s owns the n_s x n_s row-major block at map + map_off[s] (map_off: int64 (B) on the device).
 * workspace: esme_hip_contact_workspace_bytes(B, T, H) bytes, 16-byte aligned.  B == 0 or T == 0 is a no-op. */
int esme_hip_contact_layer(const void* q, const void* k, int64_t ld_qk, const int32_t* cu_lens, int B, int64_t T, int H, int d,
                           int max_len, float softmax_scale, int q_prescaled, int trim_front, int trim_back, const float* w,
                           float bias, int init, float* map, const int64_t* map_off, void* workspace, int64_t ws_bytes,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
