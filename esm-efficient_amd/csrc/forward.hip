// esme_hip_forward / _half / _exact: the whole packed forward (L transformer layers, final LayerNorm, LM head) enqueued by ONE call.
//
// Host-only code: it issues exactly the launches the Python modules issue (esme/attention.py, esme/esm.py, esme/head.py
// in this repository, which mirror the reference's esme/attention.py:241-255, esme/esm.py:243-252, esme/head.py:25-27),
// through this library's own C entry points, so results are bit-identical to the module-by-module path.  What it
// removes is the host: ~160 ctypes calls (3-10 ms of Python per forward) become one, which is what a small model
// (ESM2-8M / 150M at a few thousand residues: less GPU work than that) needs when it is not replayed from a hipGraph.
//
// Three precision modes share one driver: the workspace arena, the argument prologue, the sequence-order step and the fusion-field
// helpers below.  'fast' (bf16) and 'half' (IEEE fp16 operands, the residual stream as an fp16 pair) run the SAME
// LayerNorm-folded layer, written once in forward_folded; 'exact' (split operands, LayerNorms not folded) keeps a layer body of its own.
// tools/forward_launch_log.cpp records every launch of this file on the CPU; tests/test_forward_launch_log_cpu.py holds it to the log.
#include "launch.h"

using namespace esme;

namespace {

#define ESME_TRY(call) do { if (const int rc_ = (call)) return rc_; } while (0)

enum Mode { FAST, HALF, EXACT };
const char* const kWho[] = {"forward", "forward_half", "forward_exact"};
constexpr float kLog2e = 1.4426950408889634f;

// ---- the caller's workspace: an align-256 bump arena (null base = size query) and the three layouts carved from it
struct Arena {
    char* base;
    int64_t off;
    char* take(int64_t bytes) {
        const int64_t o = off;
        off += (bytes + 255) & ~int64_t(255);
        return base ? base + o : nullptr;
    }
};

struct Ws {
    char* xs;                                  // half: the stream as an fp16 pair [hi | ext | lo]
    char* h;                                   // exact: LayerNorm output pair
    char* qkv; char* attn; char* mid;
    char* head;                                // fast: LM-head scratch
    char* x16;                                 // exact: bf16 rounding of the stream (written by the residual epilogue, unused)
    float* sums; float* part_a; float* part_b; // folded modes: row statistics of the stream
    int32_t* order;                            // dispatch order of the sequences for the attention launches (batches of <= 1024 sequences)
};

int64_t layout(Mode mode, const esme_model_desc_t* m, int64_t T, Ws* out, void* base) {
    const int64_t Ea = (int64_t)m->heads * m->head_pad, Ep = m->phys_dim, F = m->ffn_dim;
    Arena a{(char*)base, 0};
    Ws w{};
    if (mode == EXACT) {
        w.h = a.take(T * 2 * Ep * 2);
        w.attn = Ea == Ep ? w.h : a.take(T * 2 * Ea * 2);       // attention output pair (shares the LayerNorm pair's buffer when the widths agree)
        w.qkv = a.take(T * 6 * Ea * 2);                         // [q k v hi | q k v lo]
        w.mid = a.take(T * 2 * F * 2);
        w.x16 = a.take(T * Ep * 2);
    } else {
        const int64_t nblk = esme_hip_gemm_stats_blocks(T, (int)Ep);
        if (mode == HALF) {
            w.xs = a.take(T * (2 * Ep + (m->half_ext_n > 0 ? 64 : 0)) * 2);
            w.qkv = a.take(T * (3 + (m->half_qk_pair ? 2 : 0)) * Ea * 2);      // [q k v | q_lo k_lo] when q / k travel as pairs
        } else {
            w.qkv = a.take(T * 3 * Ea * 2);
        }
        w.attn = a.take(T * Ea * 2);
        w.mid = a.take(T * F * 2);                              // output columns of the FFN up-projection (F)
        if (mode == FAST) w.head = a.take(m->head_dense_w ? T * Ep * 2 : 0);   // LM-head scratch only when the descriptor carries the head (logits != NULL)
        w.sums = (float*)a.take(T * 2 * 4);
        w.part_a = (float*)a.take(nblk * T * 2 * 4);
        w.part_b = (float*)a.take(nblk * T * 2 * 4);
    }
    w.order = (int32_t*)a.take(1024 * 4);
    if (out) *out = w;
    return a.off;
}

int64_t workspace_bytes(Mode mode, const esme_model_desc_t* m, int64_t T) { return !m || T < 0 ? -1 : layout(mode, m, T, nullptr, nullptr); }

int refuse(Mode mode, const char* what, const char* note = "") {
    snprintf(error_buffer(), kErrorBufferSize, "%s: %s%s", kWho[mode], what, note);
    return ESME_ERR_ARG;
}

// ---- the argument checks of an entry, in one order for the three modes.  Returns 1 when there is nothing to do (T == 0).
// `pair` / ld_pair: the output of the half and exact entries (they also need at least one layer).
int prologue(Mode mode, const esme_model_desc_t* m, const void* x, int64_t ldx, const int32_t* cu_lens, int B, int64_t T, int max_len, const int32_t* pos,
             const void* workspace, int64_t ws_bytes, const void* pair, int64_t ld_pair) {
    const bool fast = mode == FAST;
    if (!(m && m->struct_bytes == (int)sizeof(esme_model_desc_t))) return refuse(mode, "descriptor missing or of another ABI");
    if (!(T >= 0 && B >= 0 && max_len >= 0)) return refuse(mode, "bad sizes");
    if (T == 0) return 1;
    if (!(x && cu_lens && workspace && (fast || pair) && m->layers && m->n_layers >= (fast ? 0 : 1))) return refuse(mode, "null pointer");
    if (!(m->phys_dim % 64 == 0 && m->embed_dim > 0 && m->embed_dim <= m->phys_dim && ldx >= m->phys_dim && (fast || ld_pair >= 2 * (int64_t)m->phys_dim)))
        return refuse(mode, "the physical width must be a multiple of 64", fast ? " (LayerNorm-folded path)" : ", ld_pair >= 2 * phys_dim");
    if (mode == HALF && !(m->half_ext_n >= 0 && m->half_ext_n <= 64 && (m->half_ext_n == 0 || m->half_ext_sel)))
        return refuse(mode, "half_ext_n in [0, 64] with its channel list");
    if (!(ws_bytes >= layout(mode, m, T, nullptr, nullptr) && aligned16(workspace))) return refuse(mode, "workspace too small or misaligned");
    if (!(!m->rotary || (m->cos && m->sin && pos))) return refuse(mode, mode == EXACT ? "rotary models need (fp32) cos, sin and pos" : "rotary models need cos, sin and pos");
    if (mode == HALF && !(!m->half_qk_pair || !m->rotary || (m->cos32 && m->sin32))) return refuse(mode, "q/k pairs need the fp32 rotary tables cos32 / sin32");
    return ESME_OK;
}
#define ESME_PROLOGUE(...) do { if (const int rc_ = prologue(__VA_ARGS__)) return rc_ > 0 ? ESME_OK : rc_; } while (0)

// longest sequences first in every attention launch (speed only; ragged batches), computed once per forward
int sequence_order(const int32_t* cu_lens, int B, int32_t* buffer, void* stream, const int32_t** order) {
    *order = nullptr;
    if (B > 1 && B <= 1024) {
        ESME_TRY(esme_hip_seq_order(cu_lens, B, buffer, stream));
        *order = buffer;
    }
    return ESME_OK;
}

// rotary in a QKV projection's epilogue: the q and k column blocks, with the given tables
void rotary_fields(esme_gemm_fusion_t& f, const esme_model_desc_t* m, const void* cos, const void* sin, const int32_t* pos) {
    f.cos = cos; f.sin = sin; f.pos = pos; f.head_dim = m->head_pad; f.max_len = m->table_len; f.rot_cols = 2 * m->heads * m->head_pad;
}

// LayerNorm folded into the projection that reads the stream: its row statistics and the weight's c1 / c2
void ln_fields(esme_gemm_fusion_t& f, const esme_model_desc_t* m, const float* partial, int nblk, const float* c1, const float* c2) {
    f.ln_partial = partial; f.ln_nblk = nblk; f.ln_dim = m->embed_dim; f.ln_eps = m->ln_eps; f.ln_c1 = c1; f.ln_c2 = c2;
}

// ---- 'fast' and 'half': the LayerNorm-folded layer stack.
// fast: bf16 operands, the stream is `x` (T, phys_dim) itself, updated in place; the tail is the in-place final LayerNorm + optional LM head.
// half: IEEE fp16 operands.  The descriptor's layer weights are then the fp16 copies (W' = fp16(W diag(gamma)) with ITS row sums c1; out / down
// weights converted exactly from bf16), cos / sin are fp16 tables.  `x` is the fp32 stream at the start (embedding rows; ESM-1b / 1v: token +
// position sums); the stream lives in the workspace as an fp16 pair [hi | ext | lo]; the result is the final LayerNorm in the split-operand form:
// `pair` (T, 2 * phys_dim) bf16 = [hi | lo] (the LM head's operand, esme/head.py forward_exact) and, when rep32 != NULL, its fp32 value.
// Same launches as the module-by-module path (esme/attention.py forward / forward_high_precision with ctx.f16): bit-identical.
int forward_folded(Mode mode, const esme_model_desc_t* m, void* x, int64_t ldx, const int32_t* cu_lens, int B, int64_t T, int max_len, const int32_t* pos,
                   void* workspace, void* logits, int64_t ld_logits, void* pair, int64_t ld_pair, float* rep32, int64_t ld_rep, void* stream) {
    const bool half = mode == HALF;
    Ws w;
    layout(mode, m, T, &w, workspace);
    const int Ep = m->phys_dim, E = m->embed_dim, H = m->heads, dp = m->head_pad;
    const int64_t Ea = (int64_t)H * dp;
    const int nblk = esme_hip_gemm_stats_blocks(T, Ep);
    const bool rot_fused = m->rotary && !m->qk_norm && (dp == 16 || dp == 32 || dp == 64) && Ea % 32 == 0;
    const bool qk_pair = half && m->half_qk_pair != 0;
    if (qk_pair && (m->qk_norm || !(dp == 16 || dp == 32 || dp == 64) || Ea % 128 != 0))
        ESME_FAIL(ESME_ERR_UNSUPPORTED, "forward_half: q/k pairs cover blocks without q/k LayerNorm, head dim 16 / 32 / 64, heads * head_pad a multiple of 128");
    // half with massive stream channels: the pair rows carry the extension K-tile [hi | ext | lo]; the LayerNorm-folded GEMMs read [hi | ext]
    const int ext = half && m->half_ext_n > 0 ? 64 : 0;
    const int64_t lo_off = (int64_t)Ep + ext;
    void* const xs = half ? w.xs : x;                      // the operand the folded GEMMs read and the residual epilogues update in place
    const int64_t ldxs = half ? 2 * (int64_t)Ep + ext : ldx;
    const int Kf = Ep + ext;
    // head dim 64 / 32 with fused rotary (ESM2-650M / 3B / 150M) or ESM-C's q/k pass: softmax_scale * log2(e) rides in q and the attention kernel
    // runs without a reference maximum (esme_attn_opts_t.q_prescaled; half: the fixed-reference form, in the layers without q / k pairs); the caller
    // says so in the descriptor (no environment switch in the library: the module-by-module path must take the same decision to stay bit-identical).
    const bool qp = m->attn_q_prescale && m->rotary && (dp == 64 || dp == 32) && Ea % 64 == 0 && (rot_fused || m->qk_norm);
    const float qs = m->softmax_scale * kLog2e;
    esme_attn_opts_t aopts{(int)sizeof(esme_attn_opts_t), 0, 0, 8.0f, 1, nullptr, qp ? 1 : 0, half ? 1 : 0};
    if (m->n_layers > 0) ESME_TRY(sequence_order(cu_lens, B, w.order, stream, &aopts.seq_order));
    // statistics describing the current residual stream; half: first the stream as an fp16 pair, scaled per column for the first folded GEMM
    const float* stats = w.sums;
    int stats_nblk = 1;
    if (half)
        ESME_TRY(esme_hip_stream_operand_guarded((const float*)x, ldx, xs, ldxs, lo_off, 1, m->layers[0].ps_attn, ext ? m->half_ext_sel : nullptr, m->half_ext_n,
                                                 ext ? Ep : 0, w.sums, m->half_col_absmax, T, Ep, stream));
    else if (m->n_layers > 0)
        ESME_TRY(esme_hip_row_sums(x, ldx, T, Ep, w.sums, stream));
    // a LayerNorm-folded projection off the stream / a residual epilogue onto it (half: the pair stream arrives scaled by 1 / s_in, leaves scaled by
    // s_out; `guard_row` of the plan guard's column maxima)
    auto folded = [&](esme_gemm_fusion_t& f, const float* c1, const float* c2) {
        if (half) { f.f16 = 1; f.overflow_flag = m->half_overflow_flag; }
        ln_fields(f, m, stats, stats_nblk, c1, c2);
    };
    auto residual = [&](const void* a, int64_t lda, const void* wt, const void* bias, int K, float* stats_out, const float* s_in, const float* s_out, int guard_row) {
        esme_gemm_fusion_t f{};
        f.stats_out = stats_out;
        if (half) {
            f.f16 = 1; f.pair_off = lo_off;
            if (ext) { f.ext_sel = m->half_ext_sel; f.ext_n = m->half_ext_n; f.ext_off = Ep; }
            f.pair_scale_in = s_in; f.pair_scale_out = s_out;
            if (m->half_col_absmax) f.col_absmax = m->half_col_absmax + (int64_t)guard_row * Ep;
        }
        return esme_hip_gemm_bf16_fused(a, lda, wt, bias, xs, ldxs, xs, ldxs, T, Ep, K, ESME_EPI_RESIDUAL, m->alpha, &f, stream);
    };
    for (int i = 0; i < m->n_layers; ++i) {
        const esme_layer_weights_t& L = m->layers[i];
        // ---- attention branch: LN-folded fused QKV (+ rotary), varlen attention, out-projection + residual + statistics
        esme_gemm_fusion_t fu{};
        folded(fu, L.qkv_c1, L.qkv_c2);
        char* q = w.qkv; char* k = w.qkv + Ea * 2; char* v = w.qkv + 2 * Ea * 2;
        if (qk_pair && L.half_qk_pair) {
            // large attention scores in THIS layer: q / k as fp16 pairs [q k v | q_lo k_lo], rotated with fp32 tables, scores from three MFMA passes
            fu.pair_off = 3 * Ea; fu.pair_cols = (int)(2 * Ea);
            if (m->rotary) rotary_fields(fu, m, m->cos32, m->sin32, pos);
            ESME_TRY(esme_hip_gemm_bf16_fused(xs, ldxs, L.qkv_w, nullptr, nullptr, 0, w.qkv, 5 * Ea, T, (int)(3 * Ea), Kf, ESME_EPI_NONE, 1.0f, &fu, stream));
            ESME_TRY(esme_hip_attn_varlen_fwd_qkpair_f16(q, k, v, 5 * Ea, 3 * Ea, w.attn, Ea, cu_lens, B, T, H, dp, max_len, m->softmax_scale, aopts.seq_order, stream));
        } else {
            uint32_t* const gq = half && m->half_qk_sumsq ? m->half_qk_sumsq + (int64_t)i * 2 * H : nullptr;      // plan guard: this layer's q / k row norms
            if (rot_fused) { rotary_fields(fu, m, m->cos, m->sin, pos); fu.qk_sumsq = gq; }
            if (qp && rot_fused) { fu.q_scale = qs; fu.q_cols = (int)Ea; }
            ESME_TRY(esme_hip_gemm_bf16_fused(xs, ldxs, L.qkv_w, nullptr, nullptr, 0, w.qkv, 3 * Ea, T, (int)(3 * Ea), Kf, ESME_EPI_NONE, 1.0f, &fu, stream));
            if (m->qk_norm) {                                // ESM-C: the q/k-norm pass folds the scale in
                if (!half) ESME_TRY(esme_hip_qk_norm_rotary_scaled(q, k, 3 * Ea, L.lnq_w, L.lnk_w, L.lnq_b, L.lnk_b, m->ln_eps, m->cos, m->sin, pos, T, H, dp, m->table_len, qp ? qs : 1.0f, stream));
                else if (qp) ESME_TRY(esme_hip_qk_norm_rotary_f16_scaled(q, k, 3 * Ea, L.lnq_w, L.lnk_w, L.lnq_b, L.lnk_b, m->ln_eps, m->cos, m->sin, pos, T, H, dp, m->table_len, qs, gq, stream));
                else ESME_TRY(esme_hip_qk_norm_rotary_f16_guarded(q, k, 3 * Ea, L.lnq_w, L.lnk_w, L.lnq_b, L.lnk_b, m->ln_eps, m->cos, m->sin, pos, T, H, dp, m->table_len, gq, stream));
            } else if (m->rotary && !rot_fused) {
                ESME_TRY((half ? esme_hip_rotary_varlen_f16 : esme_hip_rotary_varlen)(q, k, 3 * Ea, m->cos, m->sin, pos, T, H, dp, m->table_len, stream));
            }
            ESME_TRY(esme_hip_attn_varlen_fwd_opts(q, k, v, 3 * Ea, w.attn, Ea, cu_lens, B, T, H, dp, max_len, m->softmax_scale, &aopts, stream));
        }
        // (half: the stream arrives scaled for this layer's attention LayerNorm, leaves scaled for its FFN LayerNorm)
        ESME_TRY(residual(w.attn, Ea, L.out_w, L.out_b, (int)Ea, w.part_b, L.ps_attn_inv, L.ps_ffn, 2 * i + 1));
        stats = w.part_b; stats_nblk = nblk;
        // ---- FFN branch: LN-folded up-projection with GELU / SiLU*mul, down-projection + residual + statistics
        esme_gemm_fusion_t fup{};
        folded(fup, L.up_c1, L.up_c2);
        ESME_TRY(esme_hip_gemm_bf16_fused(xs, ldxs, L.up_w, nullptr, nullptr, 0, w.mid, m->ffn_dim, T, m->swiglu ? 2 * m->ffn_dim : m->ffn_dim, Kf,
                                          m->swiglu ? ESME_EPI_SWIGLU : ESME_EPI_GELU, 1.0f, &fup, stream));
        // (half: the next layer's attention scaling; the final LayerNorm reads the stream unscaled)
        ESME_TRY(residual(w.mid, m->ffn_dim, L.down_w, L.down_b, m->ffn_dim, w.part_a, L.ps_ffn_inv, i + 1 < m->n_layers ? m->layers[i + 1].ps_attn : nullptr, 2 * i + 2));
        stats = w.part_a;
    }
    if (half)   // final LayerNorm over the logical width, from the fp16 pair, written as the bf16 pair the split-operand LM head reads (+ fp32)
        return esme_hip_layernorm_split_checked(xs, ldxs, 2, lo_off, m->final_ln_w, m->final_ln_b, pair, ld_pair, Ep, rep32, ld_rep, T, E, m->ln_eps, m->half_overflow_flag, stream);
    // ---- final LayerNorm over the logical width (pad columns stay zero), in place
    ESME_TRY(esme_hip_layernorm(x, ldx, m->final_ln_w, m->final_ln_b, x, ldx, T, E, m->ln_eps, stream));
    if (!logits) return ESME_OK;
    // ---- RobertaLMHead: dense + GELU, LayerNorm, vocab projection
    ESME_CHECK_ARG(m->head_dense_w && m->head_ln_w && m->head_final_w && m->vocab > 0 && ld_logits >= m->vocab, "forward: LM head weights missing");
    ESME_TRY(esme_hip_gemm_bf16(x, ldx, m->head_dense_w, m->head_dense_b, nullptr, 0, w.head, Ep, T, Ep, Ep, ESME_EPI_GELU, 1.0f, stream));
    ESME_TRY(esme_hip_layernorm(w.head, Ep, m->head_ln_w, m->head_ln_b, w.head, Ep, T, E, m->ln_eps, stream));
    return esme_hip_gemm_bf16(w.head, Ep, m->head_final_w, m->head_final_b, nullptr, 0, logits, ld_logits, T, m->vocab, Ep, ESME_EPI_NONE, 1.0f, stream);
}

}  // namespace

extern "C" int64_t esme_hip_forward_workspace_bytes(const esme_model_desc_t* m, int64_t T) { return workspace_bytes(FAST, m, T); }
extern "C" int64_t esme_hip_forward_half_workspace_bytes(const esme_model_desc_t* m, int64_t T) { return workspace_bytes(HALF, m, T); }
extern "C" int64_t esme_hip_forward_exact_workspace_bytes(const esme_model_desc_t* m, int64_t T) { return workspace_bytes(EXACT, m, T); }

extern "C" int esme_hip_forward(const esme_model_desc_t* m, void* x, int64_t ldx, const int32_t* cu_lens, int B, int64_t T,
                                int max_len, const int32_t* pos, void* workspace, int64_t ws_bytes, void* logits,
                                int64_t ld_logits, void* stream) {
    ESME_PROLOGUE(FAST, m, x, ldx, cu_lens, B, T, max_len, pos, workspace, ws_bytes, nullptr, 0);
    return forward_folded(FAST, m, x, ldx, cu_lens, B, T, max_len, pos, workspace, logits, ld_logits, nullptr, 0, nullptr, 0, stream);
}

extern "C" int esme_hip_forward_half(const esme_model_desc_t* m, const float* x32, int64_t ld32, const int32_t* cu_lens, int B, int64_t T,
                                     int max_len, const int32_t* pos, void* workspace, int64_t ws_bytes, void* pair, int64_t ld_pair,
                                     float* rep32, int64_t ld_rep, void* stream) {
    ESME_PROLOGUE(HALF, m, x32, ld32, cu_lens, B, T, max_len, pos, workspace, ws_bytes, pair, ld_pair);
    return forward_folded(HALF, m, const_cast<float*>(x32), ld32, cu_lens, B, T, max_len, pos, workspace, nullptr, 0, pair, ld_pair, rep32, ld_rep, stream);
}

// ---- split-operand ('exact') mode: the same layer stack with every activation operand as a (hi, lo) bf16 pair on an fp32
// residual stream, through one call.  Mirrors esme/attention.py FlashTransformerLayer.forward_exact launch for launch.
extern "C" int esme_hip_forward_exact(const esme_model_desc_t* m, float* x32, int64_t ld32, const int32_t* cu_lens, int B, int64_t T,
                                      int max_len, const int32_t* pos, void* workspace, int64_t ws_bytes, void* pair, int64_t ld_pair,
                                      float* rep32, int64_t ld_rep, void* stream) {
    ESME_PROLOGUE(EXACT, m, x32, ld32, cu_lens, B, T, max_len, pos, workspace, ws_bytes, pair, ld_pair);
    const int Ep = m->phys_dim, E = m->embed_dim, H = m->heads, dp = m->head_pad, F = m->ffn_dim;
    const int64_t Ea = (int64_t)H * dp;
    if (dp != 16 && dp != 32 && dp != 64 && dp != 128) ESME_FAIL(ESME_ERR_UNSUPPORTED, "forward_exact: head dims 16, 32, 64 and 128");
    Ws w;
    layout(EXACT, m, T, &w, workspace);
    const bool rot_fused = m->rotary && !m->qk_norm && dp <= 64 && Ea % 64 == 0;      // (head dim 128: esme_hip_rotary_split)
    const int32_t* order;
    ESME_TRY(sequence_order(cu_lens, B, w.order, stream, &order));
    auto residual = [&](const void* a, const void* wt, const void* bias, int K) {       // fp32 accumulators added straight into the fp32 stream
        esme_gemm_fusion_t f{};
        f.w_k = K; f.resid32 = x32; f.ld32 = ld32;
        return esme_hip_gemm_bf16_fused(a, 2 * (int64_t)K, wt, bias, nullptr, 0, w.x16, Ep, T, Ep, 2 * K, ESME_EPI_RESIDUAL, m->alpha, &f, stream);
    };
    for (int i = 0; i < m->n_layers; ++i) {
        const esme_layer_weights_t& L = m->layers[i];
        ESME_CHECK_ARG(L.ln1_w && L.ln2_w && L.qkv_w && L.out_w && L.up_w && L.down_w, "forward_exact: the descriptor needs the plain weights and the LayerNorm parameters");
        // ---- attention branch
        ESME_TRY(esme_hip_layernorm_split(x32, ld32, 0, 0, L.ln1_w, L.ln1_b, w.h, 2 * (int64_t)Ep, Ep, nullptr, 0, T, E, m->ln_eps, stream));
        esme_gemm_fusion_t fq{};
        fq.w_k = Ep; fq.pair_off = 3 * Ea;
        if (rot_fused) rotary_fields(fq, m, m->cos, m->sin, pos);
        ESME_TRY(esme_hip_gemm_bf16_fused(w.h, 2 * (int64_t)Ep, L.qkv_w, L.qkv_b, nullptr, 0, w.qkv, 6 * Ea, T, (int)(3 * Ea), 2 * Ep, ESME_EPI_NONE, 1.0f, &fq, stream));
        if (m->qk_norm) {                    // ESM-C: q / k LayerNorm over the full width, pair in -> pair out, in place
            ESME_TRY(esme_hip_layernorm_split(w.qkv, 6 * Ea, 1, 3 * Ea, L.lnq_w, L.lnq_b, w.qkv, 6 * Ea, 3 * Ea, nullptr, 0, T, (int)Ea, m->ln_eps, stream));
            ESME_TRY(esme_hip_layernorm_split(w.qkv + Ea * 2, 6 * Ea, 1, 3 * Ea, L.lnk_w, L.lnk_b, w.qkv + Ea * 2, 6 * Ea, 3 * Ea, nullptr, 0, T, (int)Ea, m->ln_eps, stream));
        }
        if (m->rotary && !rot_fused)
            ESME_TRY(esme_hip_rotary_split(w.qkv, 6 * Ea, 3 * Ea, (const float*)m->cos, (const float*)m->sin, pos, T, 2 * H, dp, m->table_len, stream));
        ESME_TRY(esme_hip_attn_varlen_fwd_split(w.qkv, w.qkv + Ea * 2, w.qkv + 2 * Ea * 2, 6 * Ea, 3 * Ea, w.attn, 2 * Ea, Ea, cu_lens, B, T, H, dp, max_len,
                                                m->softmax_scale, order, stream));
        ESME_TRY(residual(w.attn, L.out_w, L.out_b, (int)Ea));
        // ---- FFN branch
        ESME_TRY(esme_hip_layernorm_split(x32, ld32, 0, 0, L.ln2_w, L.ln2_b, w.h, 2 * (int64_t)Ep, Ep, nullptr, 0, T, E, m->ln_eps, stream));
        esme_gemm_fusion_t fu{};
        fu.w_k = Ep; fu.pair_off = F;
        ESME_TRY(esme_hip_gemm_bf16_fused(w.h, 2 * (int64_t)Ep, L.up_w, L.up_b, nullptr, 0, w.mid, 2 * (int64_t)F, T, m->swiglu ? 2 * F : F, 2 * Ep,
                                          m->swiglu ? ESME_EPI_SWIGLU : ESME_EPI_GELU, 1.0f, &fu, stream));
        ESME_TRY(residual(w.mid, L.down_w, L.down_b, F));
    }
    return esme_hip_layernorm_split(x32, ld32, 0, 0, m->final_ln_w, m->final_ln_b, pair, ld_pair, Ep, rep32, ld_rep, T, E, m->ln_eps, stream);
}
