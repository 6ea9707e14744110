// Launch log of the one-call forwards (esme_hip_forward / _half / _exact), on the CPU.
//
// csrc/forward.hip is host-only code: it calls 18 esme_hip_* entries plus esme::error_buffer() and never dereferences a device
// pointer.  This program links its host side against LOGGING STUBS of those entries and runs a table of descriptors through the
// three entries; every stub appends one line (entry name, scalars, every pointer as "buffer+byte offset", every field of the fusion /
// options structs).  The log of a refactored forward.hip must equal the log of the one before, byte for byte:
// tests/test_forward_launch_log_cpu.py compares per-case digests with tests/golden/forward_launch_log.txt.
//
//   hipcc --offload-host-only -std=c++17 -I include -o fll tools/forward_launch_log.cpp esm-efficient_amd/csrc/forward.hip
//   ./fll            every case: "== name" line, then its log
//   ./fll --dump C   the log of case C alone (diff it against a build with another forward.hip)
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/esme_hip.h"

namespace esme {
char* error_buffer() {
    static thread_local char buf[512];
    return buf;
}
}  // namespace esme

namespace {

// ---- fake device buffers: named address ranges that are never dereferenced
constexpr uintptr_t kBase = uintptr_t(1) << 40;
constexpr int kShift = 30;                               // 1 GiB per buffer
std::vector<std::string> g_names;
std::string g_log;
int g_calls = 0;

void* buf(const std::string& name) {
    g_names.push_back(name);
    return reinterpret_cast<void*>(kBase + (uintptr_t(g_names.size() - 1) << kShift));
}

std::string P(const void* p) {
    if (!p) return "null";
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    char tmp[96];
    if (a >= kBase && ((a - kBase) >> kShift) < g_names.size()) {
        snprintf(tmp, sizeof tmp, "+%llu", (unsigned long long)((a - kBase) & ((uintptr_t(1) << kShift) - 1)));
        return g_names[(a - kBase) >> kShift] + tmp;
    }
    snprintf(tmp, sizeof tmp, "?%llx", (unsigned long long)a);
    return tmp;
}

void emit(const char* fmt, ...) {
    char line[4096];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    g_log += line;
    g_log += '\n';
}

#define S(p) P(p).c_str()

std::string fusion(const esme_gemm_fusion_t* f) {
    if (!f) return "fusion=null";
    char t[2048];
    snprintf(t, sizeof t,
             "fusion{ln_partial=%s ln_nblk=%d ln_dim=%d ln_eps=%a ln_c1=%s ln_c2=%s stats_out=%s cos=%s sin=%s pos=%s head_dim=%d max_len=%d "
             "rot_cols=%d resid32=%s ld32=%lld q_scale=%a q_cols=%d w_k=%d pair_off=%lld c32=%s ldc32=%lld f16=%d pair_scale_in=%s "
             "pair_scale_out=%s ext_sel=%s ext_n=%d ext_off=%lld pair_cols=%d overflow_flag=%s col_absmax=%s qk_sumsq=%s}",
             S(f->ln_partial), f->ln_nblk, f->ln_dim, f->ln_eps, S(f->ln_c1), S(f->ln_c2), S(f->stats_out), S(f->cos), S(f->sin), S(f->pos),
             f->head_dim, f->max_len, f->rot_cols, S(f->resid32), (long long)f->ld32, f->q_scale, f->q_cols, f->w_k, (long long)f->pair_off,
             S(f->c32), (long long)f->ldc32, f->f16, S(f->pair_scale_in), S(f->pair_scale_out), S(f->ext_sel), f->ext_n, (long long)f->ext_off,
             f->pair_cols, S(f->overflow_flag), S(f->col_absmax), S(f->qk_sumsq));
    return t;
}

std::string attn_opts(const esme_attn_opts_t* o) {
    if (!o) return "opts=null";
    char t[512];
    snprintf(t, sizeof t, "opts{struct_bytes=%d variant=%d q_blocks=%d defer_max_thr=%a speculative=%d seq_order=%s q_prescaled=%d f16=%d}",
             o->struct_bytes, o->variant, o->q_blocks, o->defer_max_thr, o->speculative, S(o->seq_order), o->q_prescaled, o->f16);
    return t;
}

}  // namespace

// ---- the logging stubs (signatures: include/esme_hip.h)
#define CALL(...) do { ++g_calls; emit(__VA_ARGS__); return ESME_OK; } while (0)
typedef long long ll;

extern "C" {

int esme_hip_gemm_stats_blocks(int64_t, int N) { return (N + 255) / 256 + 1; }       // a fixed function of the shape with nblk > 1

int esme_hip_seq_order(const int32_t* cu, int B, int32_t* order, void* st) { CALL("seq_order cu=%s B=%d order=%s stream=%s", S(cu), B, S(order), S(st)); }

int esme_hip_row_sums(const void* x, int64_t ldx, int64_t T, int E, float* sums, void* st) {
    CALL("row_sums x=%s ldx=%lld T=%lld E=%d sums=%s stream=%s", S(x), (ll)ldx, (ll)T, E, S(sums), S(st));
}

int esme_hip_layernorm(const void* x, int64_t ldx, const void* w, const void* b, void* y, int64_t ldy, int64_t T, int E, float eps, void* st) {
    CALL("layernorm x=%s ldx=%lld w=%s b=%s y=%s ldy=%lld T=%lld E=%d eps=%a stream=%s", S(x), (ll)ldx, S(w), S(b), S(y), (ll)ldy, (ll)T, E, eps, S(st));
}

int esme_hip_stream_operand_guarded(const float* x32, int64_t ld32, void* x16, int64_t ld16, int64_t lo_off, int f16, const float* scale,
                                    const int32_t* ext_sel, int ext_n, int64_t ext_off, float* sums, uint32_t* col_absmax, int64_t T, int E, void* st) {
    CALL("stream_operand_guarded x32=%s ld32=%lld x16=%s ld16=%lld lo_off=%lld f16=%d scale=%s ext_sel=%s ext_n=%d ext_off=%lld sums=%s col_absmax=%s T=%lld E=%d stream=%s",
         S(x32), (ll)ld32, S(x16), (ll)ld16, (ll)lo_off, f16, S(scale), S(ext_sel), ext_n, (ll)ext_off, S(sums), S(col_absmax), (ll)T, E, S(st));
}

int esme_hip_rotary_varlen(void* q, void* k, int64_t ld, const void* cos, const void* sin, const int32_t* pos, int64_t T, int H, int d, int max_len, void* st) {
    CALL("rotary_varlen q=%s k=%s ld=%lld cos=%s sin=%s pos=%s T=%lld H=%d d=%d max_len=%d stream=%s", S(q), S(k), (ll)ld, S(cos), S(sin), S(pos), (ll)T, H, d, max_len, S(st));
}

int esme_hip_rotary_varlen_f16(void* q, void* k, int64_t ld, const void* cos, const void* sin, const int32_t* pos, int64_t T, int H, int d, int max_len, void* st) {
    CALL("rotary_varlen_f16 q=%s k=%s ld=%lld cos=%s sin=%s pos=%s T=%lld H=%d d=%d max_len=%d stream=%s", S(q), S(k), (ll)ld, S(cos), S(sin), S(pos), (ll)T, H, d, max_len, S(st));
}

int esme_hip_qk_norm_rotary_scaled(void* q, void* k, int64_t ld, const void* wq, const void* wk, const void* bq, const void* bk, float eps, const void* cos,
                                   const void* sin, const int32_t* pos, int64_t T, int H, int d, int max_len, float q_scale, void* st) {
    CALL("qk_norm_rotary_scaled q=%s k=%s ld=%lld wq=%s wk=%s bq=%s bk=%s eps=%a cos=%s sin=%s pos=%s T=%lld H=%d d=%d max_len=%d q_scale=%a stream=%s",
         S(q), S(k), (ll)ld, S(wq), S(wk), S(bq), S(bk), eps, S(cos), S(sin), S(pos), (ll)T, H, d, max_len, q_scale, S(st));
}

int esme_hip_qk_norm_rotary_f16_guarded(void* q, void* k, int64_t ld, const void* wq, const void* wk, const void* bq, const void* bk, float eps, const void* cos,
                                        const void* sin, const int32_t* pos, int64_t T, int H, int d, int max_len, uint32_t* qk_sumsq, void* st) {
    CALL("qk_norm_rotary_f16_guarded q=%s k=%s ld=%lld wq=%s wk=%s bq=%s bk=%s eps=%a cos=%s sin=%s pos=%s T=%lld H=%d d=%d max_len=%d qk_sumsq=%s stream=%s",
         S(q), S(k), (ll)ld, S(wq), S(wk), S(bq), S(bk), eps, S(cos), S(sin), S(pos), (ll)T, H, d, max_len, S(qk_sumsq), S(st));
}

int esme_hip_qk_norm_rotary_f16_scaled(void* q, void* k, int64_t ld, const void* wq, const void* wk, const void* bq, const void* bk, float eps, const void* cos,
                                       const void* sin, const int32_t* pos, int64_t T, int H, int d, int max_len, float q_scale, uint32_t* qk_sumsq, void* st) {
    CALL("qk_norm_rotary_f16_scaled q=%s k=%s ld=%lld wq=%s wk=%s bq=%s bk=%s eps=%a cos=%s sin=%s pos=%s T=%lld H=%d d=%d max_len=%d q_scale=%a qk_sumsq=%s stream=%s",
         S(q), S(k), (ll)ld, S(wq), S(wk), S(bq), S(bk), eps, S(cos), S(sin), S(pos), (ll)T, H, d, max_len, q_scale, S(qk_sumsq), S(st));
}

int esme_hip_attn_varlen_fwd_opts(const void* q, const void* k, const void* v, int64_t ld_qkv, void* o, int64_t ld_o, const int32_t* cu, int B, int64_t T,
                                  int H, int d, int max_len, float scale, const esme_attn_opts_t* opts, void* st) {
    CALL("attn_varlen_fwd_opts q=%s k=%s v=%s ld_qkv=%lld o=%s ld_o=%lld cu=%s B=%d T=%lld H=%d d=%d max_len=%d scale=%a %s stream=%s",
         S(q), S(k), S(v), (ll)ld_qkv, S(o), (ll)ld_o, S(cu), B, (ll)T, H, d, max_len, scale, attn_opts(opts).c_str(), S(st));
}

int esme_hip_attn_varlen_fwd_qkpair_f16(const void* q, const void* k, const void* v, int64_t ld_qkv, int64_t lo_qk, void* o, int64_t ld_o, const int32_t* cu, int B,
                                        int64_t T, int H, int d, int max_len, float scale, const int32_t* order, void* st) {
    CALL("attn_varlen_fwd_qkpair_f16 q=%s k=%s v=%s ld_qkv=%lld lo_qk=%lld o=%s ld_o=%lld cu=%s B=%d T=%lld H=%d d=%d max_len=%d scale=%a seq_order=%s stream=%s",
         S(q), S(k), S(v), (ll)ld_qkv, (ll)lo_qk, S(o), (ll)ld_o, S(cu), B, (ll)T, H, d, max_len, scale, S(order), S(st));
}

int esme_hip_attn_varlen_fwd_split(const void* q, const void* k, const void* v, int64_t ld_qkv, int64_t lo_qkv, void* o, int64_t ld_o, int64_t lo_o,
                                   const int32_t* cu, int B, int64_t T, int H, int d, int max_len, float scale, const int32_t* order, void* st) {
    CALL("attn_varlen_fwd_split q=%s k=%s v=%s ld_qkv=%lld lo_qkv=%lld o=%s ld_o=%lld lo_o=%lld cu=%s B=%d T=%lld H=%d d=%d max_len=%d scale=%a seq_order=%s stream=%s",
         S(q), S(k), S(v), (ll)ld_qkv, (ll)lo_qkv, S(o), (ll)ld_o, (ll)lo_o, S(cu), B, (ll)T, H, d, max_len, scale, S(order), S(st));
}

int esme_hip_layernorm_split(const void* x, int64_t ldx, int in_pair, int64_t in_off, const void* w, const void* b, void* y, int64_t ldy, int64_t out_off,
                             float* y32, int64_t ld32, int64_t T, int E, float eps, void* st) {
    CALL("layernorm_split x=%s ldx=%lld in_pair=%d in_off=%lld w=%s b=%s y=%s ldy=%lld out_off=%lld y32=%s ld32=%lld T=%lld E=%d eps=%a stream=%s",
         S(x), (ll)ldx, in_pair, (ll)in_off, S(w), S(b), S(y), (ll)ldy, (ll)out_off, S(y32), (ll)ld32, (ll)T, E, eps, S(st));
}

int esme_hip_layernorm_split_checked(const void* x, int64_t ldx, int in_pair, int64_t in_off, const void* w, const void* b, void* y, int64_t ldy, int64_t out_off,
                                     float* y32, int64_t ld32, int64_t T, int E, float eps, int* flag, void* st) {
    CALL("layernorm_split_checked x=%s ldx=%lld in_pair=%d in_off=%lld w=%s b=%s y=%s ldy=%lld out_off=%lld y32=%s ld32=%lld T=%lld E=%d eps=%a overflow_flag=%s stream=%s",
         S(x), (ll)ldx, in_pair, (ll)in_off, S(w), S(b), S(y), (ll)ldy, (ll)out_off, S(y32), (ll)ld32, (ll)T, E, eps, S(flag), S(st));
}

int esme_hip_rotary_split(void* x, int64_t ld, int64_t lo_off, const float* cos, const float* sin, const int32_t* pos, int64_t T, int nheads, int d, int max_len, void* st) {
    CALL("rotary_split x=%s ld=%lld lo_off=%lld cos=%s sin=%s pos=%s T=%lld nheads=%d d=%d max_len=%d stream=%s", S(x), (ll)ld, (ll)lo_off, S(cos), S(sin), S(pos), (ll)T, nheads, d,
         max_len, S(st));
}

int esme_hip_gemm_bf16(const void* A, int64_t lda, const void* W, const void* bias, const void* resid, int64_t ldr, void* C, int64_t ldc, int64_t M, int N, int K,
                       int epi, float alpha, void* st) {
    CALL("gemm_bf16 A=%s lda=%lld W=%s bias=%s resid=%s ldr=%lld C=%s ldc=%lld M=%lld N=%d K=%d epi=%d alpha=%a stream=%s", S(A), (ll)lda, S(W), S(bias), S(resid), (ll)ldr, S(C),
         (ll)ldc, (ll)M, N, K, epi, alpha, S(st));
}

int esme_hip_gemm_bf16_fused(const void* A, int64_t lda, const void* W, const void* bias, const void* resid, int64_t ldr, void* C, int64_t ldc, int64_t M, int N, int K,
                             int epi, float alpha, const esme_gemm_fusion_t* f, void* st) {
    CALL("gemm_bf16_fused A=%s lda=%lld W=%s bias=%s resid=%s ldr=%lld C=%s ldc=%lld M=%lld N=%d K=%d epi=%d alpha=%a %s stream=%s", S(A), (ll)lda, S(W), S(bias), S(resid),
         (ll)ldr, S(C), (ll)ldc, (ll)M, N, K, epi, alpha, fusion(f).c_str(), S(st));
}

}  // extern "C"

namespace {

// ---- the cases
enum Mode { FAST, HALF, EXACT };
enum Tweak { NONE, BAD_STRUCT, WS_SHORT, NO_COS, NO_COS32, NO_HEAD, NO_LN };

struct Cfg {
    std::string name;
    Mode mode = FAST;
    int E = 512, Ep = 512, H = 8, dp = 64, F = 1024, L = 3, B = 3;
    bool rotary = true, qk_norm = false, swiglu = false;
    int qp = 1;
    bool logits = false;                 // fast: LM head
    int ext_n = 0;                       // half
    bool qk_pair = false, guard = true, ovf = true, rep32 = true;
    Tweak tweak = NONE;
};

Cfg esm2(Mode mode, int dp, const char* name) {          // 8 heads of dp columns
    Cfg c;
    c.name = name; c.mode = mode; c.dp = dp; c.E = c.Ep = 8 * dp; c.F = 4 * c.E;
    return c;
}
Cfg esmc(Mode mode, const char* name) {                  // q/k LayerNorm, SwiGLU
    Cfg c;
    c.name = name; c.mode = mode; c.H = 6; c.dp = 64; c.E = c.Ep = 384; c.F = 1024; c.qk_norm = c.swiglu = true;
    return c;
}
Cfg esm1b(Mode mode, const char* name) {                 // learned positions: no rotary
    Cfg c;
    c.name = name; c.mode = mode; c.H = 20; c.dp = 16; c.E = c.Ep = 320; c.F = 1280; c.rotary = false;
    return c;
}
Cfg padded(Mode mode, const char* name) {                // embed_dim 96 in 128 physical columns, head dim 24 in 32
    Cfg c;
    c.name = name; c.mode = mode; c.H = 4; c.dp = 32; c.E = 96; c.Ep = 128; c.F = 384;
    return c;
}
template <class F> Cfg with(Cfg c, const char* name, F&& f) { c.name = name; f(c); return c; }

std::vector<Cfg> cases() {
    std::vector<Cfg> v;
    for (Mode mode : {FAST, HALF}) {
        const std::string p = mode == FAST ? "fast_" : "half_";
        for (int dp : {16, 32, 64, 128}) v.push_back(esm2(mode, dp, (p + "esm2_d" + std::to_string(dp)).c_str()));
        v.push_back(with(esm2(mode, 64, ""), (p + "esm2_d64_noqp").c_str(), [](Cfg& c) { c.qp = 0; }));
        v.push_back(with(esm2(mode, 32, ""), (p + "esm2_d32_noqp").c_str(), [](Cfg& c) { c.qp = 0; }));
        v.push_back(esmc(mode, (p + "esmc").c_str()));
        v.push_back(with(esmc(mode, ""), (p + "esmc_noqp").c_str(), [](Cfg& c) { c.qp = 0; }));
        v.push_back(esm1b(mode, (p + "esm1b").c_str()));
        v.push_back(padded(mode, (p + "padded").c_str()));
        v.push_back(with(esm2(mode, 64, ""), (p + "B1").c_str(), [](Cfg& c) { c.B = 1; }));
        v.push_back(with(esm2(mode, 64, ""), (p + "B1025").c_str(), [](Cfg& c) { c.B = 1025; }));
        v.push_back(with(esm2(mode, 64, ""), (p + "L0").c_str(), [](Cfg& c) { c.L = 0; }));        // half: refused
        v.push_back(with(esm2(mode, 64, ""), (p + "bad_struct").c_str(), [](Cfg& c) { c.tweak = BAD_STRUCT; }));
        v.push_back(with(esm2(mode, 64, ""), (p + "phys_96").c_str(), [](Cfg& c) { c.E = c.Ep = 96; }));
        v.push_back(with(esm2(mode, 64, ""), (p + "ws_short").c_str(), [](Cfg& c) { c.tweak = WS_SHORT; }));
        v.push_back(with(esm2(mode, 64, ""), (p + "no_cos").c_str(), [](Cfg& c) { c.tweak = NO_COS; }));
    }
    v.push_back(with(esm2(FAST, 64, ""), "fast_logits", [](Cfg& c) { c.logits = true; }));
    v.push_back(with(esmc(FAST, ""), "fast_esmc_logits", [](Cfg& c) { c.logits = true; }));
    v.push_back(with(esm2(FAST, 64, ""), "fast_L0_logits", [](Cfg& c) { c.L = 0; c.logits = true; }));
    v.push_back(with(esm2(FAST, 64, ""), "fast_logits_no_head", [](Cfg& c) { c.logits = true; c.tweak = NO_HEAD; }));
    v.push_back(with(esm2(FAST, 64, ""), "fast_L0_B1", [](Cfg& c) { c.L = 0; c.B = 1; }));
    // half: extension tile, q / k pairs (layers on / off / on), guards absent, rep32 absent
    for (int dp : {16, 32, 64}) {
        v.push_back(with(esm2(HALF, dp, ""), ("half_esm2_d" + std::to_string(dp) + "_ext3_pairs").c_str(), [](Cfg& c) { c.ext_n = 3; c.qk_pair = true; }));
        v.push_back(with(esm2(HALF, dp, ""), ("half_esm2_d" + std::to_string(dp) + "_pairs_noqp").c_str(), [](Cfg& c) { c.qk_pair = true; c.qp = 0; }));
    }
    v.push_back(with(esm2(HALF, 64, ""), "half_ext3", [](Cfg& c) { c.ext_n = 3; }));
    v.push_back(with(esm2(HALF, 128, ""), "half_d128_ext3", [](Cfg& c) { c.ext_n = 3; }));
    v.push_back(with(esmc(HALF, ""), "half_esmc_ext3", [](Cfg& c) { c.ext_n = 3; }));
    v.push_back(with(esm1b(HALF, ""), "half_esm1b_ext3_pairs", [](Cfg& c) { c.ext_n = 3; c.qk_pair = true; c.H = 8; c.E = c.Ep = 128; c.F = 512; }));
    v.push_back(with(padded(HALF, ""), "half_padded_ext3_pairs", [](Cfg& c) { c.ext_n = 3; c.qk_pair = true; }));
    v.push_back(with(esm2(HALF, 64, ""), "half_noguard", [](Cfg& c) { c.guard = false; }));
    v.push_back(with(esm2(HALF, 64, ""), "half_noovf", [](Cfg& c) { c.ovf = false; }));
    v.push_back(with(esmc(HALF, ""), "half_esmc_noguard_noovf", [](Cfg& c) { c.guard = c.ovf = false; }));
    v.push_back(with(esmc(HALF, ""), "half_esmc_noqp_noguard", [](Cfg& c) { c.guard = false; c.qp = 0; }));
    v.push_back(with(esm2(HALF, 64, ""), "half_pairs_noguard_norep", [](Cfg& c) { c.qk_pair = true; c.ext_n = 3; c.guard = c.ovf = c.rep32 = false; }));
    v.push_back(with(esm2(HALF, 64, ""), "half_norep", [](Cfg& c) { c.rep32 = false; }));
    v.push_back(with(esm2(HALF, 64, ""), "half_pairs_B1025", [](Cfg& c) { c.qk_pair = true; c.B = 1025; }));
    v.push_back(with(esm2(HALF, 64, ""), "half_pairs_no_cos32", [](Cfg& c) { c.qk_pair = true; c.tweak = NO_COS32; }));
    v.push_back(with(esmc(HALF, ""), "half_esmc_pairs_refused", [](Cfg& c) { c.qk_pair = true; }));
    v.push_back(with(esm2(HALF, 128, ""), "half_d128_pairs_refused", [](Cfg& c) { c.qk_pair = true; }));
    v.push_back(with(esm2(HALF, 64, ""), "half_ext65", [](Cfg& c) { c.ext_n = 65; }));
    v.push_back(with(esm2(HALF, 64, ""), "half_ext65_ws_short", [](Cfg& c) { c.ext_n = 65; c.tweak = WS_SHORT; }));
    v.push_back(with(esm2(HALF, 64, ""), "half_ext64", [](Cfg& c) { c.ext_n = 64; }));
    // exact
    for (int dp : {16, 64, 128}) v.push_back(esm2(EXACT, dp, ("exact_esm2_d" + std::to_string(dp)).c_str()));
    v.push_back(esmc(EXACT, "exact_esmc"));
    v.push_back(esm1b(EXACT, "exact_esm1b"));
    v.push_back(padded(EXACT, "exact_padded_Ea_eq_Ep"));
    v.push_back(with(padded(EXACT, ""), "exact_padded_Ea_ne_Ep", [](Cfg& c) { c.H = 6; }));
    v.push_back(with(esm2(EXACT, 64, ""), "exact_norep", [](Cfg& c) { c.rep32 = false; }));
    v.push_back(with(esm2(EXACT, 64, ""), "exact_B1", [](Cfg& c) { c.B = 1; }));
    v.push_back(with(esm2(EXACT, 64, ""), "exact_B1025", [](Cfg& c) { c.B = 1025; }));
    v.push_back(with(esm2(EXACT, 64, ""), "exact_L0", [](Cfg& c) { c.L = 0; }));
    v.push_back(with(esm2(EXACT, 64, ""), "exact_bad_struct", [](Cfg& c) { c.tweak = BAD_STRUCT; }));
    v.push_back(with(esm2(EXACT, 64, ""), "exact_phys_96", [](Cfg& c) { c.E = c.Ep = 96; }));
    v.push_back(with(esm2(EXACT, 64, ""), "exact_ws_short", [](Cfg& c) { c.tweak = WS_SHORT; }));
    v.push_back(with(esm2(EXACT, 64, ""), "exact_no_cos", [](Cfg& c) { c.tweak = NO_COS; }));
    v.push_back(with(esm2(EXACT, 64, ""), "exact_layer1_no_ln", [](Cfg& c) { c.tweak = NO_LN; }));
    v.push_back(with(padded(EXACT, ""), "exact_head_pad_24", [](Cfg& c) { c.dp = 24; c.H = 4; c.Ep = 128; }));
    return v;
}

void run(const Cfg& c) {
    g_names.clear(); g_log.clear(); g_calls = 0;
    std::vector<esme_layer_weights_t> layers(c.L > 0 ? c.L : 1);
    for (int i = 0; i < (int)layers.size(); ++i) {
        esme_layer_weights_t& w = layers[i];
        memset(&w, 0, sizeof w);
        const std::string l = "L" + std::to_string(i) + ".";
        w.qkv_w = buf(l + "qkv_w"); w.qkv_c1 = (float*)buf(l + "qkv_c1"); w.qkv_c2 = (float*)buf(l + "qkv_c2");
        w.out_w = buf(l + "out_w"); w.out_b = buf(l + "out_b");
        w.up_w = buf(l + "up_w"); w.up_c1 = (float*)buf(l + "up_c1"); w.up_c2 = (float*)buf(l + "up_c2");
        w.down_w = buf(l + "down_w"); w.down_b = buf(l + "down_b");
        w.lnq_w = buf(l + "lnq_w"); w.lnk_w = buf(l + "lnk_w"); w.lnq_b = buf(l + "lnq_b"); w.lnk_b = buf(l + "lnk_b");
        w.ps_attn = (float*)buf(l + "ps_attn"); w.ps_attn_inv = (float*)buf(l + "ps_attn_inv");
        w.ps_ffn = (float*)buf(l + "ps_ffn"); w.ps_ffn_inv = (float*)buf(l + "ps_ffn_inv");
        w.ln1_w = buf(l + "ln1_w"); w.ln1_b = buf(l + "ln1_b"); w.ln2_w = buf(l + "ln2_w"); w.ln2_b = buf(l + "ln2_b");
        w.qkv_b = buf(l + "qkv_b"); w.up_b = buf(l + "up_b");
        w.half_qk_pair = c.qk_pair && i % 2 == 0;                 // on / off / on
        if (c.tweak == NO_LN && i == 1) w.ln1_w = nullptr;
    }
    esme_model_desc_t d;
    memset(&d, 0, sizeof d);
    d.struct_bytes = c.tweak == BAD_STRUCT ? (int)sizeof d - 8 : (int)sizeof d;
    d.n_layers = c.L; d.embed_dim = c.E; d.phys_dim = c.Ep; d.heads = c.H; d.head_dim = c.E / c.H; d.head_pad = c.dp; d.ffn_dim = c.F; d.vocab = 33;
    d.swiglu = c.swiglu; d.rotary = c.rotary; d.qk_norm = c.qk_norm; d.table_len = 1026;
    d.ln_eps = 1e-5f; d.alpha = c.swiglu ? 1.0f / 1.5f : 1.0f; d.softmax_scale = 1.0f / 7.0f; d.attn_q_prescale = c.qp;
    d.layers = layers.data();
    d.final_ln_w = buf("final_ln_w"); d.final_ln_b = buf("final_ln_b");
    if (c.logits && c.tweak != NO_HEAD) {
        d.head_dense_w = buf("head_dense_w"); d.head_dense_b = buf("head_dense_b"); d.head_ln_w = buf("head_ln_w"); d.head_ln_b = buf("head_ln_b");
        d.head_final_w = buf("head_final_w"); d.head_final_b = buf("head_final_b");
    }
    if (c.tweak != NO_COS) { d.cos = buf("cos"); d.sin = buf("sin"); }
    if (c.mode == HALF) {
        if (c.ext_n) { d.half_ext_n = c.ext_n; d.half_ext_sel = (int32_t*)buf("ext_sel"); }
        d.half_qk_pair = c.qk_pair;
        if (c.ovf) d.half_overflow_flag = (int*)buf("overflow_flag");
        if (c.tweak != NO_COS32) { d.cos32 = (float*)buf("cos32"); d.sin32 = (float*)buf("sin32"); }
        if (c.guard) { d.half_col_absmax = (uint32_t*)buf("col_absmax"); d.half_qk_sumsq = (uint32_t*)buf("qk_sumsq"); }
    }
    void* x = buf(c.mode == FAST ? "x" : "x32");
    void* cu = buf("cu_lens"); void* pos = buf("pos"); void* ws = buf("workspace"); void* st = buf("stream");
    void* pair = buf("pair"); void* rep32 = c.rep32 ? buf("rep32") : nullptr; void* logits = c.logits ? buf("logits") : nullptr;
    auto ws_bytes = [&](const esme_model_desc_t* m, int64_t T) {
        return c.mode == FAST ? esme_hip_forward_workspace_bytes(m, T) : c.mode == HALF ? esme_hip_forward_half_workspace_bytes(m, T)
                                                                                        : esme_hip_forward_exact_workspace_bytes(m, T);
    };
    emit("workspace_bytes null=%lld T-1=%lld T0=%lld T1=%lld T77=%lld", (ll)ws_bytes(nullptr, 77), (ll)ws_bytes(&d, -1), (ll)ws_bytes(&d, 0), (ll)ws_bytes(&d, 1),
         (ll)ws_bytes(&d, 77));
    const int64_t T = 77, need = ws_bytes(&d, T) - (c.tweak == WS_SHORT ? 1 : 0);
    const int max_len = 40;
    for (int64_t Tc : {int64_t(0), T}) {               // T = 0 returns before most checks; then the real call
        esme::error_buffer()[0] = 0;
        int rc;
        if (c.mode == FAST) rc = esme_hip_forward(&d, x, c.Ep, (int32_t*)cu, c.B, Tc, max_len, (int32_t*)pos, ws, need, logits, 40, st);
        else if (c.mode == HALF) rc = esme_hip_forward_half(&d, (float*)x, c.Ep, (int32_t*)cu, c.B, Tc, max_len, (int32_t*)pos, ws, need, pair, 2 * c.Ep, (float*)rep32, c.Ep, st);
        else rc = esme_hip_forward_exact(&d, (float*)x, c.Ep, (int32_t*)cu, c.B, Tc, max_len, (int32_t*)pos, ws, need, pair, 2 * c.Ep, (float*)rep32, c.Ep, st);
        emit("T=%lld rc=%d err=%s", (ll)Tc, rc, esme::error_buffer());
    }
}

}  // namespace

int main(int argc, char** argv) {
    const char* only = argc == 3 && !strcmp(argv[1], "--dump") ? argv[2] : nullptr;
    if (argc != 1 && !only) { fprintf(stderr, "usage: %s [--dump CASE]\n", argv[0]); return 2; }
    bool found = false;
    for (const Cfg& c : cases()) {
        if (only && c.name != only) continue;
        found = true;
        run(c);
        if (!only) printf("== %s %d\n", c.name.c_str(), g_calls);
        fputs(g_log.c_str(), stdout);
    }
    if (!found) { fprintf(stderr, "no case %s\n", only); return 2; }
    return 0;
}
