// Linear-chain CRF over packed sequences (include/esme_hip_crf.h): log Z and the forward variables, the backward recursion with the
// gradients of the emissions and of the parameters, and Viterbi decoding.
//
// One wavefront owns one sequence (a 256-thread workgroup takes four); lane j owns label j.  The recursion over the rows is serial,
// the C x C work of a step is spread as C lanes x a loop over the other index, unrolled at compile time for C rounded up to
// CP = 4 / 16 / 32 / 64 (indices C .. CP - 1 are skipped by a wave-uniform test; lanes C .. 63 compute on zeros, are never read by
// another lane and never stored, and hold no NaN on finite operands).
//  - crf_fwd_kernel: column j of the transitions in lane j's registers; the previous step's alpha reaches every lane through
//    v_readlane, one predecessor at a time in ascending order: the exact maximum first, then the sum of exp(. - max).
//  - crf_bwd_kernel: ROW i of the transitions in lane i's registers, so that one broadcast of u[j] = e_next[j] + beta_next[j] serves
//    both beta[i] = log sum_j exp(A[i][j] + u[j]) and the pairwise marginals exp(alpha[i] + A[i][j] + u[j] - log Z), which reuse the
//    exponentials of the sum: p_j = exp(s_j - m) times the per-lane factor grad exp(alpha[i] + m - log Z).  Wave w of P = min(B, 1024)
//    takes the sequences w, w + P, ... in ascending order and keeps row i of d_transitions, d_start[i] and d_end[i] in registers; its
//    partial goes to the workspace and crf_param_reduce_kernel adds the P partials in ascending order.
//  - crf_viterbi_kernel: the max-plus recursion with one back-pointer byte per (row, label) in the workspace (255 on rows outside
//    chains); it leaves the final label in the sequence's last path slot.  crf_backtrace_kernel, a launch of its own so that the
//    back-pointers are visible whichever lane wrote them, walks them backwards with the label as a wave-uniform lane index.
// Rows are loaded kCrfRows at a time (tags, emissions, alpha, back-pointers), so a step waits on memory once per kCrfRows rows.
// No atomics; every element of every output is written by exactly one thread.
#include "common.h"
#include "launch.h"
#include "../../include/esme_hip_crf.h"

namespace esme {

static constexpr int kCrfRows = 8;            // rows per batch of loads
static constexpr int kCrfNone = 255;          // back-pointer of a row outside every chain

__device__ __forceinline__ float crf_lane(float v, int i) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i)); }
__device__ __forceinline__ bool crf_spoils(float e) { return !(e < INFINITY); }          // NaN or +inf

// The rows of sequence b: [s0, s1) may hold chain rows; [z0, z1) are the rows its wave writes (sequence 0 takes the rows before
// cu_lens[0], sequence B - 1 those from cu_lens[B] on, so that every row of [0, T) has one writer).
struct CrfRows { int64_t s0, s1, z0, z1; };
__device__ __forceinline__ CrfRows crf_rows(const int32_t* __restrict__ cu, int64_t b, int64_t B, int64_t T) {
    CrfRows r;
    r.s0 = cu[b];
    r.s1 = cu[b + 1];
    r.s0 = r.s0 < 0 ? 0 : (r.s0 > T ? T : r.s0);
    r.s1 = r.s1 < r.s0 ? r.s0 : (r.s1 > T ? T : r.s1);
    r.z0 = b == 0 ? 0 : r.s0;
    r.z1 = b == B - 1 ? T : r.s1;
    return r;
}

__device__ __forceinline__ bool crf_in_chain(int tag, int C) { return tag >= ESME_HIP_CRF_FREE && tag < C; }

// log sum_{i < C} exp(v[i]) for wave-uniform v[]: the exact maximum, then the sum in ascending i.  All terms -inf: -inf, no NaN.
template <int CP>
__device__ __forceinline__ float crf_lse(float (&s)[CP], int C, float& m_out) {
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < CP; ++i)
        if (i < C) m = fmaxf(m, s[i]);                                                // [max] exact
    const float ms = m == -INFINITY ? 0.f : m;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < CP; ++i)
        if (i < C) {
            s[i] = __expf(s[i] - ms);                                                 // [sub] [exp]
            sum += s[i];                                                              // [sum] ascending
        }
    m_out = ms;
    return ms + __logf(sum);                                                          // [log] [add]
}

template <int CP>
__global__ __launch_bounds__(256) void crf_fwd_kernel(const float* __restrict__ e, int64_t lde, const float* __restrict__ A,
                                                      const float* __restrict__ start, const float* __restrict__ end,
                                                      const int32_t* __restrict__ cu, const int32_t* __restrict__ tags, int64_t B, int64_t T,
                                                      int C, float* __restrict__ logz, float* __restrict__ alpha) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const bool mine = lane < C;
    float a[CP], s[CP];                                                               // a[i] = A[i][lane]
#pragma unroll
    for (int i = 0; i < CP; ++i) a[i] = (mine && i < C) ? A[i * C + lane] : 0.f;
    const float st = mine ? start[lane] : 0.f, en = mine ? end[lane] : 0.f;
    const CrfRows R = crf_rows(cu, b, B, T);
    float al = 0.f, ms;
    bool has = false, bad = false;
    for (int64_t t0 = R.z0; t0 < R.z1; t0 += kCrfRows) {
        int tg[kCrfRows];
        float ev[kCrfRows];
#pragma unroll
        for (int k = 0; k < kCrfRows; ++k) {
            const int64_t t = t0 + k;
            const bool in = t >= R.s0 && t < R.s1;
            tg[k] = in ? tags[t] : ESME_HIP_CRF_SKIP;
            ev[k] = (in && mine) ? e[t * lde + lane] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < kCrfRows; ++k) {
            const int64_t t = t0 + k;
            if (t < R.z1) {
                const int tag = __builtin_amdgcn_readfirstlane(tg[k]);
                float out = 0.f;
                if (crf_in_chain(tag, C)) {
                    float v;
                    if (!has) {
                        v = st + ev[k];                                               // [add]
                    } else {
#pragma unroll
                        for (int i = 0; i < CP; ++i)
                            if (i < C) s[i] = crf_lane(al, i) + a[i];                 // [add]
                        v = crf_lse<CP>(s, C, ms) + ev[k];                            // [add]
                    }
                    bad |= crf_spoils(ev[k]);
                    if (tag >= 0 && lane != tag) v = -INFINITY;
                    al = out = v;
                    has = true;
                }
                if (mine) alpha[t * C + lane] = out;
            }
        }
    }
    float z = 0.f;
    if (has) {
        const float f = al + en;                                                      // [add]
#pragma unroll
        for (int i = 0; i < CP; ++i)
            if (i < C) s[i] = crf_lane(f, i);
        z = crf_lse<CP>(s, C, ms);
    }
    if (__ballot(bad) != 0ull) z = __builtin_nanf("");
    if (lane == 0) logz[b] = z;
}

template <int CP, bool PARAMS>
__global__ __launch_bounds__(256) void crf_bwd_kernel(const float* __restrict__ e, int64_t lde, const float* __restrict__ A,
                                                      const float* __restrict__ end, const int32_t* __restrict__ cu,
                                                      const int32_t* __restrict__ tags, int64_t B, int64_t T, int C, int64_t P,
                                                      const float* __restrict__ alpha, const float* __restrict__ logz,
                                                      const float* __restrict__ grad, float* __restrict__ de, int64_t ldde,
                                                      float* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= P) return;
    const bool mine = lane < C;
    float r[CP], s[CP], dA[PARAMS ? CP : 1];                                          // r[j] = A[lane][j]; dA[j]: row `lane` of d_transitions
#pragma unroll
    for (int j = 0; j < CP; ++j) r[j] = (mine && j < C) ? A[lane * C + j] : 0.f;
    if constexpr (PARAMS) {
#pragma unroll
        for (int j = 0; j < CP; ++j) dA[j] = 0.f;
    }
    const float en = mine ? end[lane] : 0.f;
    float d_start = 0.f, d_end = 0.f;
    for (int64_t b = w; b < B; b += P) {                                              // [part-sum] the part's sequences in ascending order
        const CrfRows R = crf_rows(cu, b, B, T);
        const float g = grad[b], lz = logz[b];
        float u = 0.f, last = 0.f, ms;
        bool has = false;
        for (int64_t t1 = R.z1; t1 > R.z0; t1 -= kCrfRows) {
            int tg[kCrfRows];
            float ev[kCrfRows], av[kCrfRows];
#pragma unroll
            for (int k = 0; k < kCrfRows; ++k) {
                const int64_t t = t1 - 1 - k;
                const bool in = t >= R.s0 && t < R.s1;
                tg[k] = in ? tags[t] : ESME_HIP_CRF_SKIP;
                ev[k] = (in && mine) ? e[t * lde + lane] : 0.f;
                av[k] = (in && mine) ? alpha[t * C + lane] : -INFINITY;
            }
#pragma unroll
            for (int k = 0; k < kCrfRows; ++k) {
                const int64_t t = t1 - 1 - k;
                if (t >= R.z0) {
                    const int tag = __builtin_amdgcn_readfirstlane(tg[k]);
                    float out = 0.f;
                    if (crf_in_chain(tag, C)) {
                        float beta;
                        if (!has) {
                            beta = en;
                        } else {
#pragma unroll
                            for (int j = 0; j < CP; ++j)
                                if (j < C) s[j] = r[j] + crf_lane(u, j);              // [add]
                            beta = crf_lse<CP>(s, C, ms);                             // s[j] = exp(s_j - m) from here on
                            if constexpr (PARAMS) {
                                const float f = g * __expf((av[k] + ms) - lz);        // [pair] grad exp(alpha_i + m - log Z)
#pragma unroll
                                for (int j = 0; j < CP; ++j)
                                    if (j < C) dA[j] += f * s[j];                     // [row-sum] rows in descending order
                            }
                        }
                        out = g * __expf((av[k] + beta) - lz);                        // [marginal]
                        if (!has) d_end += out;
                        last = out;
                        u = ev[k] + beta;                                             // [add]
                        if (tag >= 0 && lane != tag) u = -INFINITY;
                        has = true;
                    }
                    if (mine) de[t * ldde + lane] = out;
                }
            }
        }
        if (has) d_start += last;
    }
    if constexpr (PARAMS) {
        if (mine) {
            float* p = part + w * ((int64_t)C * C + 2 * C);
#pragma unroll
            for (int j = 0; j < CP; ++j)
                if (j < C) p[lane * C + j] = dA[j];
            p[C * C + lane] = d_start;
            p[C * C + C + lane] = d_end;
        }
    }
}

// element idx of [d_transitions | d_start | d_end] = the parts' partials in ascending part order (no part: zero)
__global__ __launch_bounds__(64) void crf_param_reduce_kernel(const float* __restrict__ part, int64_t P, int C, float* __restrict__ dA,
                                                              float* __restrict__ d_start, float* __restrict__ d_end) {
    const int n = C * C + 2 * C;
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= n) return;
    float v = 0.f;
    for (int64_t p = 0; p < P; ++p) v += part[p * n + idx];                           // [parts-sum] ascending
    if (idx < C * C) dA[idx] = v;
    else if (idx < C * C + C) d_start[idx - C * C] = v;
    else d_end[idx - C * C - C] = v;
}

template <bool I64>
__device__ __forceinline__ void crf_store_path(void* path, int64_t t, int64_t v) {
    if constexpr (I64) reinterpret_cast<int64_t*>(path)[t] = v;
    else reinterpret_cast<int32_t*>(path)[t] = (int32_t)v;
}

template <int CP, bool I64>
__global__ __launch_bounds__(256) void crf_viterbi_kernel(const float* __restrict__ e, int64_t lde, const float* __restrict__ A,
                                                          const float* __restrict__ start, const float* __restrict__ end,
                                                          const int32_t* __restrict__ cu, const int32_t* __restrict__ tags, int64_t B,
                                                          int64_t T, int C, void* __restrict__ path, float* __restrict__ score,
                                                          unsigned char* __restrict__ bp) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const bool mine = lane < C;
    float a[CP];
#pragma unroll
    for (int i = 0; i < CP; ++i) a[i] = (mine && i < C) ? A[i * C + lane] : 0.f;
    const float st = mine ? start[lane] : 0.f, en = mine ? end[lane] : 0.f;
    const CrfRows R = crf_rows(cu, b, B, T);
    float v = 0.f;
    bool has = false, bad = false;
    for (int64_t t0 = R.z0; t0 < R.z1; t0 += kCrfRows) {
        int tg[kCrfRows];
        float ev[kCrfRows];
#pragma unroll
        for (int k = 0; k < kCrfRows; ++k) {
            const int64_t t = t0 + k;
            const bool in = t >= R.s0 && t < R.s1;
            tg[k] = in ? tags[t] : ESME_HIP_CRF_SKIP;
            ev[k] = (in && mine) ? e[t * lde + lane] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < kCrfRows; ++k) {
            const int64_t t = t0 + k;
            if (t < R.z1) {
                const int tag = __builtin_amdgcn_readfirstlane(tg[k]);
                int arg = kCrfNone;
                if (crf_in_chain(tag, C)) {
                    float best = -INFINITY;
                    arg = 0;
                    if (!has) {
                        best = st;
                    } else {
#pragma unroll
                        for (int i = 0; i < CP; ++i)
                            if (i < C) {
                                const float c = crf_lane(v, i) + a[i];
                                if (c > best) { best = c; arg = i; }                  // ties: the lowest predecessor
                            }
                    }
                    bad |= crf_spoils(ev[k]);
                    v = best + ev[k];
                    if (tag >= 0 && lane != tag) v = -INFINITY;
                    has = true;
                }
                if (mine) bp[t * C + lane] = (unsigned char)arg;
            }
        }
    }
    float best = 0.f;
    int y = 0;
    if (has) {
        const float f = v + en;
        best = -INFINITY;
#pragma unroll
        for (int i = 0; i < CP; ++i)
            if (i < C) {
                const float c = crf_lane(f, i);
                if (c > best) { best = c; y = i; }                                    // ties: the lowest final label
            }
    }
    if (__ballot(bad) != 0ull) best = __builtin_nanf("");
    if (lane == 0) {
        score[b] = best;
        if (R.z1 > R.z0) crf_store_path<I64>(path, R.z1 - 1, y);                      // handed to crf_backtrace_kernel
    }
}

template <bool I64>
__global__ __launch_bounds__(256) void crf_backtrace_kernel(const int32_t* __restrict__ cu, int64_t B, int64_t T, int C, void* __restrict__ path,
                                                            int64_t fill, const unsigned char* __restrict__ bp) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const bool mine = lane < C;
    const CrfRows R = crf_rows(cu, b, B, T);
    if (R.z1 <= R.z0) return;
    int y;
    if constexpr (I64) y = (int)reinterpret_cast<const int64_t*>(path)[R.z1 - 1];
    else y = reinterpret_cast<const int32_t*>(path)[R.z1 - 1];
    y = __builtin_amdgcn_readfirstlane(y);
    y = y < 0 ? 0 : (y >= C ? C - 1 : y);
    for (int64_t t1 = R.z1; t1 > R.z0; t1 -= kCrfRows) {
        int q[kCrfRows];
#pragma unroll
        for (int k = 0; k < kCrfRows; ++k) {
            const int64_t t = t1 - 1 - k;
            q[k] = (t >= R.z0 && mine) ? (int)bp[t * C + lane] : kCrfNone;
        }
#pragma unroll
        for (int k = 0; k < kCrfRows; ++k) {
            const int64_t t = t1 - 1 - k;
            if (t >= R.z0) {
                const int prev = __builtin_amdgcn_readlane(q[k], y);
                if (lane == 0) crf_store_path<I64>(path, t, prev == kCrfNone ? fill : (int64_t)y);
                if (prev != kCrfNone) y = prev < C ? prev : y;
            }
        }
    }
}

}  // namespace esme

using namespace esme;

static int crf_check_sizes(int64_t B, int64_t T, int C) {
    ESME_CHECK_ARG(B >= 0 && T >= 0, "crf: bad sizes");
    if (C < 1 || C > ESME_HIP_CRF_MAX_C) ESME_FAIL(ESME_ERR_UNSUPPORTED, "crf: need 1 <= C <= 64 (one lane of a wavefront per label)");
    if (T >= 0x80000000LL || B >= 0x80000000LL) ESME_FAIL(ESME_ERR_UNSUPPORTED, "crf: T >= 2^31 or B >= 2^31");
    return ESME_OK;
}

static inline int64_t crf_parts(int64_t B) { return B < ESME_HIP_CRF_PARTS ? B : ESME_HIP_CRF_PARTS; }
static inline int64_t crf_bwd_bytes(int64_t B, int C) { return crf_parts(B) * ((int64_t)C * C + 2 * C) * (int64_t)sizeof(float); }
static inline int64_t crf_decode_bytes(int64_t T, int C) { return (T * C + 15) / 16 * 16; }

extern "C" int64_t esme_hip_crf_bwd_workspace_bytes(int64_t B, int64_t T, int C) {
    const int rc = crf_check_sizes(B, T, C);
    if (rc != ESME_OK) return rc;
    return crf_bwd_bytes(B, C);
}

extern "C" int64_t esme_hip_crf_decode_workspace_bytes(int64_t T, int C) {
    const int rc = crf_check_sizes(0, T, C);
    if (rc != ESME_OK) return rc;
    return crf_decode_bytes(T, C);
}

static int crf_check_operands(const float* e, int64_t ld_e, const float* A, const float* start, const float* end, const int32_t* cu,
                              const int32_t* tags, int64_t T, int C) {
    ESME_CHECK_ARG(A && start && end && cu, "crf: null pointer");
    ESME_CHECK_ARG(aligned16(A) && aligned16(start) && aligned16(end) && aligned16(cu), "crf: misaligned transitions, start, end or cu_lens");
    if (T > 0) {
        ESME_CHECK_ARG(e && tags, "crf: null pointer");
        ESME_CHECK_ARG(aligned16(e) && aligned16(tags), "crf: misaligned emissions or tags");
        ESME_CHECK_ARG(ld_e >= C, "crf: bad row stride (need ld_e >= C)");
    }
    return ESME_OK;
}

// f(std::integral_constant<int, CP>{}) for the smallest CP of 4 / 16 / 32 / 64 that covers C
template <class F>
static inline int crf_dispatch_labels(int C, F&& f) {
    if (C <= 4) return f(std::integral_constant<int, 4>{});
    if (C <= 16) return f(std::integral_constant<int, 16>{});
    if (C <= 32) return f(std::integral_constant<int, 32>{});
    return f(std::integral_constant<int, 64>{});
}

extern "C" int esme_hip_crf_fwd(const float* emissions, int64_t ld_e, const float* transitions, const float* start, const float* end,
                                const int32_t* cu_lens, const int32_t* tags, int64_t B, int64_t T, int C, float* logz, float* alpha,
                                void* stream) {
    int rc = crf_check_sizes(B, T, C);
    if (rc != ESME_OK) return rc;
    if (B == 0) return ESME_OK;
    if ((rc = crf_check_operands(emissions, ld_e, transitions, start, end, cu_lens, tags, T, C)) != ESME_OK) return rc;
    ESME_CHECK_ARG(logz && aligned16(logz), "crf_fwd: logz null or misaligned");
    if (T > 0) ESME_CHECK_ARG(alpha && aligned16(alpha), "crf_fwd: alpha null or misaligned");
    const hipStream_t st = (hipStream_t)stream;
    const unsigned int blocks = (unsigned int)((B + 3) / 4);
    rc = crf_dispatch_labels(C, [&](auto cp) {
        hipLaunchKernelGGL((crf_fwd_kernel<decltype(cp)::value>), dim3(blocks), dim3(256), 0, st, emissions, ld_e, transitions, start, end,
                           cu_lens, tags, B, T, C, logz, alpha);
        return ESME_OK;
    });
    if (rc != ESME_OK) return rc;
    return check_launch("crf_fwd");
}

extern "C" int esme_hip_crf_bwd(const float* emissions, int64_t ld_e, const float* transitions, const float* start, const float* end,
                                const int32_t* cu_lens, const int32_t* tags, int64_t B, int64_t T, int C, const float* alpha,
                                const float* logz, const float* grad, float* d_emissions, int64_t ld_de, int want_params,
                                float* d_transitions, float* d_start, float* d_end, void* workspace, int64_t ws_bytes, void* stream) {
    int rc = crf_check_sizes(B, T, C);
    if (rc != ESME_OK) return rc;
    if (want_params) {
        ESME_CHECK_ARG(d_transitions && d_start && d_end, "crf_bwd: null pointer (d_transitions, d_start or d_end)");
        ESME_CHECK_ARG(aligned16(d_transitions) && aligned16(d_start) && aligned16(d_end), "crf_bwd: misaligned d_transitions, d_start or d_end");
    }
    const hipStream_t st = (hipStream_t)stream;
    const int64_t P = crf_parts(B);
    const unsigned int nred = (unsigned int)((C * C + 2 * C + 63) / 64);
    if (B == 0) {
        if (want_params) {
            hipLaunchKernelGGL(crf_param_reduce_kernel, dim3(nred), dim3(64), 0, st, (const float*)nullptr, (int64_t)0, C, d_transitions, d_start, d_end);
            return check_launch("crf_bwd");
        }
        return ESME_OK;
    }
    if ((rc = crf_check_operands(emissions, ld_e, transitions, start, end, cu_lens, tags, T, C)) != ESME_OK) return rc;
    ESME_CHECK_ARG(logz && grad, "crf_bwd: null pointer (logz or grad)");
    ESME_CHECK_ARG(aligned16(logz) && aligned16(grad), "crf_bwd: misaligned logz or grad");
    if (T > 0) {
        ESME_CHECK_ARG(alpha && d_emissions, "crf_bwd: null pointer (alpha or d_emissions)");
        ESME_CHECK_ARG(aligned16(alpha) && aligned16(d_emissions), "crf_bwd: misaligned alpha or d_emissions");
        ESME_CHECK_ARG(ld_de >= C, "crf_bwd: bad row stride (need ld_de >= C)");
    }
    if (want_params) {
        ESME_CHECK_ARG(workspace && aligned16(workspace), "crf_bwd: workspace null or misaligned");
        ESME_CHECK_ARG(ws_bytes >= crf_bwd_bytes(B, C), "crf_bwd: workspace too small (see esme_hip_crf_bwd_workspace_bytes)");
    }
    const unsigned int blocks = (unsigned int)((P + 3) / 4);
    rc = crf_dispatch_labels(C, [&](auto cp) {
        return dispatch_flags([&](auto pf) {
            hipLaunchKernelGGL((crf_bwd_kernel<decltype(cp)::value, decltype(pf)::value>), dim3(blocks), dim3(256), 0, st, emissions, ld_e,
                               transitions, end, cu_lens, tags, B, T, C, P, alpha, logz, grad, d_emissions, ld_de, (float*)workspace);
            return ESME_OK;
        }, want_params != 0);
    });
    if (rc != ESME_OK) return rc;
    if (want_params)
        hipLaunchKernelGGL(crf_param_reduce_kernel, dim3(nred), dim3(64), 0, st, (const float*)workspace, P, C, d_transitions, d_start, d_end);
    return check_launch("crf_bwd");
}

extern "C" int esme_hip_crf_decode(const float* emissions, int64_t ld_e, const float* transitions, const float* start, const float* end,
                                   const int32_t* cu_lens, const int32_t* tags, int64_t B, int64_t T, int C, void* path, int path_i64,
                                   int64_t fill, float* score, void* workspace, int64_t ws_bytes, void* stream) {
    int rc = crf_check_sizes(B, T, C);
    if (rc != ESME_OK) return rc;
    if (B == 0) return ESME_OK;
    if ((rc = crf_check_operands(emissions, ld_e, transitions, start, end, cu_lens, tags, T, C)) != ESME_OK) return rc;
    ESME_CHECK_ARG(score && aligned16(score), "crf_decode: score null or misaligned");
    if (T > 0) {
        ESME_CHECK_ARG(path && workspace, "crf_decode: null pointer (path or workspace)");
        ESME_CHECK_ARG(aligned16(path) && aligned16(workspace), "crf_decode: misaligned path or workspace");
        ESME_CHECK_ARG(ws_bytes >= crf_decode_bytes(T, C), "crf_decode: workspace too small (see esme_hip_crf_decode_workspace_bytes)");
    }
    const hipStream_t st = (hipStream_t)stream;
    const unsigned int blocks = (unsigned int)((B + 3) / 4);
    rc = crf_dispatch_labels(C, [&](auto cp) {
        return dispatch_flags([&](auto i64) {
            hipLaunchKernelGGL((crf_viterbi_kernel<decltype(cp)::value, decltype(i64)::value>), dim3(blocks), dim3(256), 0, st, emissions, ld_e,
                               transitions, start, end, cu_lens, tags, B, T, C, path, score, (unsigned char*)workspace);
            if (T > 0)
                hipLaunchKernelGGL((crf_backtrace_kernel<decltype(i64)::value>), dim3(blocks), dim3(256), 0, st, cu_lens, B, T, C, path, fill,
                                   (const unsigned char*)workspace);
            return ESME_OK;
        }, path_i64 != 0);
    });
    if (rc != ESME_OK) return rc;
    return check_launch("crf_decode");
}
