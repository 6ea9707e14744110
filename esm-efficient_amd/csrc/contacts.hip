// Residue-contact logits from the attention maps of one layer, reduced as they are produced (include/esme_hip_contacts.h).
//
// Per sequence (S rows, f / e rows trimmed at the ends, n = S - f - e) and head h:
//     P = softmax_j(q_i . k_j * scale) over all S keys,  A = P[f : S - e, f : S - e],  Y = A + A^T,  r = Y 1,  t = 1^T r,
//     map += sum_h w_h (Y - r r^T / t).
// Everything but r r^T / t is linear in P, so no S x S object is ever stored: four launches per layer, each a sweep of
// 64 x 64 score tiles on v_mfma_f32_16x16x32_bf16 (fp32 accumulators, softmax in fp32 log2 units, P never rounded):
//  - contact_stats_kernel   per (sequence, head, 64 query rows): all key tiles twice (softmax_row_stats of score_tiles.h, the pass
//                           attn_maps.hip runs without a trim) -> row maximum m, row sum l, and the row sum of A (the sum over the
//                           kept keys only, times 1 / l);
//  - contact_colsum_kernel  per (sequence, head, 64 key rows): all kept query tiles, P normalised with their m, l -> column sums
//                           of A; r = row sum + column sum;
//  - contact_total_kernel   per (sequence, head): t = sum_i r_i, lane-strided partial sums and one butterfly (a fixed order);
//  - contact_pair_kernel    per (sequence, tile pair I <= J), heads in index order: S_IJ = Q_I K_J^T and S_JI^T = K_I Q_J^T land in
//                           the same register layout, acc += w_h (A_IJ + A_JI^T) - (w_h / t_h) r_I r_J^T; the tile and its mirror
//                           image are stored (or added to the map) from the same registers: the map is exactly symmetric.
// The tile code (operand fragments, LDS staging, the score MFMAs) is score_tiles.h, shared with the attention backward; the checks
// of the (q, k) operand arguments (check_qk_operands) are there too, shared with esme_hip_attn_maps.
// Every index is relative to the sequence's own first row and every reduction has a fixed order: a sequence's map does not
// depend on its neighbours (bit-identical alone and packed, run to run).  No atomics.
//
// The regression's features at chosen residue pairs (include/esme_hip_contact_features.h) run the three statistics kernels
// unchanged and then
//  - contact_gather_kernel  per pair (s, i, j) one wave, every head: N_ij = A_ij + A_ji - r_i r_j / t from two fp32 dot products
//                           and the stored m, l, r, t; D / 8 lanes share a head (16 bytes of each of the four rows per lane).
#include "common.h"
#include "launch.h"
#include "score_tiles.h"
#include "../../include/esme_hip_contacts.h"
#include "../../include/esme_hip_contact_features.h"

namespace esme {

static constexpr int kContactMaxZ = 65535;

struct ContactArgs {
    const u16* q; const u16* k; int64_t ld;
    const int32_t* cu; int b0; int B; int64_t T; int H;
    float cs;                             // softmax_scale * log2(e), or 1 with a prescaled q
    int f, e;                             // rows trimmed at the front / back of every sequence
    float* ws_m; float* ws_l; float* ws_r; float* ws_t;
    const float* w; float bias; int init; float* map; const int64_t* map_off;
};

template <int D>
__global__ __launch_bounds__(256) void contact_stats_kernel(const ContactArgs a) {
    __shared__ __attribute__((aligned(16))) u16 tile[kCT * TileDims<D>::LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int b = a.b0 + blockIdx.z, h = blockIdx.y;
    const int s0 = a.cu[b], S = a.cu[b + 1] - s0, n = S - a.f - a.e;
    const int I0 = blockIdx.x * kCT;
    if (n <= 0 || I0 >= n) return;                                          // (block-uniform)
    const unsigned int ld = (unsigned int)a.ld;
    const u16* qb = a.q + (int64_t)s0 * a.ld + h * D;
    const u16* kb = a.k + (int64_t)s0 * a.ld + h * D;
    int qi = I0 + wave * 16 + c;
    qi = qi < n ? qi : n - 1;
    const RowStats st = softmax_row_stats<D, true>(tile, qb, kb, ld, a.f + qi, S, a.cs, a.f, a.e, c, g);
    if (c == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = I0 + wave * 16 + 4 * g + r;
            if (row < n) {
                const int64_t idx = (int64_t)h * a.T + s0 + a.f + row;
                a.ws_m[idx] = st.m[r];
                a.ws_l[idx] = st.l[r];
                a.ws_r[idx] = st.lt[r] * (1.0f / st.l[r]);                                                 // [inv-l] [normalise]
            }
        }
    }
}

template <int D>
__global__ __launch_bounds__(256) void contact_colsum_kernel(const ContactArgs a) {
    constexpr int DS = TileDims<D>::DS;
    __shared__ __attribute__((aligned(16))) u16 tile[kCT * TileDims<D>::LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int b = a.b0 + blockIdx.z, h = blockIdx.y;
    const int s0 = a.cu[b], S = a.cu[b + 1] - s0, n = S - a.f - a.e;
    const int I0 = blockIdx.x * kCT;
    if (n <= 0 || I0 >= n) return;                                          // (block-uniform)
    const unsigned int ld = (unsigned int)a.ld;
    const u16* qb = a.q + (int64_t)s0 * a.ld + h * D;
    const u16* kb = a.k + (int64_t)s0 * a.ld + h * D;
    const int64_t st = (int64_t)h * a.T + s0 + a.f;                        // statistics of this (head, sequence): kept row i at st + i
    int kj = I0 + wave * 16 + c;
    kj = kj < n ? kj : n - 1;
    bf16x8 af[DS];
#pragma unroll
    for (int ks = 0; ks < DS; ++ks) af[ks] = global_frag<D>(kb, ld, a.f + kj, ks, g);

    f32x4 s[4];
    float col[4] = {0.f, 0.f, 0.f, 0.f};
    for (int qt = 0; qt < n; qt += kCT) {
        __syncthreads();
        stage_tile<D>(tile, qb, ld, a.f + qt, S);
        __syncthreads();
        score_tile<D>(af, tile, c, g, s);                                   // s[cb][r] = k (own row 4 g + r) . q (row qt + 16 cb + c)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const int qi = qt + cb * 16 + c;
            const bool valid = qi < n;
            const int64_t qs = st + (valid ? qi : n - 1);
            const float m = a.ws_m[qs], inv = 1.0f / a.ws_l[qs];                                      // [inv-l]
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = exp2f(s[cb][r] * a.cs - m) * inv;                                     // [exp] [normalise]
                col[r] += valid ? p : 0.f;                                                            // [col-sum]
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) col[r] = row16_sum(col[r]);
    if (c == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = I0 + wave * 16 + 4 * g + r;
            if (row < n) a.ws_r[st + row] = a.ws_r[st + row] + col[r];                                // [r]
        }
    }
}

// t = sum_i r_i: lane l sums rows l, l + 64, ... in order, then one butterfly.  Grid (H, sequences), one wave.
__global__ __launch_bounds__(64) void contact_total_kernel(const ContactArgs a) {
    const int b = a.b0 + blockIdx.y, h = blockIdx.x;
    const int s0 = a.cu[b], n = a.cu[b + 1] - s0 - a.f - a.e;
    if (n <= 0) return;
    const float* r = a.ws_r + (int64_t)h * a.T + s0 + a.f;
    float v = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) v += r[i];                                              // [t]
    v = wave_sum(v);
    if (threadIdx.x == 0) a.ws_t[(int64_t)h * a.B + b] = v;
}

template <int D>
__global__ __launch_bounds__(256) void contact_pair_kernel(const ContactArgs a) {
    constexpr int DS = TileDims<D>::DS;
    __shared__ __attribute__((aligned(16))) u16 tk[kCT * TileDims<D>::LD];
    __shared__ __attribute__((aligned(16))) u16 tq[kCT * TileDims<D>::LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int b = a.b0 + blockIdx.z;
    const int s0 = a.cu[b], S = a.cu[b + 1] - s0, n = S - a.f - a.e;
    if (n <= 0) return;                                                     // (block-uniform)
    // tile pair p -> (I, J), I <= J: J is the largest integer with J (J + 1) / 2 <= p
    const long long p = blockIdx.x;
    long long J = (long long)((sqrt((double)(8 * p + 1)) - 1.0) * 0.5);
    while ((J + 1) * (J + 2) / 2 <= p) ++J;
    while (J * (J + 1) / 2 > p) --J;
    const long long I = p - J * (J + 1) / 2;
    if (J * kCT >= n) return;                                               // (block-uniform)
    const int I0 = (int)I * kCT, J0 = (int)J * kCT;
    const unsigned int ld = (unsigned int)a.ld;
    int ri = I0 + wave * 16 + c;                                            // own operand row (fragment map: row on lane bits 0..3)
    ri = ri < n ? ri : n - 1;
    int si[4];                                                              // own accumulator rows
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        si[r] = I0 + wave * 16 + 4 * g + r;
        si[r] = si[r] < n ? si[r] : n - 1;
    }
    float acc[4][4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[cb][r] = 0.f;

    for (int h = 0; h < a.H; ++h) {                                         // heads in index order
        const u16* qb = a.q + (int64_t)s0 * a.ld + h * D;
        const u16* kb = a.k + (int64_t)s0 * a.ld + h * D;
        const int64_t st = (int64_t)h * a.T + s0 + a.f;
        __syncthreads();
        stage_tile<D>(tk, kb, ld, a.f + J0, S);
        stage_tile<D>(tq, qb, ld, a.f + J0, S);
        __syncthreads();
        bf16x8 aq[DS], ak[DS];
#pragma unroll
        for (int ks = 0; ks < DS; ++ks) {
            aq[ks] = global_frag<D>(qb, ld, a.f + ri, ks, g);
            ak[ks] = global_frag<D>(kb, ld, a.f + ri, ks, g);
        }
        float mi[4], ii[4], rr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            mi[r] = a.ws_m[st + si[r]];
            ii[r] = 1.0f / a.ws_l[st + si[r]];                                                        // [inv-l]
            rr[r] = a.ws_r[st + si[r]];
        }
        const float wh = a.w[h];
        const float u = wh / a.ws_t[(int64_t)h * a.B + b];                                            // [w-over-t]
        f32x4 s1[4], s2[4];
        score_tile<D>(aq, tk, c, g, s1);                                    // s1[cb][r] = q_i . k_j,  i = own row 4 g + r, j = J0 + 16 cb + c
        score_tile<D>(ak, tq, c, g, s2);                                    // s2[cb][r] = k_i . q_j = the score of (j, i)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            int sj = J0 + cb * 16 + c;
            sj = sj < n ? sj : n - 1;
            const float mj = a.ws_m[st + sj], ij = 1.0f / a.ws_l[st + sj], rj = a.ws_r[st + sj];     // [inv-l]
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p1 = exp2f(s1[cb][r] * a.cs - mi[r]) * ii[r];                             // [exp] [normalise]  A_ij
                const float p2 = exp2f(s2[cb][r] * a.cs - mj) * ij;                                   // [exp] [normalise]  A_ji
                acc[cb][r] = fmaf(wh, p1 + p2, acc[cb][r]);                                           // [sym] [head-sum]
                acc[cb][r] = fmaf(-u, rr[r] * rj, acc[cb][r]);                                        // [apc] [head-sum]
            }
        }
    }

    float* mo = a.map + a.map_off[b];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        const int j = J0 + cb * 16 + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = I0 + wave * 16 + 4 * g + r;
            if (i < n && j < n && (I != J || i <= j)) {                     // the diagonal tile: its upper triangle, mirrored
                const int64_t up = (int64_t)i * n + j, lo = (int64_t)j * n + i;
                const float v = a.init ? a.bias + acc[cb][r] : mo[up] + acc[cb][r];                   // [layer-sum]
                mo[up] = v;
                if (i != j) mo[lo] = v;
            }
        }
    }
}

// m, l, r and t of sequences a.b0 .. a.b0 + nb - 1 into the workspace: the three statistics launches
template <int D>
static void launch_contact_stats(const ContactArgs& a, int nt, int nb, hipStream_t s) {
    const dim3 tiles((unsigned int)nt, (unsigned int)a.H, (unsigned int)nb);
    hipLaunchKernelGGL(contact_stats_kernel<D>, tiles, dim3(256), 0, s, a);
    hipLaunchKernelGGL(contact_colsum_kernel<D>, tiles, dim3(256), 0, s, a);
    hipLaunchKernelGGL(contact_total_kernel, dim3((unsigned int)a.H, (unsigned int)nb), dim3(64), 0, s, a);
}

template <int D>
static int launch_contacts(const ContactArgs& a0, int nt, int64_t npairs, hipStream_t s) {
    return for_sequence_chunks(a0.B, kContactMaxZ, [&](int b0, int nb) {
        ContactArgs a = a0;
        a.b0 = b0;
        launch_contact_stats<D>(a, nt, nb, s);
        hipLaunchKernelGGL(contact_pair_kernel<D>, dim3((unsigned int)npairs, 1u, (unsigned int)nb), dim3(256), 0, s, a);
        return check_launch("contact_layer");
    });
}

// ------------------------------------------------------------------ features at chosen pairs (esme_hip_contact_features.h)

struct GatherArgs {
    const int32_t* pairs; int64_t P;      // (P, 3) rows (s, i, j); i, j count from the first kept row
    float* feat; int64_t ld; int col0;    // pair p, head h -> feat[p * ld + col0 + h]
    int nmax;                             // max_len - f - e: kept rows past it have no statistics
};

// eight bf16 of one row against eight of another, fp32, elements in index order (bf16 products are exact in fp32)
__device__ __forceinline__ float dot8(const u32x4 x, const u32x4 y) {
    float acc = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        acc = fmaf(__uint_as_float(x[w] << 16), __uint_as_float(y[w] << 16), acc);                    // [dot]
        acc = fmaf(__uint_as_float(x[w] & 0xffff0000u), __uint_as_float(y[w] & 0xffff0000u), acc);    // [dot]
    }
    return acc;
}

// One wave per pair.  D / 8 neighbouring lanes share a head, so a pass covers 512 / D heads; the partial dot products meet in a
// butterfly over those lanes (every lane of a head ends with the same bits).  q_a . k_b is formed by the same code whichever of
// the pair's rows a and b are, p1 + p2 and r_i * r_j commute: (i, j) and (j, i) give the same bits.  Nothing depends on the
// pair's position in the list or on another pair.
template <int D>
__global__ __launch_bounds__(256) void contact_gather_kernel(const ContactArgs a, const GatherArgs ga) {
    constexpr int LPH = D / 8, HPP = 64 / LPH;
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= ga.P) return;                                                  // (wave-uniform)
    const int s = ga.pairs[3 * p], i = ga.pairs[3 * p + 1], j = ga.pairs[3 * p + 2];
    float* out = ga.feat + p * ga.ld + ga.col0;
    bool ok = s >= 0 && s < a.B && i >= 0 && j >= 0;
    int s0 = 0;
    if (ok) {                                                               // (cu_lens is read for a sequence of the batch only)
        s0 = a.cu[s];
        int n = a.cu[s + 1] - s0 - a.f - a.e;
        n = n < ga.nmax ? n : ga.nmax;
        ok = i < n && j < n;
    }
    if (!ok) {                                                              // out of range: no q, k or workspace read for it
        for (int h = lane; h < a.H; h += 64) out[h] = __builtin_nanf("");
        return;
    }
    const int sub = lane % LPH, hl = lane / LPH;
    const int64_t ri = (int64_t)s0 + a.f + i, rj = (int64_t)s0 + a.f + j;
    const u16* qi = a.q + ri * a.ld + sub * 8;
    const u16* ki = a.k + ri * a.ld + sub * 8;
    const u16* qj = a.q + rj * a.ld + sub * 8;
    const u16* kj = a.k + rj * a.ld + sub * 8;
    for (int h0 = 0; h0 < a.H; h0 += HPP) {
        const bool live = h0 + hl < a.H;
        const int h = live ? h0 + hl : a.H - 1;                             // idle lanes repeat the last head and store nothing
        const int c = h * D;
        float s1 = dot8(*reinterpret_cast<const u32x4*>(qi + c), *reinterpret_cast<const u32x4*>(kj + c));   // q_i . k_j
        float s2 = dot8(*reinterpret_cast<const u32x4*>(qj + c), *reinterpret_cast<const u32x4*>(ki + c));   // q_j . k_i
#pragma unroll
        for (int o = 1; o < LPH; o <<= 1) {
            s1 += __shfl_xor(s1, o, 64);                                                              // [dot-tree]
            s2 += __shfl_xor(s2, o, 64);
        }
        const int64_t st = (int64_t)h * a.T;
        const float ii = 1.0f / a.ws_l[st + ri], ij = 1.0f / a.ws_l[st + rj];                         // [inv-l]
        const float p1 = exp2f(s1 * a.cs - a.ws_m[st + ri]) * ii;                                     // [score-scale] [exp] [normalise]  A_ij
        const float p2 = exp2f(s2 * a.cs - a.ws_m[st + rj]) * ij;                                     // [score-scale] [exp] [normalise]  A_ji
        const float it = 1.0f / a.ws_t[(int64_t)h * a.B + s];                                         // [inv-t]
        const float rr = a.ws_r[st + ri] * a.ws_r[st + rj];                                           // [rr]
        const float v = fmaf(-rr, it, p1 + p2);                                                       // [sym] [apc]
        if (live && sub == 0) out[h] = v;
    }
}

template <int D>
static int launch_features(const ContactArgs& a0, const GatherArgs& ga, int nt, hipStream_t s) {
    if (nt > 0) {
        const int rc = for_sequence_chunks(a0.B, kContactMaxZ, [&](int b0, int nb) {
            ContactArgs a = a0;
            a.b0 = b0;
            launch_contact_stats<D>(a, nt, nb, s);
            return check_launch("contact_features");
        });
        if (rc) return rc;
    }
    hipLaunchKernelGGL(contact_gather_kernel<D>, dim3((unsigned int)((ga.P + 3) / 4)), dim3(256), 0, s, a0, ga);
    return check_launch("contact_features");
}

}  // namespace esme

using namespace esme;

extern "C" int64_t esme_hip_contact_workspace_bytes(int B, int64_t T, int H) {
    ESME_CHECK_ARG(B >= 0 && T >= 0 && H > 0, "contact_workspace_bytes: bad sizes");
    return (3 * (int64_t)H * T + (int64_t)H * B) * (int64_t)sizeof(float);
}

extern "C" int esme_hip_contact_layer(const void* q, const void* k, int64_t ld_qk, const int32_t* cu_lens, int B, int64_t T, int H,
                                      int d, int max_len, float softmax_scale, int q_prescaled, int trim_front, int trim_back,
                                      const float* w, float bias, int init, float* map, const int64_t* map_off, void* workspace,
                                      int64_t ws_bytes, void* stream) {
    ESME_CHECK_ARG(B >= 0 && T >= 0 && H > 0 && d > 0 && max_len >= 0 && trim_front >= 0 && trim_back >= 0, "contact_layer: bad sizes");
    if (B == 0 || T == 0) return ESME_OK;
    float cs;
    const QKEntryChecks own{w && map && map_off, nullptr, (reinterpret_cast<uintptr_t>(map) & 3u) == 0, true,
                            "contact_layer: max_len must be > 0, H <= 65535, T < 2^31"};
    if (const int rc = check_qk_operands("contact_layer", q, k, ld_qk, cu_lens, T, H, d, max_len, softmax_scale, q_prescaled, workspace, own, &cs))
        return rc;
    const int64_t need = esme_hip_contact_workspace_bytes(B, T, H);
    ESME_CHECK_ARG(ws_bytes >= need, "contact_layer: workspace too small (see esme_hip_contact_workspace_bytes)");
    const int64_t nmax = (int64_t)max_len - trim_front - trim_back;
    if (nmax <= 0) return ESME_OK;                                          // every sequence is trimmed away
    const int64_t nt = (nmax + kCT - 1) / kCT, npairs = nt * (nt + 1) / 2;
    if (npairs > 0x7fffffffLL) ESME_FAIL(ESME_ERR_UNSUPPORTED, "contact_layer: too many tile pairs");
    float* ws = (float*)workspace;
    const int64_t HT = (int64_t)H * T;
    ContactArgs a{(const u16*)q, (const u16*)k, ld_qk, cu_lens, 0, B, T, H, cs, trim_front, trim_back,
                  ws, ws + HT, ws + 2 * HT, ws + 3 * HT, w, bias, init, map, map_off};
    return dispatch_head_dim<16, 32, 64, 128>(d, "contact_layer: head dim must be 16, 32, 64 or 128", [&](auto D) {
        return launch_contacts<D()>(a, (int)nt, npairs, (hipStream_t)stream);
    });
}

extern "C" int64_t esme_hip_contact_features_workspace_bytes(int B, int64_t T, int H) {
    ESME_CHECK_ARG(B >= 0 && T >= 0 && H > 0, "contact_features_workspace_bytes: bad sizes");
    return (3 * (int64_t)H * T + (int64_t)H * B) * (int64_t)sizeof(float);
}

extern "C" int esme_hip_contact_features(const void* q, const void* k, int64_t ld_qk, const int32_t* cu_lens, int B, int64_t T, int H,
                                         int d, int max_len, float softmax_scale, int q_prescaled, int trim_front, int trim_back,
                                         const int32_t* pairs, int64_t P, float* feat, int64_t ld_feat, int col0, void* workspace,
                                         int64_t ws_bytes, void* stream) {
    ESME_CHECK_ARG(B >= 0 && T >= 0 && H > 0 && d > 0 && max_len >= 0 && trim_front >= 0 && trim_back >= 0 && P >= 0 && col0 >= 0,
                   "contact_features: bad sizes");
    if (B == 0 || T == 0 || P == 0) return ESME_OK;
    float cs;
    const QKEntryChecks own{pairs && feat, ld_feat >= (int64_t)col0 + H ? nullptr : "contact_features: ld_feat must be at least col0 + H",
                            (reinterpret_cast<uintptr_t>(feat) & 3u) == 0 && (reinterpret_cast<uintptr_t>(pairs) & 3u) == 0, P < 0x80000000LL,
                            "contact_features: max_len must be > 0, H <= 65535, T < 2^31, P < 2^31"};
    if (const int rc = check_qk_operands("contact_features", q, k, ld_qk, cu_lens, T, H, d, max_len, softmax_scale, q_prescaled, workspace, own, &cs))
        return rc;
    const int64_t need = esme_hip_contact_features_workspace_bytes(B, T, H);
    ESME_CHECK_ARG(ws_bytes >= need, "contact_features: workspace too small (see esme_hip_contact_features_workspace_bytes)");
    int64_t nmax = (int64_t)max_len - trim_front - trim_back;
    nmax = nmax > 0 ? nmax : 0;                                             // 0: every sequence is trimmed away, every pair out of range
    const int64_t nt = (nmax + kCT - 1) / kCT;
    float* ws = (float*)workspace;
    const int64_t HT = (int64_t)H * T;
    ContactArgs a{(const u16*)q, (const u16*)k, ld_qk, cu_lens, 0, B, T, H, cs, trim_front, trim_back,
                  ws, ws + HT, ws + 2 * HT, ws + 3 * HT, nullptr, 0.f, 0, nullptr, nullptr};
    const GatherArgs ga{pairs, P, feat, ld_feat, col0, (int)nmax};
    return dispatch_head_dim<16, 32, 64, 128>(d, "contact_features: head dim must be 16, 32, 64 or 128", [&](auto D) {
        return launch_features<D()>(a, ga, (int)nt, (hipStream_t)stream);
    });
}
