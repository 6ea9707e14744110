// Attention maps of chosen heads of one layer, written out (include/esme_hip_attn_maps.h).
//
// Per sequence (S rows) and listed head j (head h = head_list[j]):  P = softmax_j(q_i . k_j * scale) over all S keys, stored.
// Two launches per call, each a sweep of 64 x 64 score tiles on v_mfma_f32_16x16x32_bf16 (score_tiles.h: fp32 accumulators,
// softmax in fp32 log2 units):
//  - attn_map_stats_kernel  per (sequence, listed head, 64 query rows): softmax_row_stats of score_tiles.h (all key tiles twice -> the
//                           exact row maximum m and the row sum l of exp2(s - m); contact_stats_kernel runs the same pass with its
//                           trim), stored into the workspace;
//  - attn_map_write_kernel  per (sequence, block, 64 query rows x 64 keys): the tile's scores again, P = exp2(s - m) * (1 / l),
//                           stored from the accumulator layout (a lane holds rows 4 g .. 4 g + 3 of column c: 16 lanes write a
//                           64-byte run of one row in fp32).  Weighted mode: the listed heads in list order,
//                           acc = fma(w_j, P_j, acc), one block per sequence.
// Every index is relative to the sequence's own first row and every reduction has a fixed order: a sequence's maps do not depend
// on its neighbours or on the other heads of the list (bit-identical alone and packed, run to run).  No atomics.
#include "common.h"
#include "launch.h"
#include "score_tiles.h"
#include "../../include/esme_hip_attn_maps.h"

namespace esme {

static constexpr int kMapMaxZ = 65535;

struct MapArgs {
    const u16* q; const u16* k; int64_t ld;
    const int32_t* cu; int b0; int64_t T;
    float cs;                             // softmax_scale * log2(e), or 1 with a prescaled q
    const int32_t* heads; int nh;         // the listed heads
    const float* hw;                      // weighted mode: one weight per listed head
    float* ws_m; float* ws_l;             // (nh, T): statistics of listed head j, packed row t at j * T + t
    void* map; const int64_t* map_off; int64_t slot0;
    int nt;                               // tiles along max_len
};

template <int D>
__global__ __launch_bounds__(256) void attn_map_stats_kernel(const MapArgs a) {
    __shared__ __attribute__((aligned(16))) u16 tile[kCT * TileDims<D>::LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int b = a.b0 + blockIdx.z, j = blockIdx.y, h = a.heads[j];
    const int s0 = a.cu[b], S = a.cu[b + 1] - s0;
    const int I0 = blockIdx.x * kCT;
    if (I0 >= S) return;                                                    // (block-uniform; S <= 0 included)
    const unsigned int ld = (unsigned int)a.ld;
    const u16* qb = a.q + (int64_t)s0 * a.ld + h * D;
    const u16* kb = a.k + (int64_t)s0 * a.ld + h * D;
    int qi = I0 + wave * 16 + c;
    qi = qi < S ? qi : S - 1;
    const RowStats st = softmax_row_stats<D, false>(tile, qb, kb, ld, qi, S, a.cs, 0, 0, c, g);
    if (c == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = I0 + wave * 16 + 4 * g + r;
            if (row < S) {
                const int64_t idx = (int64_t)j * a.T + s0 + row;
                a.ws_m[idx] = st.m[r];
                a.ws_l[idx] = st.l[r];
            }
        }
    }
}

__device__ __forceinline__ void store_p(float* p, float v) { *p = v; }
__device__ __forceinline__ void store_p(u16* p, float v) { *p = f2bf(v); }                            // [out-round]

// Grid (nt * nt, blocks per sequence, sequences): tile (qt, kt) = (x / nt, x % nt) of block y.  WEIGHTED: one block, every listed head.
template <int D, class OutT, bool WEIGHTED>
__global__ __launch_bounds__(256) void attn_map_write_kernel(const MapArgs a) {
    constexpr int DS = TileDims<D>::DS;
    __shared__ __attribute__((aligned(16))) u16 tile[kCT * TileDims<D>::LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int b = a.b0 + blockIdx.z;
    const int s0 = a.cu[b], S = a.cu[b + 1] - s0;
    const int I0 = (int)(blockIdx.x / (unsigned int)a.nt) * kCT, K0 = (int)(blockIdx.x % (unsigned int)a.nt) * kCT;
    if (I0 >= S || K0 >= S) return;                                         // (block-uniform; S <= 0 included)
    const unsigned int ld = (unsigned int)a.ld;
    int qi = I0 + wave * 16 + c;                                            // own operand row (fragment map: row on lane bits 0..3)
    qi = qi < S ? qi : S - 1;
    int si[4];                                                              // own accumulator rows
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        si[r] = I0 + wave * 16 + 4 * g + r;
        si[r] = si[r] < S ? si[r] : S - 1;
    }
    float acc[4][4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[cb][r] = 0.f;

    const int j0 = WEIGHTED ? 0 : (int)blockIdx.y, j1 = WEIGHTED ? a.nh : j0 + 1;
    for (int j = j0; j < j1; ++j) {                                         // weighted mode: the listed heads in list order
        const int h = a.heads[j];
        const u16* qb = a.q + (int64_t)s0 * a.ld + h * D;
        const u16* kb = a.k + (int64_t)s0 * a.ld + h * D;
        const int64_t st = (int64_t)j * a.T + s0;
        if (WEIGHTED) __syncthreads();
        stage_tile<D>(tile, kb, ld, K0, S);
        __syncthreads();
        bf16x8 af[DS];
#pragma unroll
        for (int ks = 0; ks < DS; ++ks) af[ks] = global_frag<D>(qb, ld, qi, ks, g);
        float mi[4], ii[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            mi[r] = a.ws_m[st + si[r]];
            ii[r] = 1.0f / a.ws_l[st + si[r]];                                                        // [inv-l]
        }
        f32x4 s[4];
        score_tile<D>(af, tile, c, g, s);
        const float wj = WEIGHTED ? a.hw[j] : 1.0f;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = exp2f(s[cb][r] * a.cs - mi[r]) * ii[r];                               // [score-scale] [exp] [normalise]
                acc[cb][r] = WEIGHTED ? fmaf(wj, p, acc[cb][r]) : p;                                  // [head-sum]
            }
        }
    }

    const int64_t SS = (int64_t)S * S;
    OutT* mo = (OutT*)a.map + a.map_off[b] + (a.slot0 + (WEIGHTED ? 0 : (int64_t)blockIdx.y)) * SS;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        const int key = K0 + cb * 16 + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = I0 + wave * 16 + 4 * g + r;
            if (row < S && key < S) store_p(mo + ((int64_t)row * S + key), acc[cb][r]);
        }
    }
}

template <int D>
static int launch_maps(const MapArgs& a0, int B, bool bf16, hipStream_t s) {
    return for_sequence_chunks(B, kMapMaxZ, [&](int b0, int nb) {
        MapArgs a = a0;
        a.b0 = b0;
        const bool weighted = a.hw != nullptr;
        const dim3 gs((unsigned int)a.nt, (unsigned int)a.nh, (unsigned int)nb);
        const dim3 gw((unsigned int)a.nt * (unsigned int)a.nt, weighted ? 1u : (unsigned int)a.nh, (unsigned int)nb);
        hipLaunchKernelGGL(attn_map_stats_kernel<D>, gs, dim3(256), 0, s, a);
        if (weighted) {
            if (bf16) hipLaunchKernelGGL((attn_map_write_kernel<D, u16, true>), gw, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((attn_map_write_kernel<D, float, true>), gw, dim3(256), 0, s, a);
        } else {
            if (bf16) hipLaunchKernelGGL((attn_map_write_kernel<D, u16, false>), gw, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((attn_map_write_kernel<D, float, false>), gw, dim3(256), 0, s, a);
        }
        return check_launch("attn_maps");
    });
}

}  // namespace esme

using namespace esme;

extern "C" int64_t esme_hip_attn_maps_workspace_bytes(int B, int64_t T, int n_heads) {
    ESME_CHECK_ARG(B >= 0 && T >= 0 && n_heads > 0, "attn_maps_workspace_bytes: bad sizes");
    return 2 * (int64_t)n_heads * T * (int64_t)sizeof(float);
}

extern "C" int esme_hip_attn_maps(const void* q, const void* k, int64_t ld_qk, const int32_t* cu_lens, int B, int64_t T, int H, int d,
                                  int max_len, float softmax_scale, int q_prescaled, const int32_t* head_list, int n_heads,
                                  const float* head_weights, void* map, int out_bf16, const int64_t* map_off, int64_t slot0,
                                  void* workspace, int64_t ws_bytes, void* stream) {
    ESME_CHECK_ARG(B >= 0 && T >= 0 && H > 0 && d > 0 && max_len >= 0 && n_heads > 0 && slot0 >= 0, "attn_maps: bad sizes");
    if (B == 0 || T == 0) return ESME_OK;
    float cs;
    const QKEntryChecks own{head_list && map && map_off, nullptr,
                            (reinterpret_cast<uintptr_t>(map) & (out_bf16 ? 1u : 3u)) == 0 && (reinterpret_cast<uintptr_t>(head_list) & 3u) == 0 &&
                                (reinterpret_cast<uintptr_t>(head_weights) & 3u) == 0 && (reinterpret_cast<uintptr_t>(map_off) & 7u) == 0,
                            n_heads <= 65535, "attn_maps: max_len must be > 0, H <= 65535, n_heads <= 65535, T < 2^31"};
    if (const int rc = check_qk_operands("attn_maps", q, k, ld_qk, cu_lens, T, H, d, max_len, softmax_scale, q_prescaled, workspace, own, &cs))
        return rc;
    const int64_t need = esme_hip_attn_maps_workspace_bytes(B, T, n_heads);
    ESME_CHECK_ARG(ws_bytes >= need, "attn_maps: workspace too small (see esme_hip_attn_maps_workspace_bytes)");
    const int64_t nt = ((int64_t)max_len + kCT - 1) / kCT;
    if (nt * nt > 0x7fffffffLL) ESME_FAIL(ESME_ERR_UNSUPPORTED, "attn_maps: too many tiles");
    float* ws = (float*)workspace;
    const MapArgs a{(const u16*)q, (const u16*)k, ld_qk, cu_lens, 0, T, cs,
                    head_list, n_heads, head_weights, ws, ws + (int64_t)n_heads * T, map, map_off, slot0, (int)nt};
    return dispatch_head_dim<16, 32, 64, 128>(d, "attn_maps: head dim must be 16, 32, 64 or 128", [&](auto D) {
        return launch_maps<D()>(a, B, out_bf16 != 0, (hipStream_t)stream);
    });
}
