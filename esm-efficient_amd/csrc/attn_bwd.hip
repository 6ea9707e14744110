// Backward of the varlen attention over a cu_lens-packed batch (include/esme_hip_attn_bwd.h): dq, dk, dv from q, k, v, o, dO.
//
// Per sequence and head, S = Q K^T * scale, P = softmax(S), O = P V:
//     D_i = sum_c dO_ic O_ic,  dV = P^T dO,  dP = dO V^T,  dS = P o (dP - D),  dQ = scale * dS K,  dK = scale * dS^T Q.
// Three launches over 64 x 64 score tiles (score_tiles.h: bf16 MFMA 16x16x32, fp32 accumulators), no atomics:
//  - attn_bwd_stats_kernel  per (sequence, head, 64 query rows): all key tiles twice -> exact row maximum m (log2 units) and row sum l,
//                           as contact_stats_kernel forms them; D for the same rows in fp32 (four lanes per row, a fixed order);
//  - attn_bwd_dkdv_kernel   per (sequence, head, 64 key rows), every query tile: S^T = K Q^T and dP^T = V dO^T land in the register
//                           layout "own key row x streamed query"; P^T and dS^T, rounded to bf16, pass through a per-wave LDS strip to
//                           become the A operand of dV += P^T dO and dK += dS^T Q, whose B operands are the TRANSPOSED dO and Q tiles
//                           (the contraction runs over rows, which are not contiguous in memory: the tiles are staged twice, row-major
//                           for the scores and transposed for the products);
//  - attn_bwd_dq_kernel     per (sequence, head, 64 query rows), every key tile: S = Q K^T, dP = dO V^T, dS -> strip -> dQ += dS K
//                           against the transposed K tile.
// LDS at d = 64: dK/dV 4 tiles + 2 strips = 54 KB, dQ 3 tiles + 1 strip = 36 KB (pitch 72 elements either way: 16-byte fragment
// reads of 16 consecutive rows fall on distinct bank groups).
// Every index is relative to the sequence's own first row, every reduction has a fixed order, masked rows and keys contribute exact
// zeros (P = 0): a sequence's gradients do not depend on its neighbours (bit-identical alone and packed, run to run).
#include "common.h"
#include "launch.h"
#include "score_tiles.h"
#include "../../include/esme_hip_attn_bwd.h"

namespace esme {

static constexpr int kBwdMaxZ = 65535;
static constexpr int kLT = kCT + 8;       // row pitch of a transposed tile (D rows of 64 sequence positions) and of the P / dS strips

struct BwdArgs {
    const u16* q; const u16* k; const u16* v; int64_t ld;
    const u16* o; int64_t ldo; const u16* d_o; int64_t lddo;
    const int32_t* cu; int b0; int64_t T;
    float cs;                             // softmax_scale * log2(e)
    float scale;
    float* ws_m; float* ws_l; float* ws_d;
    u16* dq; u16* dk; u16* dv; int64_t ldg;
};

// stage_tile plus the transposed copy: tt[col * kLT + row]
template <int D>
__device__ __forceinline__ void stage_tile_t(u16* tile, u16* tt, const u16* base, unsigned int ld, int row0, int S) {
    constexpr int CPR = D / 8, NCH = kCT * CPR;
    for (int ch = threadIdx.x; ch < NCH; ch += 256) {
        const int row = ch / CPR, col = (ch % CPR) * 8;
        int gr = row0 + row;
        gr = gr < S ? gr : S - 1;
        const u32x4 x = *reinterpret_cast<const u32x4*>(base + ((unsigned int)gr * ld + (unsigned int)col));
        *reinterpret_cast<u32x4*>(tile + row * TileDims<D>::LD + col) = x;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            tt[(col + 2 * w) * kLT + row] = (u16)(x[w] & 0xffffu);
            tt[(col + 2 * w + 1) * kLT + row] = (u16)(x[w] >> 16);
        }
    }
}

// acc[nb][r] += sum_i strip(own row 4 g + r, i) * tt(column 16 nb + c, i): the strip is the wave's 16 x 64 A operand
template <int D>
__device__ __forceinline__ void strip_product(const u16* strip, const u16* tt, int c, int g, f32x4* acc) {
#pragma unroll
    for (int ks = 0; ks < kCT / 32; ++ks) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(strip + c * kLT + ks * 32 + g * 8);
#pragma unroll
        for (int nb = 0; nb < D / 16; ++nb)
            acc[nb] = mfma_16x16x32<false>(af, *reinterpret_cast<const bf16x8*>(tt + (nb * 16 + c) * kLT + ks * 32 + g * 8), acc[nb]);
    }
}

// rows row0 + wave * 16 + 4 g + r of one output, scaled, rounded once
template <int D>
__device__ __forceinline__ void store_rows(u16* out, int64_t ldg, const f32x4* acc, float scale, int row0, int S, int c, int g) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = row0 + 4 * g + r;
        if (row < S) {
#pragma unroll
            for (int nb = 0; nb < D / 16; ++nb) out[(int64_t)row * ldg + nb * 16 + c] = f2bf(acc[nb][r] * scale);
        }
    }
}

template <int D>
__global__ __launch_bounds__(256) void attn_bwd_stats_kernel(const BwdArgs a) {
    constexpr int DS = TileDims<D>::DS;
    __shared__ __attribute__((aligned(16))) u16 tile[kCT * TileDims<D>::LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int b = a.b0 + blockIdx.z, h = blockIdx.y;
    const int s0 = a.cu[b], S = a.cu[b + 1] - s0;
    const int I0 = blockIdx.x * kCT;
    if (I0 >= S) return;                                                    // (block-uniform; covers the empty sequence)
    const unsigned int ld = (unsigned int)a.ld;
    const u16* qb = a.q + (int64_t)s0 * a.ld + h * D;
    const u16* kb = a.k + (int64_t)s0 * a.ld + h * D;
    const int64_t st = (int64_t)h * a.T + s0;
    int qi = I0 + wave * 16 + c;
    qi = qi < S ? qi : S - 1;
    bf16x8 af[DS];
#pragma unroll
    for (int ks = 0; ks < DS; ++ks) af[ks] = global_frag<D>(qb, ld, qi, ks, g);

    f32x4 s[4];
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int kt = 0; kt < S; kt += kCT) {
        __syncthreads();
        stage_tile<D>(tile, kb, ld, kt, S);
        __syncthreads();
        score_tile<D>(af, tile, c, g, s);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            if (kt + cb * 16 + c < S) {
#pragma unroll
                for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], s[cb][r] * a.cs);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) mx[r] = row16_max(mx[r]);

    float ls[4] = {0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < S; kt += kCT) {
        __syncthreads();
        stage_tile<D>(tile, kb, ld, kt, S);
        __syncthreads();
        score_tile<D>(af, tile, c, g, s);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const bool valid = kt + cb * 16 + c < S;
#pragma unroll
            for (int r = 0; r < 4; ++r) ls[r] += valid ? exp2f(s[cb][r] * a.cs - mx[r]) : 0.f;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) ls[r] = row16_sum(ls[r]);
    if (c == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = I0 + wave * 16 + 4 * g + r;
            if (row < S) {
                a.ws_m[st + row] = mx[r];
                a.ws_l[st + row] = ls[r];
            }
        }
    }

    // D_i = sum_c dO_ic O_ic: four neighbouring lanes per row, D / 4 columns each in index order, then a two-step butterfly
    {
        const int row = I0 + (threadIdx.x >> 2), part = threadIdx.x & 3;
        const int rr = row < S ? row : S - 1;
        const u16* op = a.o + (int64_t)s0 * a.ldo + h * D + (unsigned int)rr * (unsigned int)a.ldo + part * (D / 4);
        const u16* gp = a.d_o + (int64_t)s0 * a.lddo + h * D + (unsigned int)rr * (unsigned int)a.lddo + part * (D / 4);
        float acc = 0.f;
#pragma unroll
        for (int ch = 0; ch < D / 32; ++ch) {
            float x[8], y[8];
            unpack8(*reinterpret_cast<const u32x4*>(op + ch * 8), x);
            unpack8(*reinterpret_cast<const u32x4*>(gp + ch * 8), y);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf(x[e], y[e], acc);
        }
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        if (part == 0 && row < S) a.ws_d[st + row] = acc;
    }
}

template <int D>
__global__ __launch_bounds__(256) void attn_bwd_dkdv_kernel(const BwdArgs a) {
    constexpr int DS = TileDims<D>::DS, LD = TileDims<D>::LD, NB = D / 16;
    __shared__ __attribute__((aligned(16))) u16 tq[kCT * LD];
    __shared__ __attribute__((aligned(16))) u16 tdo[kCT * LD];
    __shared__ __attribute__((aligned(16))) u16 tqT[D * kLT];
    __shared__ __attribute__((aligned(16))) u16 tdoT[D * kLT];
    __shared__ __attribute__((aligned(16))) u16 pst[4 * 16 * kLT];
    __shared__ __attribute__((aligned(16))) u16 dst[4 * 16 * kLT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int b = a.b0 + blockIdx.z, h = blockIdx.y;
    const int s0 = a.cu[b], S = a.cu[b + 1] - s0;
    const int J0 = blockIdx.x * kCT;
    if (J0 >= S) return;                                                    // (block-uniform; covers the empty sequence)
    const unsigned int ld = (unsigned int)a.ld, lddo = (unsigned int)a.lddo;
    const u16* qb = a.q + (int64_t)s0 * a.ld + h * D;
    const u16* kb = a.k + (int64_t)s0 * a.ld + h * D;
    const u16* vb = a.v + (int64_t)s0 * a.ld + h * D;
    const u16* gb = a.d_o + (int64_t)s0 * a.lddo + h * D;
    const int64_t st = (int64_t)h * a.T + s0;
    int kj = J0 + wave * 16 + c;
    kj = kj < S ? kj : S - 1;
    bf16x8 kf[DS], vf[DS];
#pragma unroll
    for (int ks = 0; ks < DS; ++ks) {
        kf[ks] = global_frag<D>(kb, ld, kj, ks, g);
        vf[ks] = global_frag<D>(vb, ld, kj, ks, g);
    }
    u16* pw = pst + wave * 16 * kLT;
    u16* dw = dst + wave * 16 * kLT;
    f32x4 dk[NB], dv[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) dk[nb] = dv[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

    f32x4 s[4], dp[4];
    for (int qt = 0; qt < S; qt += kCT) {
        __syncthreads();
        stage_tile_t<D>(tq, tqT, qb, ld, qt, S);
        stage_tile_t<D>(tdo, tdoT, gb, lddo, qt, S);
        __syncthreads();
        score_tile<D>(kf, tq, c, g, s);                                     // s[cb][r]  = k (own row 4 g + r) . q (row qt + 16 cb + c)
        score_tile<D>(vf, tdo, c, g, dp);                                   // dp[cb][r] = v (own row 4 g + r) . dO (row qt + 16 cb + c)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const int qi = qt + cb * 16 + c;
            const bool valid = qi < S;
            const int64_t qs = st + (valid ? qi : S - 1);
            const float m = a.ws_m[qs], inv = 1.0f / a.ws_l[qs], dd = a.ws_d[qs];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = valid ? exp2f(s[cb][r] * a.cs - m) * inv : 0.f;
                const float ds = p * (dp[cb][r] - dd);
                pw[(4 * g + r) * kLT + cb * 16 + c] = f2bf(p);
                dw[(4 * g + r) * kLT + cb * 16 + c] = f2bf(ds);
            }
        }
        __syncthreads();
        strip_product<D>(pw, tdoT, c, g, dv);                               // dV += P^T dO
        strip_product<D>(dw, tqT, c, g, dk);                                // dK += dS^T Q
    }
    const int64_t ob = (int64_t)s0 * a.ldg + h * D;
    store_rows<D>(a.dv + ob, a.ldg, dv, 1.0f, J0 + wave * 16, S, c, g);
    store_rows<D>(a.dk + ob, a.ldg, dk, a.scale, J0 + wave * 16, S, c, g);
}

template <int D>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const BwdArgs a) {
    constexpr int DS = TileDims<D>::DS, LD = TileDims<D>::LD, NB = D / 16;
    __shared__ __attribute__((aligned(16))) u16 tk[kCT * LD];
    __shared__ __attribute__((aligned(16))) u16 tv[kCT * LD];
    __shared__ __attribute__((aligned(16))) u16 tkT[D * kLT];
    __shared__ __attribute__((aligned(16))) u16 dst[4 * 16 * kLT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int b = a.b0 + blockIdx.z, h = blockIdx.y;
    const int s0 = a.cu[b], S = a.cu[b + 1] - s0;
    const int I0 = blockIdx.x * kCT;
    if (I0 >= S) return;                                                    // (block-uniform; covers the empty sequence)
    const unsigned int ld = (unsigned int)a.ld, lddo = (unsigned int)a.lddo;
    const u16* qb = a.q + (int64_t)s0 * a.ld + h * D;
    const u16* kb = a.k + (int64_t)s0 * a.ld + h * D;
    const u16* vb = a.v + (int64_t)s0 * a.ld + h * D;
    const u16* gb = a.d_o + (int64_t)s0 * a.lddo + h * D;
    const int64_t st = (int64_t)h * a.T + s0;
    int qi = I0 + wave * 16 + c;
    qi = qi < S ? qi : S - 1;
    bf16x8 qf[DS], gf[DS];
#pragma unroll
    for (int ks = 0; ks < DS; ++ks) {
        qf[ks] = global_frag<D>(qb, ld, qi, ks, g);
        gf[ks] = global_frag<D>(gb, lddo, qi, ks, g);
    }
    float m[4], inv[4], dd[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int row = I0 + wave * 16 + 4 * g + r;
        row = row < S ? row : S - 1;
        m[r] = a.ws_m[st + row];
        inv[r] = 1.0f / a.ws_l[st + row];
        dd[r] = a.ws_d[st + row];
    }
    u16* dw = dst + wave * 16 * kLT;
    f32x4 dq[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) dq[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

    f32x4 s[4], dp[4];
    for (int kt = 0; kt < S; kt += kCT) {
        __syncthreads();
        stage_tile_t<D>(tk, tkT, kb, ld, kt, S);
        stage_tile<D>(tv, vb, ld, kt, S);
        __syncthreads();
        score_tile<D>(qf, tk, c, g, s);                                     // s[cb][r]  = q (own row 4 g + r) . k (row kt + 16 cb + c)
        score_tile<D>(gf, tv, c, g, dp);                                    // dp[cb][r] = dO (own row 4 g + r) . v (row kt + 16 cb + c)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const bool valid = kt + cb * 16 + c < S;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = valid ? exp2f(s[cb][r] * a.cs - m[r]) * inv[r] : 0.f;
                dw[(4 * g + r) * kLT + cb * 16 + c] = f2bf(p * (dp[cb][r] - dd[r]));
            }
        }
        __syncthreads();
        strip_product<D>(dw, tkT, c, g, dq);                                // dQ += dS K
    }
    store_rows<D>(a.dq + (int64_t)s0 * a.ldg + h * D, a.ldg, dq, a.scale, I0 + wave * 16, S, c, g);
}

template <int D>
static int launch_attn_bwd(const BwdArgs& a0, int B, int H, int nt, hipStream_t s) {
    return for_sequence_chunks(B, kBwdMaxZ, [&](int b0, int nb) {
        BwdArgs a = a0;
        a.b0 = b0;
        const dim3 tiles((unsigned int)nt, (unsigned int)H, (unsigned int)nb);
        hipLaunchKernelGGL(attn_bwd_stats_kernel<D>, tiles, dim3(256), 0, s, a);
        hipLaunchKernelGGL(attn_bwd_dkdv_kernel<D>, tiles, dim3(256), 0, s, a);
        hipLaunchKernelGGL(attn_bwd_dq_kernel<D>, tiles, dim3(256), 0, s, a);
        return check_launch("attn_varlen_bwd");
    });
}

}  // namespace esme

using namespace esme;

extern "C" int64_t esme_hip_attn_varlen_bwd_workspace_bytes(int B, int64_t T, int H) {
    ESME_CHECK_ARG(B >= 0 && T >= 0 && H > 0, "attn_varlen_bwd_workspace_bytes: bad sizes");
    return 3 * (int64_t)H * T * (int64_t)sizeof(float);
}

extern "C" int esme_hip_attn_varlen_bwd(const void* q, const void* k, const void* v, int64_t ld_qkv, const void* o, int64_t ld_o,
                                        const void* d_o, int64_t ld_do, const int32_t* cu_lens, int B, int64_t T, int H, int d,
                                        int max_len, float softmax_scale, void* dq, void* dk, void* dv, int64_t ld_dqkv,
                                        void* workspace, int64_t ws_bytes, void* stream) {
    ESME_CHECK_ARG(B >= 0 && T >= 0 && H > 0 && d > 0 && max_len >= 0, "attn_varlen_bwd: bad sizes");
    if (B == 0 || T == 0) return ESME_OK;
    ESME_CHECK_ARG(q && k && v && o && d_o && cu_lens && dq && dk && dv && workspace, "attn_varlen_bwd: null pointer");
    const int64_t E = (int64_t)H * d;
    ESME_CHECK_ARG(ld_qkv % 8 == 0 && ld_qkv >= E && ld_o % 8 == 0 && ld_o >= E && ld_do % 8 == 0 && ld_do >= E && ld_dqkv % 8 == 0 && ld_dqkv >= E,
                   "attn_varlen_bwd: bad row stride");
    ESME_CHECK_ARG(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(o) && aligned16(d_o) && aligned16(dq) && aligned16(dk) && aligned16(dv) &&
                   aligned16(workspace), "attn_varlen_bwd: misaligned");
    ESME_CHECK_ARG(max_len > 0 && H <= 65535 && T < 0x80000000LL, "attn_varlen_bwd: max_len must be > 0, H <= 65535, T < 2^31");
    if (d != 32 && d != 64) ESME_FAIL(ESME_ERR_UNSUPPORTED, "attn_varlen_bwd: head dim must be 32 or 64");
    const int64_t ldmax = ld_qkv > ld_o ? (ld_qkv > ld_do ? ld_qkv : ld_do) : (ld_o > ld_do ? ld_o : ld_do);
    if ((int64_t)max_len * ldmax >= ESME_HIP_ATTN_BWD_MAX_SEQ_ELEMS)
        ESME_FAIL(ESME_ERR_UNSUPPORTED, "attn_varlen_bwd: max_len * row stride passes 2^32 elements (ESME_HIP_ATTN_BWD_MAX_SEQ_ELEMS)");
    const int64_t need = esme_hip_attn_varlen_bwd_workspace_bytes(B, T, H);
    ESME_CHECK_ARG(ws_bytes >= need, "attn_varlen_bwd: workspace too small (see esme_hip_attn_varlen_bwd_workspace_bytes)");
    const int64_t nt = ((int64_t)max_len + kCT - 1) / kCT;
    float* ws = (float*)workspace;
    const int64_t HT = (int64_t)H * T;
    const BwdArgs a{(const u16*)q, (const u16*)k, (const u16*)v, ld_qkv, (const u16*)o, ld_o, (const u16*)d_o, ld_do, cu_lens, 0, T,
                    softmax_scale * 1.4426950408889634f, softmax_scale, ws, ws + HT, ws + 2 * HT, (u16*)dq, (u16*)dk, (u16*)dv, ld_dqkv};
    const hipStream_t s = (hipStream_t)stream;
    return d == 32 ? launch_attn_bwd<32>(a, B, H, (int)nt, s) : launch_attn_bwd<64>(a, B, H, (int)nt, s);
}
