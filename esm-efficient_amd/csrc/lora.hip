// LoRA down-projection for the packed forward (reference esme/lora.py: LoRA.lora_forward, the inner F.linear(x, lora_A)).
//
// The adapters of one GEMM ride in an "extension K-tile": the operand row is [x | u] (X = 64 n extra columns) and the weight
// [W | s B | 0], so the GEMM's own MFMA chain adds the low-rank delta in fp32 and every fused epilogue stays as it is
// (DESIGN.md section 8).  This file fills the extension columns:
//     plain form      u[t, j] = bf16( sum_k x[t, k] A[j, k] )                                  (out-projection: x = attention output)
//     LayerNorm form  u[t, j] = bf16( sum_k x[t, k] A'[j, k] - mean_t c1[j] + sd_t b[j] )      (QKV projection on the RAW stream)
// with A' = bf16(gamma * A), c1[j] = sum_k A'[j, k], b[j] = sum_k beta[k] A[j, k] and sd_t = sqrt(var_t + eps): that is
// LN(x_t) . A_j DIVIDED by rstd_t, because the LayerNorm-folded GEMM multiplies its whole accumulator by rstd_t afterwards.
// A has `rank` rows (all adapters and projections of that GEMM stacked); columns rank .. X-1 of u are written as zeros.
//
// K range: E is the K of the projection the adapters belong to: the model width (320 .. 2 560) for q / k / v / out and the FFN
// up-projection, the FFN width F (512 .. 10 240) for the FFN down-projection (x = the first F columns of the (T, F + X) activation
// buffer, ldx = F + X).  Row offsets (t * ldx, row * E) are 64-bit; k0 + 8 s, the A chunk's ch * 8 and the LDS offsets are ints
// below E + 64 <= 10 304 and NB * 16 * 72 <= 18 432: nothing depends on E beyond E % 64 == 0.
//
// A skinny product (M = T, N = X, K = E) that reads x once.  One workgroup = 4 waves x 32 rows; the A chunk of a 64-wide K step
// is shared through LDS (144-byte rows: the 16 rows a fragment read touches fall on different banks), x goes global -> register
// as the MFMA's other operand.  v_mfma_f32_16x16x32_bf16 in transposed form (A rows on the matrix's row side, x rows on the lanes),
// so a lane ends with 4 consecutive u columns of ONE row: its statistics are per lane and the result leaves as 8-byte stores.
// The k order inside a 64-wide step is permuted identically for both operands (lane group g, step s <-> k = 16 g + 8 s + j): each
// lane then reads 32 contiguous bytes of its x row and the four groups of a row cover one whole 128-byte line.
#include "common.h"
#include "launch.h"

namespace esme {
namespace {

constexpr int kLoraRows = 128;     // x rows per workgroup (4 waves x 2 blocks of 16)
constexpr int kLoraBK = 64;        // K step
constexpr int kLoraLd = 72;        // LDS row of the A chunk in elements: 64 + 8 pad
constexpr int kLoraMaxX = 256;     // widest extension this build serves

template <int NB, bool LN>         // NB = X / 16
__global__ __launch_bounds__(256) void lora_down_kernel(const u16* __restrict__ x, int64_t ldx, const u16* __restrict__ A, int R,
                                                        int64_t T, int E, u16* __restrict__ u, int64_t ldu,
                                                        const float* __restrict__ part, int nblk, int ln_dim, float eps,
                                                        const float* __restrict__ c1, const float* __restrict__ bA) {
    __shared__ __attribute__((aligned(16))) u16 As[NB * 16 * kLoraLd];
    constexpr int CH = NB * 16 * 8 / 256;                 // 16-byte chunks of the A tile per thread (NB / 2)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.x * kLoraRows + wave * 32;
    const u16* xr[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        int64_t t = m0 + rb * 16 + c;
        t = t < T ? t : T - 1;                            // (rows past the end read the last row; never stored)
        xr[rb] = x + t * ldx + 16 * g;
    }
    f32x4 acc[2][NB];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[rb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < E; k0 += kLoraBK) {
        u32x4 xf[2][2], av[CH];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int s = 0; s < 2; ++s) xf[rb][s] = *reinterpret_cast<const u32x4*>(xr[rb] + k0 + 8 * s);
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int id = tid + i * 256, row = id >> 3, ch = id & 7;
            av[i] = u32x4{0u, 0u, 0u, 0u};
            if (row < R) av[i] = *reinterpret_cast<const u32x4*>(A + (int64_t)row * E + k0 + ch * 8);
        }
        __syncthreads();                                  // the previous step's fragment reads are done
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int id = tid + i * 256, row = id >> 3, ch = id & 7;
            *reinterpret_cast<u32x4*>(&As[row * kLoraLd + ch * 8]) = av[i];
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const bf16x8 af = *reinterpret_cast<const bf16x8*>(&As[(nb * 16 + c) * kLoraLd + 16 * g + 8 * s]);
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
                    acc[rb][nb] = mfma_16x16x32<false>(af, __builtin_bit_cast(bf16x8, xf[rb][s]), acc[rb][nb]);
            }
    }

    // lane (c, g) holds u[m0 + 16 rb + c][16 nb + 4 g + i], i = 0..3
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const int64_t t = m0 + rb * 16 + c;
        if (t >= T) continue;
        float mean = 0.f, sd = 0.f;
        if constexpr (LN) {
            // the row's statistics, associated as the LayerNorm-folded GEMM associates them (gemm.hip): 128-column partials pair up first
            const f32x2* pp = reinterpret_cast<const f32x2*>(part) + t;
            float s1 = 0.f, s2 = 0.f;
            int b = 0;
            if (nblk > ((E + 255) >> 8)) {
                for (; b + 2 <= nblk; b += 2) {
                    const f32x2 p0 = pp[(int64_t)b * T], p1 = pp[(int64_t)(b + 1) * T];
                    s1 += p0[0] + p1[0]; s2 += p0[1] + p1[1];
                }
            }
            for (; b < nblk; ++b) { const f32x2 p = pp[(int64_t)b * T]; s1 += p[0]; s2 += p[1]; }
            const float inv = 1.0f / (float)ln_dim;
            mean = s1 * inv;
            sd = sqrtf(fmaxf(s2 * inv - mean * mean, 0.f) + eps);
        }
        u16* ur = u + t * ldu + 4 * g;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[i] = acc[rb][nb][i];
                if constexpr (LN) {
                    const int j = nb * 16 + 4 * g + i;
                    if (j < R) v[i] = fmaf(sd, bA[j], fmaf(-mean, c1[j], v[i]));
                }
            }
            *reinterpret_cast<u32x2*>(ur + nb * 16) = u32x2{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3])};
        }
    }
}

template <bool LN>
int launch_lora_down(const u16* x, int64_t ldx, const u16* A, int R, int64_t T, int E, int X, u16* u, int64_t ldu, const float* part,
                     int nblk, int ln_dim, float eps, const float* c1, const float* bA, hipStream_t s) {
    const int64_t grid = (T + kLoraRows - 1) / kLoraRows;
    if (grid > 0x7fffffffLL) ESME_FAIL(ESME_ERR_UNSUPPORTED, "lora_down: too many rows for one launch");
#define ESME_LORA_CASE(NB) \
    case NB: hipLaunchKernelGGL((lora_down_kernel<NB, LN>), dim3((unsigned)grid), dim3(256), 0, s, x, ldx, A, R, T, E, u, ldu, part, nblk, ln_dim, eps, c1, bA); break
    switch (X / 16) {
        ESME_LORA_CASE(4);
        ESME_LORA_CASE(8);
        ESME_LORA_CASE(12);
        ESME_LORA_CASE(16);
        default: ESME_FAIL(ESME_ERR_UNSUPPORTED, "lora_down: extension width must be 64, 128, 192 or 256");
    }
#undef ESME_LORA_CASE
    return check_launch("lora_down");
}

int check_lora_args(const void* x, int64_t ldx, const void* A, int rank, int64_t T, int E, int X, void* u, int64_t ldu) {
    ESME_CHECK_ARG(T >= 0 && E > 0 && X > 0 && rank > 0, "lora_down: bad sizes");
    ESME_CHECK_ARG(x && A && u, "lora_down: null pointer");
    if (E % kLoraBK != 0) ESME_FAIL(ESME_ERR_UNSUPPORTED, "lora_down: E must be a multiple of 64");
    if (X % 64 != 0) ESME_FAIL(ESME_ERR_UNSUPPORTED, "lora_down: the extension width X must be a multiple of 64");
    if (X > kLoraMaxX) ESME_FAIL(ESME_ERR_UNSUPPORTED, "lora_down: extension widths above 256 are not built");
    ESME_CHECK_ARG(rank <= X, "lora_down: more adapter rows than extension columns");
    ESME_CHECK_ARG(ldx >= E && ldx % 8 == 0 && ldu >= X && ldu % 8 == 0, "lora_down: bad ldx / ldu (rows of at least E / X elements, multiples of 8)");
    ESME_CHECK_ARG(aligned16(x) && aligned16(A) && aligned16(u), "lora_down: x, A and u must be 16-byte aligned");
    return ESME_OK;
}

}  // namespace
}  // namespace esme

using namespace esme;

extern "C" int esme_hip_lora_down(const void* x, int64_t ldx, const void* A, int rank, int64_t T, int E, int X, void* u, int64_t ldu,
                                  void* stream) {
    const int rc = check_lora_args(x, ldx, A, rank, T, E, X, u, ldu);
    if (rc != ESME_OK || T == 0) return rc;
    return launch_lora_down<false>((const u16*)x, ldx, (const u16*)A, rank, T, E, X, (u16*)u, ldu, nullptr, 0, 0, 0.f, nullptr, nullptr,
                                   (hipStream_t)stream);
}

extern "C" int esme_hip_lora_down_ln(const void* x, int64_t ldx, const void* A, int rank, int64_t T, int E, int X, void* u, int64_t ldu,
                                     const float* ln_partial, int ln_nblk, int ln_dim, float ln_eps, const float* c1, const float* bA,
                                     void* stream) {
    const int rc = check_lora_args(x, ldx, A, rank, T, E, X, u, ldu);
    if (rc != ESME_OK) return rc;
    ESME_CHECK_ARG(ln_partial && c1 && bA, "lora_down_ln: null statistics / c1 / bA pointer");
    ESME_CHECK_ARG((reinterpret_cast<uintptr_t>(ln_partial) & 7u) == 0 && ln_nblk > 0 && ln_dim > 0 && ln_eps >= 0.f,
                   "lora_down_ln: 8-byte aligned partial sums, ln_nblk > 0, ln_dim > 0, ln_eps >= 0");
    if (T == 0) return ESME_OK;
    return launch_lora_down<true>((const u16*)x, ldx, (const u16*)A, rank, T, E, X, (u16*)u, ldu, ln_partial, ln_nblk, ln_dim, ln_eps, c1,
                                  bA, (hipStream_t)stream);
}
