// Fused linear + cross-entropy over packed rows (include/esme_hip_linear_xent.h): loss, lse and the gradients dX, dW, db without
// materialising the (T, C) logits.
//
// A workgroup of 4 waves owns a tile of kLxTile = 64 rows; a wave owns 16 of them (score_tiles.h's pattern).  The logits of the tile
// against the up to 64 classes are one 64-wide MFMA column tile: the wave's x fragments come straight from global memory (16 bytes
// per lane), W is staged in LDS in K-chunks of kLxKC columns (rows C .. 63 and columns past E as zeros), v_mfma_f32_16x16x32_bf16,
// fp32 accumulators.  In an accumulator lane (c = lane & 15, g = lane >> 4) holds rows 4 g + 0..3 of class 16 cb + c.
// The padded classes C .. 63 are masked to -inf before the maximum, so they never enter the softmax.
//  - lx_fwd_kernel: logits, lse_t, l_t; the tile's partial of L and D (64 rows added in row order by one thread).
//  - lx_sum_kernel: the tiles' partials in a fixed order (lane i takes tiles i, i + 64, ..., then the 64 lane sums in lane order).
//  - lx_wt_kernel: W transposed and padded to (E, 64), the B operand layout of dX = G W.
//  - lx_bwd_kernel: logits again, G in fp32, rounded to bf16 into LDS (row-major, the operand of dX) and transposed into the workspace
//    (G^T (C, Tp), the operand of dW); the tile's db partial (64 rows in row order); dX through the MFMA with W^T staged in E-chunks.
//  - lx_wgrad_kernel: a workgroup owns (chunk of kLxChunk rows, slab of 128 columns): G^T fragments from global memory, x transposed
//    through LDS, accumulators over the chunk's rows in fp32, the (C, 128) partial to the workspace.
//  - lx_wgrad_reduce_kernel / lx_bgrad_reduce_kernel: partials in ascending chunk / tile order, one rounding.
// No atomics; every element of every output is written by exactly one thread.
#include "common.h"
#include "launch.h"
#include "../../include/esme_hip_linear_xent.h"

namespace esme {

static constexpr int kLxTile = ESME_HIP_LINEAR_XENT_TILE;
static constexpr int kLxChunk = ESME_HIP_LINEAR_XENT_CHUNK;
static constexpr int kLxKC = 128;             // columns of W per staged K-chunk; columns of dX / dW per staged E-chunk / slab
static constexpr int kLxLD = kLxKC + 8;       // LDS row pitch of the W chunk (elements)
static constexpr int kLxGP = 64 + 8;          // LDS row pitch of G, W^T and x^T tiles (elements): 16-byte fragment reads off the same bank
static constexpr int kLxStage = (64 * kLxLD > kLxKC * kLxGP ? 64 * kLxLD : kLxKC * kLxGP);   // elements of the shared staging buffer

__device__ __forceinline__ bf16x8 lx_zero_frag() { return __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u}); }

__device__ __forceinline__ int64_t lx_label(const void* y, int y64, int64_t row) {
    return y64 ? reinterpret_cast<const int64_t*>(y)[row] : (int64_t)reinterpret_cast<const int32_t*>(y)[row];
}

// s[cb][r] = x[row0 + 16 wave + 4 g + r] . W[16 cb + c]  (no bias), for cb < nb = ceil(C / 16); rows past T repeat row T - 1.
__device__ __forceinline__ void lx_logits(const u16* __restrict__ x, int64_t ldx, const u16* __restrict__ w, int64_t ldw, int64_t T, int E, int C,
                                          int64_t row0, u16* stage, f32x4* s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int nb = (C + 15) >> 4;
    int64_t arow = row0 + wave * 16 + c;
    arow = arow < T ? arow : T - 1;
    const u16* xa = x + arow * ldx;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) s[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < E; k0 += kLxKC) {
        bf16x8 a[kLxKC / 32];
#pragma unroll
        for (int ks = 0; ks < kLxKC / 32; ++ks) {
            const int kk = k0 + ks * 32 + g * 8;
            a[ks] = kk < E ? *reinterpret_cast<const bf16x8*>(xa + kk) : lx_zero_frag();
        }
        __syncthreads();
        for (int ch = threadIdx.x; ch < nb * 16 * (kLxKC / 8); ch += 256) {
            const int row = ch / (kLxKC / 8), col = (ch % (kLxKC / 8)) * 8;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (row < C && k0 + col < E) v = *reinterpret_cast<const u32x4*>(w + (int64_t)row * ldw + k0 + col);
            *reinterpret_cast<u32x4*>(stage + row * kLxLD + col) = v;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < kLxKC / 32; ++ks) {
            if (k0 + ks * 32 < E) {
#pragma unroll
                for (int cb = 0; cb < 4; ++cb)
                    if (cb < nb)
                        s[cb] = mfma_16x16x32<false>(a[ks], *reinterpret_cast<const bf16x8*>(stage + (cb * 16 + c) * kLxLD + ks * 32 + g * 8), s[cb]);
            }
        }
    }
}

// over the 16 lanes that hold one accumulator row (lane bits 0..3), a fixed butterfly
__device__ __forceinline__ float lx_row16_max(float v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float lx_row16_sum(float v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void lx_fwd_kernel(const u16* __restrict__ x, int64_t ldx, const u16* __restrict__ w, int64_t ldw,
                                                     const u16* __restrict__ bias, const void* __restrict__ y, int y64, int64_t ignore,
                                                     const float* __restrict__ cw, int64_t T, int E, int C, float* __restrict__ loss_rows,
                                                     float* __restrict__ lse_out, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) u16 stage[kLxStage];
    __shared__ float pl[kLxTile], pd[kLxTile];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * kLxTile;
    f32x4 s[4];
    lx_logits(x, ldx, w, ldw, T, E, C, row0, stage, s);
    float bv[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) bv[cb] = (bias && cb * 16 + c < C) ? bf2f(bias[cb * 16 + c]) : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t row = row0 + wave * 16 + g * 4 + r;
        const bool live = row < T;
        const int64_t yv = live ? lx_label(y, y64, row) : -1;
        const bool kept = live && yv != ignore && yv >= 0 && yv < C;
        float z[4], m = -INFINITY;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            z[cb] = cb * 16 + c < C ? s[cb][r] + bv[cb] : -INFINITY;                 // [bias]; padded classes never enter the softmax
            m = fmaxf(m, z[cb]);
        }
        m = lx_row16_max(m);
        float e = 0.f, zy = 0.f;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            e += cb * 16 + c < C ? __expf(z[cb] - m) : 0.f;                            // [exp]
            zy += (kept && cb * 16 + c == yv) ? z[cb] : 0.f;
        }
        e = lx_row16_sum(e);                                                          // [row-sum]
        zy = lx_row16_sum(zy);                                                        // (one non-zero term)
        const float lse = m + __logf(e);                                              // [log]
        const float cwv = kept ? (cw ? cw[yv] : 1.f) : 0.f;
        const float l = kept ? cwv * (lse - zy) : 0.f;
        if (c == 0) {
            if (live) { loss_rows[row] = l; lse_out[row] = lse; }
            pl[wave * 16 + g * 4 + r] = l;
            pd[wave * 16 + g * 4 + r] = cwv;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float L = 0.f, D = 0.f;
        for (int i = 0; i < kLxTile; ++i) { L += pl[i]; D += pd[i]; }                 // [tile-sum] rows in ascending order
        part[2 * (int64_t)blockIdx.x] = L;
        part[2 * (int64_t)blockIdx.x + 1] = D;
    }
}

// sums[0] = L, sums[1] = D, sums[2] = the loss.  One wave: lane i adds tiles i, i + 64, ... in ascending order, lane 0 the 64 lane sums.
__global__ __launch_bounds__(64) void lx_sum_kernel(const float* __restrict__ part, int64_t n, int mean, float* __restrict__ sums) {
    __shared__ float sl[64], sd[64];
    float L = 0.f, D = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 64) { L += part[2 * i]; D += part[2 * i + 1]; }
    sl[threadIdx.x] = L;
    sd[threadIdx.x] = D;
    __syncthreads();
    if (threadIdx.x == 0) {
        L = 0.f, D = 0.f;
        for (int i = 0; i < 64; ++i) { L += sl[i]; D += sd[i]; }
        sums[0] = L;
        sums[1] = D;
        sums[2] = mean ? (D == 0.f ? 0.f : L / D) : L;
        sums[3] = 0.f;
    }
}

// wt (E, 64) bf16: wt[e][c] = W[c][e] for c < C, 0 for the padded classes
__global__ __launch_bounds__(256) void lx_wt_kernel(const u16* __restrict__ w, int64_t ldw, int E, int C, u16* __restrict__ wt) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= E * 64) return;
    const int e = idx >> 6, c = idx & 63;
    wt[idx] = c < C ? w[(int64_t)c * ldw + e] : (u16)0;
}

template <bool DX, bool DW>
__global__ __launch_bounds__(256) void lx_bwd_kernel(const u16* __restrict__ x, int64_t ldx, const u16* __restrict__ w, int64_t ldw,
                                                     const u16* __restrict__ bias, const void* __restrict__ y, int y64, int64_t ignore,
                                                     const float* __restrict__ cw, int64_t T, int E, int C, int mean,
                                                     const float* __restrict__ lse_in, const float* __restrict__ sums,
                                                     const float* __restrict__ grad, const u16* __restrict__ wt, u16* __restrict__ dx,
                                                     int64_t lddx, u16* __restrict__ gt, int64_t Tp, float* __restrict__ dbp) {
    __shared__ __attribute__((aligned(16))) u16 stage[kLxStage];
    __shared__ __attribute__((aligned(16))) u16 gs[kLxTile * kLxGP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * kLxTile;
    f32x4 s[4];
    lx_logits(x, ldx, w, ldw, T, E, C, row0, stage, s);
    float bv[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) bv[cb] = (bias && cb * 16 + c < C) ? bf2f(bias[cb * 16 + c]) : 0.f;
    const float Dv = sums[1];
    const float gsc = grad[0] * (mean ? (Dv == 0.f ? 0.f : 1.0f / Dv) : 1.0f);       // [coef] g s
    u16 gb[4][4];                                                                     // [cb][r]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t row = row0 + wave * 16 + g * 4 + r;
        const bool live = row < T;
        const int64_t yv = live ? lx_label(y, y64, row) : -1;
        const bool kept = live && yv != ignore && yv >= 0 && yv < C;
        const float lse = live ? lse_in[row] : 0.f;
        const float coef = kept ? gsc * (cw ? cw[yv] : 1.f) : 0.f;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const int cls = cb * 16 + c;
            float G = 0.f;
            if (kept && cls < C) G = coef * (__expf((s[cb][r] + bv[cb]) - lse) - (cls == yv ? 1.f : 0.f));   // [G]
            gb[cb][r] = f2bf(G);                                                      // [bf16] G as an MFMA operand
            gs[(wave * 16 + g * 4 + r) * kLxGP + cls] = gb[cb][r];
        }
    }
    if constexpr (DW) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const int cls = cb * 16 + c;
            if (cls < C) {
                u32x2 v;
                v[0] = (unsigned int)gb[cb][0] | ((unsigned int)gb[cb][1] << 16);
                v[1] = (unsigned int)gb[cb][2] | ((unsigned int)gb[cb][3] << 16);
                *reinterpret_cast<u32x2*>(gt + (int64_t)cls * Tp + row0 + wave * 16 + g * 4) = v;
            }
        }
    }
    __syncthreads();
    if constexpr (DW) {
        if (threadIdx.x < 64) {
            float a = 0.f;
            for (int r = 0; r < kLxTile; ++r) a += bf2f(gs[r * kLxGP + threadIdx.x]);  // [tile-sum] rows in ascending order
            dbp[(int64_t)blockIdx.x * 64 + threadIdx.x] = a;
        }
    }
    if constexpr (DX) {
        const int nks = C > 32 ? 2 : 1;
        bf16x8 gf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) gf[ks] = *reinterpret_cast<const bf16x8*>(gs + (wave * 16 + c) * kLxGP + ks * 32 + g * 8);
        const int64_t orow = row0 + wave * 16 + c;
        for (int e0 = 0; e0 < E; e0 += kLxKC) {
            __syncthreads();
            for (int ch = threadIdx.x; ch < kLxKC * 8; ch += 256) {
                const int row = ch >> 3, col = (ch & 7) * 8;
                u32x4 v = {0u, 0u, 0u, 0u};
                if (e0 + row < E) v = *reinterpret_cast<const u32x4*>(wt + (int64_t)(e0 + row) * 64 + col);
                *reinterpret_cast<u32x4*>(stage + row * kLxGP + col) = v;
            }
            __syncthreads();
#pragma unroll
            for (int eb = 0; eb < kLxKC / 16; ++eb) {
                const int e = e0 + eb * 16 + g * 4;
                if (e0 + eb * 16 < E) {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks)
                        if (ks < nks)
                            acc = mfma_16x16x32<false>(*reinterpret_cast<const bf16x8*>(stage + (eb * 16 + c) * kLxGP + ks * 32 + g * 8), gf[ks], acc);
                    if (orow < T && e < E) {                                          // acc[r] = dX[orow][e + r]
                        u32x2 v;
                        v[0] = pack_bf16(acc[0], acc[1]);                             // [round]
                        v[1] = pack_bf16(acc[2], acc[3]);
                        *reinterpret_cast<u32x2*>(dx + orow * lddx + e) = v;
                    }
                }
            }
        }
    }
}

// part[chunk][cls][e] = sum over the chunk's rows of G[t][cls] x[t][e], e in the workgroup's slab of kLxKC columns; wave w owns 32 of them
__global__ __launch_bounds__(256) void lx_wgrad_kernel(const u16* __restrict__ x, int64_t ldx, const u16* __restrict__ gt, int64_t Tp, int64_t T,
                                                       int E, int C, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) u16 xt[kLxKC * kLxGP];                    // x^T of one 64-row tile: [column][row]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int nb = (C + 15) >> 4;
    const int slab = blockIdx.x * kLxKC;
    const int64_t chunk = blockIdx.y;
    const int64_t t_begin = chunk * kLxChunk, t_end = t_begin + kLxChunk < T ? t_begin + kLxChunk : T;
    f32x4 acc[4][2];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[mb][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t t0 = t_begin; t0 < t_end; t0 += kLxTile) {                           // [acc] rows in ascending order, 32 per MFMA
        bf16x8 a[4][2];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                a[mb][ks] = (mb < nb && mb * 16 + c < C) ? *reinterpret_cast<const bf16x8*>(gt + (int64_t)(mb * 16 + c) * Tp + t0 + ks * 32 + g * 8)
                                                          : lx_zero_frag();
        __syncthreads();
        for (int it = threadIdx.x; it < 32 * (kLxKC / 8); it += 256) {                // (row pair, 8 columns): two 16-byte loads, eight 4-byte LDS stores
            const int pair = it & 31, col = (it >> 5) * 8;
            const int64_t r = t0 + 2 * pair;
            u32x4 v0 = {0u, 0u, 0u, 0u}, v1 = {0u, 0u, 0u, 0u};
            if (slab + col < E) {
                if (r < T) v0 = *reinterpret_cast<const u32x4*>(x + r * ldx + slab + col);
                if (r + 1 < T) v1 = *reinterpret_cast<const u32x4*>(x + (r + 1) * ldx + slab + col);
            }
            unsigned int* dst = reinterpret_cast<unsigned int*>(xt) + pair;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dst[(col + 2 * i) * (kLxGP / 2)] = (v0[i] & 0xffffu) | (v1[i] << 16);
                dst[(col + 2 * i + 1) * (kLxGP / 2)] = (v0[i] >> 16) | (v1[i] & 0xffff0000u);
            }
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const bf16x8 b = *reinterpret_cast<const bf16x8*>(xt + (wave * 32 + n * 16 + c) * kLxGP + ks * 32 + g * 8);
#pragma unroll
                for (int mb = 0; mb < 4; ++mb)
                    if (mb < nb) acc[mb][n] = mfma_16x16x32<false>(a[mb][ks], b, acc[mb][n]);
            }
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int e = slab + wave * 32 + n * 16 + c;
        if (e < E) {
#pragma unroll
            for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int cls = mb * 16 + g * 4 + r;
                    if (cls < C) part[(chunk * C + cls) * (int64_t)E + e] = acc[mb][n][r];
                }
        }
    }
}

// d_w[idx] = the chunks' partials in ascending chunk order, idx over (class, column); no chunk at all (T == 0): zeros
static constexpr int kLxReduceLoads = 16;
template <bool F32>
__global__ __launch_bounds__(64) void lx_wgrad_reduce_kernel(const float* __restrict__ part, int64_t n_chunks, int64_t n, void* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (idx >= n) return;
    float v = 0.f;
    for (int64_t c0 = 0; c0 < n_chunks; c0 += kLxReduceLoads) {
        float p[kLxReduceLoads];
#pragma unroll
        for (int i = 0; i < kLxReduceLoads; ++i) p[i] = c0 + i < n_chunks ? part[(c0 + i) * n + idx] : 0.f;
#pragma unroll
        for (int i = 0; i < kLxReduceLoads; ++i) v += p[i];                           // [chunk-sum] ascending chunk order
    }
    if constexpr (F32) reinterpret_cast<float*>(out)[idx] = v;
    else reinterpret_cast<u16*>(out)[idx] = f2bf(v);                                  // [round]
}

// d_b[c] = the tiles' partials dbp[tile][c] in ascending tile order
template <bool F32>
__global__ __launch_bounds__(64) void lx_bgrad_reduce_kernel(const float* __restrict__ dbp, int64_t n_tiles, int C, void* __restrict__ out) {
    const int c = threadIdx.x;
    if (c >= C) return;
    float v = 0.f;
    for (int64_t t0 = 0; t0 < n_tiles; t0 += kLxReduceLoads) {
        float p[kLxReduceLoads];
#pragma unroll
        for (int i = 0; i < kLxReduceLoads; ++i) p[i] = t0 + i < n_tiles ? dbp[(t0 + i) * 64 + c] : 0.f;
#pragma unroll
        for (int i = 0; i < kLxReduceLoads; ++i) v += p[i];                           // [tile-sum] ascending tile order
    }
    if constexpr (F32) reinterpret_cast<float*>(out)[c] = v;
    else reinterpret_cast<u16*>(out)[c] = f2bf(v);                                    // [round]
}

}  // namespace esme

using namespace esme;

static int lx_check_sizes(int64_t T, int E, int C) {
    ESME_CHECK_ARG(T >= 0 && E > 0, "linear_xent: bad sizes");
    if (C < 1 || C > ESME_HIP_LINEAR_XENT_MAX_C) ESME_FAIL(ESME_ERR_UNSUPPORTED, "linear_xent: need 1 <= C <= 64 (one 64-wide MFMA column tile)");
    if (E % 8 != 0) ESME_FAIL(ESME_ERR_UNSUPPORTED, "linear_xent: E % 8 != 0");
    if (T >= 0x80000000LL) ESME_FAIL(ESME_ERR_UNSUPPORTED, "linear_xent: T >= 2^31");
    return ESME_OK;
}

static inline int64_t lx_tiles(int64_t T) { return (T + kLxTile - 1) / kLxTile; }
static inline int64_t lx_chunks(int64_t T) { return (T + kLxChunk - 1) / kLxChunk; }

struct LxWorkspace { int64_t wt, gt, dbp, dwp, total; };      // byte offsets of the backward's workspace
static LxWorkspace lx_layout(int64_t T, int E, int C) {
    LxWorkspace l;
    l.wt = 0;
    l.gt = l.wt + (int64_t)E * 64 * 2;
    l.dbp = l.gt + (int64_t)C * lx_tiles(T) * kLxTile * 2;
    l.dwp = l.dbp + lx_tiles(T) * 64 * 4;
    l.total = l.dwp + lx_chunks(T) * C * E * 4;
    return l;
}

extern "C" int64_t esme_hip_linear_xent_fwd_workspace_bytes(int64_t T) {
    ESME_CHECK_ARG(T >= 0, "linear_xent: bad sizes");
    if (T >= 0x80000000LL) ESME_FAIL(ESME_ERR_UNSUPPORTED, "linear_xent: T >= 2^31");
    return lx_tiles(T) * 2 * (int64_t)sizeof(float);
}

extern "C" int64_t esme_hip_linear_xent_bwd_workspace_bytes(int64_t T, int E, int C) {
    const int rc = lx_check_sizes(T, E, C);
    if (rc != ESME_OK) return rc;
    return T == 0 ? 0 : lx_layout(T, E, C).total;
}

static int lx_check_operands(const void* x, int64_t ld_x, const void* w, int64_t ld_w, const void* bias, const void* labels,
                             const float* class_weight, int64_t T, int E) {
    ESME_CHECK_ARG(w, "linear_xent: null pointer");
    ESME_CHECK_ARG(ld_w >= E && ld_w % 8 == 0, "linear_xent: bad row stride (need ld_w >= E, ld_w % 8 == 0)");
    ESME_CHECK_ARG(aligned16(w) && aligned16(bias) && aligned16(class_weight), "linear_xent: misaligned w, bias or class_weight");
    if (T > 0) {
        ESME_CHECK_ARG(x && labels, "linear_xent: null pointer");
        ESME_CHECK_ARG(ld_x >= E && ld_x % 8 == 0, "linear_xent: bad row stride (need ld_x >= E, ld_x % 8 == 0)");
        ESME_CHECK_ARG(aligned16(x) && aligned16(labels), "linear_xent: misaligned x or labels");
    }
    return ESME_OK;
}

extern "C" int esme_hip_linear_xent_fwd(const void* x, int64_t ld_x, const void* w, int64_t ld_w, const void* bias, const void* labels,
                                        int labels_i64, int64_t ignore_index, const float* class_weight, int64_t T, int E, int C, int mean,
                                        float* loss_rows, float* lse, float* sums, void* workspace, int64_t ws_bytes, void* stream) {
    int rc = lx_check_sizes(T, E, C);
    if (rc != ESME_OK) return rc;
    if ((rc = lx_check_operands(x, ld_x, w, ld_w, bias, labels, class_weight, T, E)) != ESME_OK) return rc;
    ESME_CHECK_ARG(sums && aligned16(sums), "linear_xent_fwd: sums null or misaligned");
    const hipStream_t st = (hipStream_t)stream;
    const int64_t tiles = lx_tiles(T);
    if (T > 0) {
        ESME_CHECK_ARG(loss_rows && lse && workspace, "linear_xent_fwd: null pointer");
        ESME_CHECK_ARG(aligned16(loss_rows) && aligned16(lse) && aligned16(workspace), "linear_xent_fwd: misaligned loss_rows, lse or workspace");
        ESME_CHECK_ARG(ws_bytes >= tiles * 2 * (int64_t)sizeof(float), "linear_xent_fwd: workspace too small (see esme_hip_linear_xent_fwd_workspace_bytes)");
        hipLaunchKernelGGL(lx_fwd_kernel, dim3((unsigned int)tiles), dim3(256), 0, st, (const u16*)x, ld_x, (const u16*)w, ld_w, (const u16*)bias,
                           labels, labels_i64, ignore_index, class_weight, T, E, C, loss_rows, lse, (float*)workspace);
    }
    hipLaunchKernelGGL(lx_sum_kernel, dim3(1), dim3(64), 0, st, (const float*)workspace, tiles, mean, sums);
    return check_launch("linear_xent_fwd");
}

extern "C" int esme_hip_linear_xent_bwd(const void* x, int64_t ld_x, const void* w, int64_t ld_w, const void* bias, const void* labels,
                                        int labels_i64, int64_t ignore_index, const float* class_weight, int64_t T, int E, int C, int mean,
                                        const float* lse, const float* sums, const float* grad, int want_dx, void* d_x, int64_t ld_dx,
                                        int want_dw, void* d_w, void* d_b, int out_f32, void* workspace, int64_t ws_bytes, void* stream) {
    int rc = lx_check_sizes(T, E, C);
    if (rc != ESME_OK) return rc;
    if ((rc = lx_check_operands(x, ld_x, w, ld_w, bias, labels, class_weight, T, E)) != ESME_OK) return rc;
    ESME_CHECK_ARG(sums && grad && aligned16(sums) && aligned16(grad), "linear_xent_bwd: sums or grad null or misaligned");
    if (want_dw) ESME_CHECK_ARG(d_w && aligned16(d_w) && aligned16(d_b), "linear_xent_bwd: d_w null, or d_w / d_b misaligned");
    if (want_dx && T > 0) {
        ESME_CHECK_ARG(d_x && aligned16(d_x), "linear_xent_bwd: d_x null or misaligned");
        ESME_CHECK_ARG(ld_dx >= E && ld_dx % 8 == 0, "linear_xent_bwd: bad row stride (need ld_dx >= E, ld_dx % 8 == 0)");
    }
    const hipStream_t st = (hipStream_t)stream;
    const int64_t tiles = lx_tiles(T), chunks = lx_chunks(T), n = (int64_t)C * E;
    const LxWorkspace l = lx_layout(T, E, C);
    char* ws = (char*)workspace;
    if (T > 0 && (want_dx || want_dw)) {
        ESME_CHECK_ARG(lse && workspace, "linear_xent_bwd: null pointer");
        ESME_CHECK_ARG(aligned16(lse) && aligned16(workspace), "linear_xent_bwd: misaligned lse or workspace");
        ESME_CHECK_ARG(ws_bytes >= l.total, "linear_xent_bwd: workspace too small (see esme_hip_linear_xent_bwd_workspace_bytes)");
        u16* wt = (u16*)(ws + l.wt);
        u16* gt = (u16*)(ws + l.gt);
        float* dbp = (float*)(ws + l.dbp);
        if (want_dx) hipLaunchKernelGGL(lx_wt_kernel, dim3((unsigned int)((E * 64 + 255) / 256)), dim3(256), 0, st, (const u16*)w, ld_w, E, C, wt);
        rc = dispatch_flags([&](auto dxf, auto dwf) {
            hipLaunchKernelGGL((lx_bwd_kernel<decltype(dxf)::value, decltype(dwf)::value>), dim3((unsigned int)tiles), dim3(256), 0, st,
                               (const u16*)x, ld_x, (const u16*)w, ld_w, (const u16*)bias, labels, labels_i64, ignore_index, class_weight, T, E, C,
                               mean, lse, sums, grad, (const u16*)wt, (u16*)d_x, ld_dx, gt, tiles * kLxTile, dbp);
            return ESME_OK;
        }, want_dx != 0, want_dw != 0);
        if (rc != ESME_OK) return rc;
        if (want_dw)
            hipLaunchKernelGGL(lx_wgrad_kernel, dim3((unsigned int)((E + kLxKC - 1) / kLxKC), (unsigned int)chunks), dim3(256), 0, st, (const u16*)x,
                               ld_x, (const u16*)gt, tiles * kLxTile, T, E, C, (float*)(ws + l.dwp));
    }
    if (want_dw) {
        const float* dwp = T > 0 ? (const float*)(ws + l.dwp) : nullptr;
        const float* dbp = T > 0 ? (const float*)(ws + l.dbp) : nullptr;
        if (out_f32) {
            hipLaunchKernelGGL(lx_wgrad_reduce_kernel<true>, dim3((unsigned int)((n + 63) / 64)), dim3(64), 0, st, dwp, chunks, n, d_w);
            if (d_b) hipLaunchKernelGGL(lx_bgrad_reduce_kernel<true>, dim3(1), dim3(64), 0, st, dbp, tiles, C, d_b);
        } else {
            hipLaunchKernelGGL(lx_wgrad_reduce_kernel<false>, dim3((unsigned int)((n + 63) / 64)), dim3(64), 0, st, dwp, chunks, n, d_w);
            if (d_b) hipLaunchKernelGGL(lx_bgrad_reduce_kernel<false>, dim3(1), dim3(64), 0, st, dbp, tiles, C, d_b);
        }
    }
    return check_launch("linear_xent_bwd");
}
