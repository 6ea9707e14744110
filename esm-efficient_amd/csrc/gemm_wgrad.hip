// Weight gradient dW = dY^T X and bias gradient db = column sums of dY (include/esme_hip_gemm_wgrad.h).
//
// The contraction index is the ROW of both operands, so neither lies in memory the way an MFMA operand wants it (lane = row or
// column, 8 consecutive contraction indices per lane).  The tiles are therefore staged in LDS exactly as they lie in memory,
// [row t][128 columns] with 16-byte global loads and 16-byte LDS stores, and every fragment is gathered by two transposing reads
// (ds_read_b64_tr_b16: per 16-lane group a [4 rows][16 columns] block, lane 4q + p supplies row q / columns 4p..4p+3, lane c
// receives column c of the 4 rows).  For the 16x16x32 MFMA, lane (c = lane & 15, g = lane >> 4) wants column c at rows 8g..8g+7 of a
// 32-row step: group g reads rows 8g..8g+3 and 8g+4..8g+7.  The image is the plain 256-byte-row one with the 16-byte chunk index
// XORed by ((row & 3) << 2) | ((row >> 2) & 3): a 32-lane half's two blocks lie 8 rows apart in the same columns, which that image
// serves without bank conflicts.
//  - wgrad_tile_kernel: one workgroup per (row chunk, N tile, K tile), 4 waves, each a 64 x 64 quarter of the 128 x 128 tile of dW as 4 x 4
//    MFMA blocks.  The A operand is X^T (rows = k), the B operand dY (columns = n): a lane then holds 4 CONSECUTIVE k of one row n of
//    dW and stores them as one 8- or 16-byte word.  A wave whose quarter lies outside N x K (a width that is 64 mod 128) issues no
//    MFMA.  A stage is 64 rows in one of two LDS buffers; the next stage's global loads are in flight while the current one is
//    multiplied, and there is one barrier per stage.  Rows at or past
//    the chunk's end are zero-filled in LDS, never masked: the transposing read needs EXEC all ones.
//  - wgrad_reduce_kernel: dW and db = the chunks' fp32 partials in chunk order, rounded once.
// No atomics, and the partition of the rows is a function of (M, N, K) only (wgrad_split): bit-equal from run to run, box to box.
#include "common.h"
#include "launch.h"
#include "../../include/esme_hip_gemm_wgrad.h"

namespace esme {

static constexpr int kWgTile = 128;        // columns of dY / of X per workgroup
static constexpr int kWgRows = 64;         // rows per stage
static constexpr int kWgRowB = 256;        // bytes of an LDS row
static constexpr int kWgTarget = 512;      // workgroups of one round the split fills (a constant: never the device's CU count)
static constexpr int kWgMaxChunks = 64;    // most chunks
static constexpr int kWgMaxWork = 2048;    // ... and most workgroups (tiles * chunks) a split may create: bounds the workspace
static constexpr int kWgMinRows = 256;     // a chunk is not cut below this many rows
static constexpr int kWgGroup = 8;         // N tiles per group of the tile walk

struct WgradSplit { int64_t rows; int chunks; };

// c, the number of chunks aimed at: among 1 .. min(kWgMaxChunks, max(1, kWgMaxWork / tiles), ceil(M / kWgMinRows)) the smallest c that
// maximises tiles * c / (kWgTarget * ceil(tiles * c / kWgTarget)), the share of the last round of kWgTarget workgroups that does work.
static WgradSplit wgrad_split(int64_t M, int N, int K) {
    const int64_t tiles = (int64_t)((N + kWgTile - 1) / kWgTile) * ((K + kWgTile - 1) / kWgTile);
    int64_t most = (M + kWgMinRows - 1) / kWgMinRows;
    const int64_t by_work = kWgMaxWork / tiles > 1 ? kWgMaxWork / tiles : 1;
    if (most > by_work) most = by_work;
    if (most > kWgMaxChunks) most = kWgMaxChunks;
    int64_t c = 1, ba = 0, bb = 1;                                  // the best share so far, ba / bb
    for (int64_t i = 1; i <= most; ++i) {
        const int64_t a = tiles * i, b = kWgTarget * ((a + kWgTarget - 1) / kWgTarget);
        if (a * bb > ba * b) { c = i; ba = a; bb = b; }
    }
    int64_t rows = ((M + c - 1) / c + kWgRows - 1) / kWgRows * kWgRows;
    if (rows < kWgRows) rows = kWgRows;
    const int64_t chunks = (M + rows - 1) / rows;
    return {rows, (int)(chunks < 1 ? 1 : chunks)};
}

// byte offset of 16-byte chunk ch (0..15) of row `row` in a [rows][128 x bf16] image
__device__ __forceinline__ int wg_off(const int row, const int ch) { return kWgRowB * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

enum { kWgPartial = 0, kWgBf16 = 1, kWgF32 = 2 };   // what the tile kernel writes: fp32 partials of its chunk, or dW itself

__global__ __launch_bounds__(256, 2) void wgrad_tile_kernel(const u16* __restrict__ dy, int64_t ld_dy, const u16* __restrict__ x, int64_t ld_x,
                                                         int64_t M, int N, int K, int64_t chunk_rows, void* __restrict__ out, int64_t ld_out,
                                                         void* __restrict__ dbo, int mode) {
    __shared__ __attribute__((aligned(16))) char lds[2][2 * kWgRows * kWgRowB];   // two stages, each the X image, then the dY image
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    // Workgroup -> (chunk, N tile, K tile).  Workgroup b runs on XCD b % 8 (xcd_remap): each XCD, with its own L2, gets a contiguous range
    // of ids, and ids walk the tiles of a chunk in groups of kWgGroup N tiles with the N tile fastest, so the workgroups that share an
    // L2 at one time cover a compact block of tiles and re-read each other's dY and X stages from it.  Speed only: every (chunk, tile)
    // is computed by exactly one workgroup, whichever it is.
    const int nt = (N + kWgTile - 1) / kWgTile, kt = (K + kWgTile - 1) / kWgTile;
    const unsigned int id = xcd_remap(blockIdx.x, gridDim.x);
    const int chunk = id / (unsigned int)(nt * kt), tile = id % (unsigned int)(nt * kt);
    const int grp = tile / (kWgGroup * kt), n_first = grp * kWgGroup, rem = tile - grp * kWgGroup * kt;
    const int gh = nt - n_first < kWgGroup ? nt - n_first : kWgGroup;
    const int n_tile = n_first + rem % gh, k_tile = rem / gh;
    const int k0 = k_tile * kWgTile, n0 = n_tile * kWgTile;
    const int64_t r_begin = (int64_t)chunk * chunk_rows;
    const int64_t r_end = r_begin + chunk_rows < M ? r_begin + chunk_rows : M;
    const int wk = wave & 1, wn = wave >> 1;                                      // the wave's quarter: k from wk * 64, n from wn * 64
    const bool active = k0 + wk * 64 < K && n0 + wn * 64 < N;                     // (wave-uniform)
    const bool want_db = dbo != nullptr && k_tile == 0 && wk == 0 && n0 + wn * 64 < N;

    // loader: thread t carries 16-byte chunk ch of rows lr, lr + 16, lr + 32, lr + 48 of the stage, of both operands
    const int ch = t & 15, lr = t >> 4;
    const bool xcol = k0 + ch * 8 < K, ycol = n0 + ch * 8 < N;                    // (K, N are multiples of 64: a chunk is inside or outside)
    const u16* const xg = x + k0 + ch * 8;
    const u16* const yg = dy + n0 + ch * 8;
    u32x4 xr[4], yr[4];
    auto gload = [&](const int64_t r0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = r0 + lr + 16 * j;
            const bool in = row < r_end;
            const u32x4 z = {0u, 0u, 0u, 0u};
            xr[j] = (in && xcol) ? *reinterpret_cast<const u32x4*>(xg + row * ld_x) : z;
            yr[j] = (in && ycol) ? *reinterpret_cast<const u32x4*>(yg + row * ld_dy) : z;
        }
    };
    auto lstore = [&](char* stage) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = wg_off(lr + 16 * j, ch);
            *reinterpret_cast<u32x4*>(stage + o) = xr[j];
            *reinterpret_cast<u32x4*>(stage + kWgRows * kWgRowB + o) = yr[j];
        }
    };
    // fragment of 16 columns from chunk c0 (two chunks) at the rows of 32-row step ks: column c = lane & 15, rows 8g .. 8g + 7
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) s16x4* ltr_t;
    const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    auto frag = [&](const char* img, const int c0, const int ks) -> bf16x8 {
        const int r = ks * 32 + g * 8 + q;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ltr_t)(img + wg_off(r, c0 + (p >> 1)) + 8 * (p & 1)));
        const s16x4 up = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ltr_t)(img + wg_off(r + 4, c0 + (p >> 1)) + 8 * (p & 1)));
        return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, up, 0, 1, 2, 3, 4, 5, 6, 7));
    };

    f32x4 acc[4][4], dba[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        dba[a] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const short one = 0x3f80;                                                     // bf16 1.0
    const bf16x8 ones = __builtin_bit_cast(bf16x8, (short __attribute__((ext_vector_type(8)))){one, one, one, one, one, one, one, one});

    // One barrier per stage: while stage s is multiplied out of one LDS buffer, the global loads of stage s + 1 are in flight; they are
    // stored to the other buffer, which every wave finished reading before the barrier that ended stage s - 1.
    if (r_begin < r_end) { gload(r_begin); lstore(lds[0]); }
    __syncthreads();
    int cur = 0;
    for (int64_t r0 = r_begin; r0 < r_end; r0 += kWgRows, cur ^= 1) {             // (block-uniform trip count)
        const bool more = r0 + kWgRows < r_end;
        if (more) gload(r0 + kWgRows);
        if (active) {
            const char* const xs = lds[cur];
            const char* const ys = lds[cur] + kWgRows * kWgRowB;
#pragma unroll
            for (int ks = 0; ks < kWgRows / 32; ++ks) {
                bf16x8 xf[4], yf[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    xf[b] = frag(xs, wk * 8 + b * 2, ks);
                    yf[b] = frag(ys, wn * 8 + b * 2, ks);
                }
#pragma unroll
                for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb) acc[kb][nb] = mfma_16x16x32<false>(xf[kb], yf[nb], acc[kb][nb]);
                if (want_db) {                                                    // (wave-uniform)
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb) dba[nb] = mfma_16x16x32<false>(ones, yf[nb], dba[nb]);
                }
            }
        }
        if (more) lstore(lds[cur ^ 1]);
        __syncthreads();
    }
    if (!active) return;

    // acc[kb][nb][i] = dW[n = n0 + wn 64 + nb 16 + c][k = k0 + wk 64 + kb 16 + 4 g + i]
    const int c = lane & 15;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        const int n = n0 + wn * 64 + nb * 16 + c;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const int k = k0 + wk * 64 + kb * 16 + 4 * g;
            const f32x4 v = acc[kb][nb];
            if (mode == kWgPartial) *reinterpret_cast<f32x4*>((float*)out + ((int64_t)chunk * N + n) * K + k) = v;
            else if (mode == kWgF32) *reinterpret_cast<f32x4*>((float*)out + (int64_t)n * ld_out + k) = v;
            else *reinterpret_cast<u32x2*>((u16*)out + (int64_t)n * ld_out + k) = u32x2{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3])};
        }
        if (want_db && g == 0) {                                                  // every row of the ones product holds the column sum
            const float s = dba[nb][0];
            if (mode == kWgPartial) ((float*)dbo)[(int64_t)chunk * N + n] = s;
            else if (mode == kWgF32) ((float*)dbo)[n] = s;
            else ((u16*)dbo)[n] = f2bf(s);
        }
    }
}

// One thread per 4 consecutive k of a row of dW, then one per element of db: the chunks' partials in chunk order.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ dbpart, int chunks, int N,
                                                           int K, void* __restrict__ dw, int64_t ld_dw, void* __restrict__ db, int f32) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k4 = K >> 2;
    const int64_t nw = (int64_t)N * k4, nk = (int64_t)N * K;
    if (idx < nw) {
        const int64_t n = idx / k4;
        const int k = (int)(idx % k4) * 4;
        const float* src = part + n * K + k;
        f32x4 v = *reinterpret_cast<const f32x4*>(src);
        for (int cidx = 1; cidx < chunks; ++cidx) v += *reinterpret_cast<const f32x4*>(src + cidx * nk);
        if (f32) *reinterpret_cast<f32x4*>((float*)dw + n * ld_dw + k) = v;
        else *reinterpret_cast<u32x2*>((u16*)dw + n * ld_dw + k) = u32x2{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3])};
    } else if (db != nullptr && idx < nw + N) {
        const int n = (int)(idx - nw);
        float s = dbpart[n];
        for (int cidx = 1; cidx < chunks; ++cidx) s += dbpart[(int64_t)cidx * N + n];
        if (f32) ((float*)db)[n] = s;
        else ((u16*)db)[n] = f2bf(s);
    }
}

static int wgrad_check_geometry(int64_t M, int N, int K) {
    ESME_CHECK_ARG(M >= 0 && M < (1LL << 31) && N > 0 && K > 0, "gemm_wgrad: need 0 <= M < 2^31, N > 0, K > 0");
    if (N % 64 || K % 64) ESME_FAIL(ESME_ERR_UNSUPPORTED, "gemm_wgrad: N and K must be multiples of 64");
    return ESME_OK;
}

}  // namespace esme

using namespace esme;

extern "C" int64_t esme_hip_gemm_wgrad_workspace_bytes(int64_t M, int N, int K) {
    const int rc = wgrad_check_geometry(M, N, K);
    if (rc != ESME_OK) return rc;
    const WgradSplit s = wgrad_split(M, N, K);
    return s.chunks == 1 ? 0 : (int64_t)s.chunks * ((int64_t)N * K + N) * (int64_t)sizeof(float);
}

extern "C" int esme_hip_gemm_wgrad(const void* dy, int64_t ld_dy, const void* x, int64_t ld_x, int64_t M, int N, int K, void* dw,
                                   int64_t ld_dw, void* db, int out_f32, void* workspace, int64_t ws_bytes, void* stream) {
    const int rc = wgrad_check_geometry(M, N, K);
    if (rc != ESME_OK) return rc;
    ESME_CHECK_ARG(dw && (M == 0 || (dy && x)), "gemm_wgrad: null pointer");
    ESME_CHECK_ARG(ld_dy >= N && ld_x >= K && ld_dw >= K, "gemm_wgrad: a row stride is smaller than its width");
    ESME_CHECK_ARG(ld_dy % 8 == 0 && ld_x % 8 == 0 && ld_dw % 8 == 0, "gemm_wgrad: row strides must be multiples of 8");
    ESME_CHECK_ARG(aligned16(dy) && aligned16(x) && aligned16(dw) && aligned16(db) && aligned16(workspace),
                   "gemm_wgrad: misaligned dy, x, dw, db or workspace (16 bytes)");
    const WgradSplit s = wgrad_split(M, N, K);
    const int64_t need = s.chunks == 1 ? 0 : (int64_t)s.chunks * ((int64_t)N * K + N) * (int64_t)sizeof(float);
    ESME_CHECK_ARG(ws_bytes >= need && (need == 0 || workspace), "gemm_wgrad: workspace too small (see esme_hip_gemm_wgrad_workspace_bytes)");
    const int nt = (N + kWgTile - 1) / kWgTile, kt = (K + kWgTile - 1) / kWgTile;
    if ((int64_t)nt * kt * s.chunks > 0x7fffffffLL) ESME_FAIL(ESME_ERR_UNSUPPORTED, "gemm_wgrad: too many tiles");
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned int)(nt * kt * s.chunks));
    if (s.chunks == 1) {
        hipLaunchKernelGGL(wgrad_tile_kernel, grid, dim3(256), 0, st, (const u16*)dy, ld_dy, (const u16*)x, ld_x, M, N, K, s.rows, dw, ld_dw,
                           db, out_f32 ? kWgF32 : kWgBf16);
        return check_launch("gemm_wgrad");
    }
    float* part = (float*)workspace;
    float* dbpart = part + (int64_t)s.chunks * N * K;
    hipLaunchKernelGGL(wgrad_tile_kernel, grid, dim3(256), 0, st, (const u16*)dy, ld_dy, (const u16*)x, ld_x, M, N, K, s.rows, (void*)part,
                       (int64_t)K, db ? (void*)dbpart : nullptr, (int)kWgPartial);
    const int64_t threads = (int64_t)N * (K / 4) + N;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned int)((threads + 255) / 256)), dim3(256), 0, st, (const float*)part,
                       (const float*)dbpart, s.chunks, N, K, dw, ld_dw, db, out_f32 ? 1 : 0);
    return check_launch("gemm_wgrad");
}
