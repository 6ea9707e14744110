// Backward of attention pooling (include/esme_hip_attn_pool_bwd.h; the forward and its algebra: pool.hip).
//
// out is differentiated as the function of (x, U) the forward kernel computes, sigma_tj = U_j . x_t in log2 units:
//     dP_tj = sum_i dO[s, c, h d + i] x_t[h d + i],  Delta_sj = sum_t p_tj dP_tj,  dsigma_tj = ln2 p_tj (dP_tj - Delta_sj),
//     dU_j = sum_t dsigma_tj x_t,   dX_t[e] = sum_j dsigma_tj U_j[e] + sum_c p_{t,(c,h(e))} dO[s, c, e].
// Work items are the forward's slots (pool.h): chunks of kPoolRows rows that start at the sequence's own first row.
//  - attn_pool_bwd_chunk_kernel: one workgroup per slot: sigma (the forward's score pass) and dP of the chunk's rows into the
//    workspace, and per (c, h) the chunk's {max, sum 2^(sigma - max), sum 2^(sigma - max) dP};
//  - attn_pool_bwd_grad_kernel: one workgroup per (slot, 256 columns of E): the sequence's {max, 1 / sum, Delta} from its chunks
//    in chunk order, then dsigma tiles through LDS; a thread owns one column e, keeps the chunk's x[:, e] in registers and
//    accumulates the chunk's partial of dU[:, e] and, when dX is wanted, the chunk's 64 rows of dX[:, e];
//  - attn_pool_bwd_reduce_kernel: dU = the partials of the slots that hold rows, in slot order.
// No atomics; every sum has a fixed order, so dX and dU are bit-equal from run to run and a sequence's dX does not depend on its
// neighbours.  Delta comes from the recomputed p and dP in fp32, never from the rounded forward output.
#include "pool.h"
#include "../../include/esme_hip_attn_pool_bwd.h"

namespace esme {

static constexpr int kPoolBwdJ = 16;      // query columns per dsigma tile of the gradient kernel
static constexpr float kLn2 = 0.6931471805599453f;

// Workspace, per slot g: meta[g] = {sequence, rows of the chunk (0: the slot holds no chunk)}, st[g][J][3] = {max, sum, delta part},
// sig[g][R][J] = sigma, dp[g][R][J] = dP, part[g][J][E] = the chunk's partial of dU.
template <bool F32>
__global__ __launch_bounds__(256) void attn_pool_bwd_chunk_kernel(const void* __restrict__ x, int64_t ldx, const int32_t* __restrict__ cu,
                                                                  int B, int E, int H, int d, int J, const float* __restrict__ U,
                                                                  const void* __restrict__ dout, int64_t ldg,
                                                                  int32_t* __restrict__ ws_meta, float* __restrict__ ws_st,
                                                                  float* __restrict__ ws_sig, float* __restrict__ ws_dp) {
    __shared__ float xs[kPoolK][kPoolRows + 4];   // x slab, k-major
    __shared__ float us[kPoolK][kPoolJ + 4];      // U slab, k-major
    __shared__ float sc[kPoolRows][kPoolJ + 1];   // sigma
    __shared__ float dp[kPoolRows][kPoolJ + 1];   // dP
    __shared__ int64_t sh_row0;
    __shared__ int sh_rows, sh_seq;
    const int t = threadIdx.x;
    const int64_t g = blockIdx.x;
    if (t == 0) {                                  // slot -> (sequence, chunk): the largest s with first_slot(s) <= g
        int lo = 0, hi = B - 1;
        while (lo < hi) {
            const int mid = lo + (hi - lo + 1) / 2;
            if (pool_first_slot(cu, mid) <= g) lo = mid; else hi = mid - 1;
        }
        const int64_t chunk = g - pool_first_slot(cu, lo);
        const int64_t len = (int64_t)cu[lo + 1] - cu[lo];
        const int64_t rows = len - chunk * kPoolRows;
        sh_rows = (chunk < 0 || rows <= 0) ? 0 : (int)(rows < kPoolRows ? rows : kPoolRows);
        sh_row0 = (int64_t)cu[lo] + chunk * kPoolRows;
        sh_seq = lo;
        ws_meta[g * 2] = lo;                       // every slot states whether it holds rows: the later kernels read nothing else of an empty one
        ws_meta[g * 2 + 1] = sh_rows;
    }
    __syncthreads();
    const int nrows = sh_rows;
    if (nrows == 0) return;                        // past the sequence's last chunk (block-uniform)
    const int64_t row0 = sh_row0;
    const int64_t seq = sh_seq;
    float* st = ws_st + g * (int64_t)J * 3;
    float* sig = ws_sig + g * (int64_t)kPoolRows * J;
    float* dpo = ws_dp + g * (int64_t)kPoolRows * J;

    const int lr = t >> 2, lc = (t & 3) * 8;       // slab loader: x row / U row lr, 8 columns from lc
    const int rq = t & 15, jq = t >> 4;            // score tile: rows rq*4.., query columns jq*4..
    for (int g0 = 0; g0 < J; g0 += kPoolJ) {
        const int jn = J - g0 < kPoolJ ? J - g0 : kPoolJ;
        const bool active = jq * 4 < jn;
        float acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
        for (int k0 = 0; k0 < E; k0 += kPoolK) {
            float f[8];
            if (lr < nrows && k0 + lc < E) load8<F32>(x, (row0 + lr) * ldx + k0 + lc, f);
            else {
#pragma unroll
                for (int i = 0; i < 8; ++i) f[i] = 0.f;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) xs[lc + i][lr] = f[i];
            if (lr < jn && k0 + lc < E) {
                const float* up = U + (int64_t)(g0 + lr) * E + k0 + lc;
                const f32x4 u0 = *reinterpret_cast<const f32x4*>(up), u1 = *reinterpret_cast<const f32x4*>(up + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) { f[i] = u0[i]; f[4 + i] = u1[i]; }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) f[i] = 0.f;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) us[lc + i][lr] = f[i];
            __syncthreads();
            if (active) {
                const int kn = E - k0 < kPoolK ? E - k0 : kPoolK;
                for (int k = 0; k < kn; ++k) {      // [score] fp32 fmaf chain over e in order (the forward's)
                    const f32x4 a = *reinterpret_cast<const f32x4*>(&xs[k][rq * 4]);
                    const f32x4 b = *reinterpret_cast<const f32x4*>(&us[k][jq * 4]);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) acc[i][jj] = fmaf(a[i], b[jj], acc[i][jj]);
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) sc[rq * 4 + i][jq * 4 + jj] = acc[i][jj];
        __syncthreads();
        for (int q = t; q < nrows * jn; q += 256) {   // dP[r, j] = dO[s, c, h d : (h + 1) d] . x[r, h d : (h + 1) d]
            const int r = q / jn, jj = q % jn;
            const int j = g0 + jj, c = j / H, col = (j % H) * d;
            const int64_t xo = (row0 + r) * ldx + col, go = seq * ldg + (int64_t)c * E + col;
            float s = 0.f;
            for (int i = 0; i < d; ++i) s = fmaf(load1<F32>(dout, go + i), load1<F32>(x, xo + i), s);   // [dp] fp32 fmaf chain over i in order
            dp[r][jj] = s;
            dpo[(int64_t)r * J + j] = s;
            sig[(int64_t)r * J + j] = sc[r][jj];
        }
        __syncthreads();
        if (t < jn) {                              // per query column, over the chunk's rows in row order
            float m = -INFINITY;
            for (int r = 0; r < nrows; ++r) m = fmaxf(m, sc[r][t]);
            float l = 0.f, dl = 0.f;
            for (int r = 0; r < nrows; ++r) {
                const float p = exp2f(sc[r][t] - m);   // [chunk-exp]
                l += p;                                 // [chunk-sum]
                dl = fmaf(p, dp[r][t], dl);             // [chunk-delta]
            }
            st[(int64_t)(g0 + t) * 3] = m;
            st[(int64_t)(g0 + t) * 3 + 1] = l;
            st[(int64_t)(g0 + t) * 3 + 2] = dl;
        }
        __syncthreads();
    }
}

// Grid (slots, ceil(E / 256)).  Thread t owns column e = 256 blockIdx.y + t of the chunk.
template <bool F32, bool DX>
__global__ __launch_bounds__(256) void attn_pool_bwd_grad_kernel(const void* __restrict__ x, int64_t ldx, const int32_t* __restrict__ cu,
                                                                 int E, int H, int d, int J, const float* __restrict__ U,
                                                                 const void* __restrict__ dout, int64_t ldg,
                                                                 const int32_t* __restrict__ ws_meta, const float* __restrict__ ws_st,
                                                                 const float* __restrict__ ws_sig, const float* __restrict__ ws_dp,
                                                                 float* __restrict__ ws_part, int64_t n_slots, void* __restrict__ dx,
                                                                 int64_t lddx) {
    __shared__ float s_m[kPoolMaxJ], s_il[kPoolMaxJ], s_delta[kPoolMaxJ];   // per j: the sequence's max, 1 / sum, Delta
    __shared__ float ds[kPoolBwdJ][kPoolRows + 4];                          // dsigma tile, j-major
    const int t = threadIdx.x;
    const int64_t g = blockIdx.x;
    const int seq = ws_meta[g * 2], nrows = ws_meta[g * 2 + 1];
    if (nrows == 0) return;                        // the slot holds no chunk (block-uniform)
    const int64_t first = pool_first_slot(cu, seq);
    const int64_t len = (int64_t)cu[seq + 1] - cu[seq];
    int64_t nch = (len + kPoolRows - 1) / kPoolRows;
    if (first + nch > n_slots) nch = n_slots - first;       // (cu_lens past T: only the slots that were launched, as the forward's combine)
    const int64_t row0 = (int64_t)cu[seq] + (g - first) * kPoolRows;
    for (int j = t; j < J; j += 256) {             // the sequence's statistics from its chunks, in chunk order
        float m = -INFINITY;
        for (int64_t k = 0; k < nch; ++k) m = fmaxf(m, ws_st[((first + k) * J + j) * 3]);
        float l = 0.f, dl = 0.f;
        for (int64_t k = 0; k < nch; ++k) {
            const float* sk = ws_st + ((first + k) * J + j) * 3;
            const float a = exp2f(sk[0] - m);      // [stat-exp]
            l = fmaf(a, sk[1], l);                 // [stat-sum]
            dl = fmaf(a, sk[2], dl);               // [stat-delta]
        }
        const float il = 1.f / l;                  // [inv-l]
        s_m[j] = m;
        s_il[j] = il;
        s_delta[j] = dl * il;                      // [delta]
    }
    __syncthreads();
    const float* sig = ws_sig + g * (int64_t)kPoolRows * J;
    const float* dpo = ws_dp + g * (int64_t)kPoolRows * J;
    float* part = ws_part + g * (int64_t)J * E;
    const int e = blockIdx.y * 256 + t;
    const bool valid = e < E;
    float xc[kPoolRows], acc[DX ? kPoolRows : 1];
#pragma unroll
    for (int r = 0; r < kPoolRows; ++r) xc[r] = (valid && r < nrows) ? load1<F32>(x, (row0 + r) * ldx + e) : 0.f;
    if constexpr (DX) {
#pragma unroll
        for (int r = 0; r < kPoolRows; ++r) acc[r] = 0.f;
    }
    for (int j0 = 0; j0 < J; j0 += kPoolBwdJ) {
        const int jn = J - j0 < kPoolBwdJ ? J - j0 : kPoolBwdJ;
        for (int q = t; q < kPoolBwdJ * kPoolRows; q += 256) {
            const int jj = q / kPoolRows, r = q % kPoolRows;
            float v = 0.f;
            if (jj < jn && r < nrows) {
                const int j = j0 + jj;
                const float p = exp2f(sig[(int64_t)r * J + j] - s_m[j]) * s_il[j];     // [p-exp] [p-norm]
                v = kLn2 * p * (dpo[(int64_t)r * J + j] - s_delta[j]);                  // [dsigma] a subtraction and two products
            }
            ds[jj][r] = v;
        }
        __syncthreads();
        if (valid) {
#pragma unroll
            for (int jj = 0; jj < kPoolBwdJ; ++jj) {
                if (jj < jn) {                     // block-uniform
                    const float u = DX ? U[(int64_t)(j0 + jj) * E + e] : 0.f;
                    float au = 0.f;
#pragma unroll
                    for (int r4 = 0; r4 < kPoolRows / 4; ++r4) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(&ds[jj][r4 * 4]);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            au = fmaf(v[i], xc[r4 * 4 + i], au);                        // [du-chunk] row order
                            if constexpr (DX) acc[r4 * 4 + i] = fmaf(v[i], u, acc[r4 * 4 + i]);   // [dx-score] j order
                        }
                    }
                    part[(int64_t)(j0 + jj) * E + e] = au;
                }
            }
        }
        __syncthreads();
    }
    if constexpr (DX) if (valid) {
        const int n_cls = J / H, h = e / d;
        for (int c = 0; c < n_cls; ++c) {          // the value path, class tokens in order
            const int j = c * H + h;
            const float go = load1<F32>(dout, (int64_t)seq * ldg + (int64_t)c * E + e);
            const float m = s_m[j], il = s_il[j];
#pragma unroll
            for (int r = 0; r < kPoolRows; ++r)
                if (r < nrows) acc[r] = fmaf(exp2f(sig[(int64_t)r * J + j] - m) * il, go, acc[r]);   // [dx-value]
        }
#pragma unroll
        for (int r = 0; r < kPoolRows; ++r) {
            if (r < nrows) {
                const int64_t o = (row0 + r) * lddx + e;
                if (F32) ((float*)dx)[o] = acc[r];
                else ((u16*)dx)[o] = f2bf(acc[r]);                                      // [dx-round]
            }
        }
    }
}

// dU[j, e] = sum over the slots that hold rows, in slot order.  One thread per (j, e); eight slots' loads are in flight at a time (a slot
// without rows enters as +0, which changes no bit of the sum).
__global__ __launch_bounds__(64) void attn_pool_bwd_reduce_kernel(const int32_t* __restrict__ ws_meta, const float* __restrict__ ws_part,
                                                                  int64_t n_slots, int64_t n, float* __restrict__ dU) {
    const int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (idx >= n) return;
    float v = 0.f;
    for (int64_t g0 = 0; g0 < n_slots; g0 += 8) {
        float p[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i] = (g0 + i < n_slots && ws_meta[(g0 + i) * 2 + 1] > 0) ? ws_part[(g0 + i) * n + idx] : 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) v += p[i];                                          // [du-sum]
    }
    dU[idx] = v;
}

}  // namespace esme

using namespace esme;

static int64_t pool_bwd_slot_floats(int E, int64_t J) { return 2 + 3 * J + 2 * (int64_t)kPoolRows * J + J * E; }

extern "C" int64_t esme_hip_attn_pool_bwd_workspace_bytes(int B, int64_t T, int E, int heads, int n_cls) {
    const int rc = pool_check_geometry(B, T, E, heads, n_cls);
    if (rc != ESME_OK) return rc;
    return pool_slots(B, T) * pool_bwd_slot_floats(E, (int64_t)n_cls * heads) * (int64_t)sizeof(float);
}

extern "C" int esme_hip_attn_pool_bwd(const void* x, int64_t ldx, const int32_t* cu_lens, int B, int64_t T, int E, int heads, int n_cls,
                                      const float* U, const void* d_out, int64_t ldg, void* dx, int64_t lddx, float* dU,
                                      void* workspace, int64_t ws_bytes, int dtype_f32, void* stream) {
    const int rc = pool_check_geometry(B, T, E, heads, n_cls);
    if (rc != ESME_OK) return rc;
    const int d = E / heads, J = n_cls * heads;
    const int64_t n = (int64_t)J * E;
    const dim3 rgrid((unsigned int)((n + 63) / 64));
    ESME_CHECK_ARG(dU, "attn_pool_bwd: null pointer");
    if (B == 0) {                                  // no sequence: dU = 0
        hipLaunchKernelGGL(attn_pool_bwd_reduce_kernel, rgrid, dim3(64), 0, (hipStream_t)stream, (const int32_t*)nullptr,
                           (const float*)nullptr, (int64_t)0, n, dU);
        return check_launch("attn_pool_bwd");
    }
    ESME_CHECK_ARG(x && cu_lens && U && d_out && workspace, "attn_pool_bwd: null pointer");
    ESME_CHECK_ARG(ldx >= E && ldg >= (int64_t)n_cls * E && (!dx || lddx >= E), "attn_pool_bwd: bad stride");
    const int vec = dtype_f32 ? 4 : 8;
    ESME_CHECK_ARG(ldx % vec == 0 && aligned16(x) && aligned16(U) && aligned16(workspace) && (!dx || (lddx % vec == 0 && aligned16(dx))),
                   "attn_pool_bwd: misaligned x, U, dx or workspace");
    const int64_t need = esme_hip_attn_pool_bwd_workspace_bytes(B, T, E, heads, n_cls);
    ESME_CHECK_ARG(ws_bytes >= need, "attn_pool_bwd: workspace too small (see esme_hip_attn_pool_bwd_workspace_bytes)");
    const int64_t n_slots = pool_slots(B, T);
    if (n_slots > 0x7fffffffLL) ESME_FAIL(ESME_ERR_UNSUPPORTED, "attn_pool_bwd: too many chunks");
    int32_t* ws_meta = (int32_t*)workspace;
    float* ws_st = (float*)workspace + n_slots * 2;
    float* ws_sig = ws_st + n_slots * J * 3;
    float* ws_dp = ws_sig + n_slots * kPoolRows * J;
    float* ws_part = ws_dp + n_slots * kPoolRows * J;
    const dim3 cgrid((unsigned int)n_slots), ggrid((unsigned int)n_slots, (unsigned int)((E + 255) / 256));
    const hipStream_t st = (hipStream_t)stream;
    dispatch_flags([&](auto f32, auto want_dx) {
        hipLaunchKernelGGL((attn_pool_bwd_chunk_kernel<decltype(f32)::value>), cgrid, dim3(256), 0, st, x, ldx, cu_lens, B, E, heads, d, J,
                           U, d_out, ldg, ws_meta, ws_st, ws_sig, ws_dp);
        hipLaunchKernelGGL((attn_pool_bwd_grad_kernel<decltype(f32)::value, decltype(want_dx)::value>), ggrid, dim3(256), 0, st, x, ldx,
                           cu_lens, E, heads, d, J, U, d_out, ldg, (const int32_t*)ws_meta, (const float*)ws_st, (const float*)ws_sig,
                           (const float*)ws_dp, ws_part, n_slots, dx, lddx);
        return ESME_OK;
    }, dtype_f32 != 0, dx != nullptr);
    hipLaunchKernelGGL(attn_pool_bwd_reduce_kernel, rgrid, dim3(64), 0, st, (const int32_t*)ws_meta, (const float*)ws_part, n_slots, n, dU);
    return check_launch("attn_pool_bwd");
}
