// Attention-pooling task heads (reference esme/pooling.py:72-228, esme/head.py:30-68).
//
// The reference projects every residue, k = x W_k^T + b_k (a T x E x E GEMM), repeats k and v = x n_cls times and runs
// flash attention with one query per (class token, head).  The queries are fixed per call, so the projection folds into
// them:  q_{c,h} . k_t = u_{c,h} . x_t + q_{c,h} . b_k[h],  u_{c,h} = W_k[h d:(h+1) d, :]^T q_{c,h}.  The bias term is
// constant over t and cancels in the softmax, so
//     out[s, c, h d + i] = sum_{t in s} softmax_t(u_{c,h} . x_t / sqrt(d)) x_t[h d + i].
//  - attn_pool_fold_kernel:  U (J = n_cls H, E) fp32 = log2(e) / sqrt(d) * u, every call (no cache that could go stale);
//  - attn_pool_chunk_kernel: one workgroup per (sequence, chunk of kPoolRows rows): scores in fp32, the chunk's running
//    max, sum and unnormalised output per (c, h) into the workspace;
//  - attn_pool_combine_kernel: a sequence's chunks merged in chunk order, one rounding to the output dtype.
// Chunks start at each sequence's own first row and are merged in a fixed order: a sequence's result does not depend on
// its neighbours or on the run (bit-identical alone and packed).
//  - relu_linear_kernel: y = b + W relu(h), the heads' last Linear (N <= 64 outputs).
#include "pool.h"   // chunk geometry, slot numbering, loaders and geometry refusals, shared with the backward (pool_bwd.hip)

namespace esme {

// U[c H + h, e] = scale * sum_{i < d} cls[c, h d + i] W[h d + i, e]: fp32 fmaf chain in i order, then one multiply by
// scale = fp32(log2(e) / sqrt(d)).  One thread per (j, e); consecutive threads read consecutive e of a W row.
__global__ __launch_bounds__(256) void attn_pool_fold_kernel(const u16* __restrict__ cls, int64_t ldc, const u16* __restrict__ w,
                                                             int64_t ldw, int E, int H, int d, int J, float scale,
                                                             float* __restrict__ U) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)J * E) return;
    const int j = (int)(idx / E), e = (int)(idx % E);
    const int c = j / H, h = j % H;
    const u16* q = cls + (int64_t)c * ldc + (int64_t)h * d;
    const u16* wr = w + (int64_t)h * d * ldw + e;
    float acc = 0.f;
    for (int i = 0; i < d; ++i) acc = fmaf(bf2f(q[i]), bf2f(wr[(int64_t)i * ldw]), acc);
    U[idx] = acc * scale;                                                    // [fold-scale]
}

// One workgroup per slot g.  Workspace per slot: ml[J][2] = {max, sum of exp2(score - max)} and o[n_cls][E] = the
// unnormalised sum_r exp2(score_r - max) x_r over the chunk's rows.
template <bool F32>
__global__ __launch_bounds__(256) void attn_pool_chunk_kernel(const void* __restrict__ x, int64_t ldx, const int32_t* __restrict__ cu,
                                                              int B, int E, int H, int d, int J, const float* __restrict__ U,
                                                              float* __restrict__ ws_ml, float* __restrict__ ws_o) {
    __shared__ float xs[kPoolK][kPoolRows + 4];   // x slab, k-major
    __shared__ float us[kPoolK][kPoolJ + 4];      // U slab, k-major
    __shared__ float sc[kPoolRows][kPoolJ + 1];   // scores, then exp2(score - max)
    __shared__ int64_t sh_row0;
    __shared__ int sh_rows;
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
    }
    __syncthreads();
    const int nrows = sh_rows;
    if (nrows == 0) return;                        // past the sequence's last chunk (block-uniform)
    const int64_t row0 = sh_row0;
    const int n_cls = J / H;
    float* ml = ws_ml + g * (int64_t)J * 2;
    float* o = ws_o + g * (int64_t)n_cls * E;

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
                for (int k = 0; k < kn; ++k) {      // [score] fp32 fmaf chain over e in order
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
        if (t < jn) {                              // per query column: max, exp2, sum over the chunk's rows in row order
            float m = -INFINITY;
            for (int r = 0; r < nrows; ++r) m = fmaxf(m, sc[r][t]);
            float l = 0.f;
            for (int r = 0; r < nrows; ++r) {
                const float p = exp2f(sc[r][t] - m);   // [exp]
                sc[r][t] = p;
                l += p;                                 // [row-sum]
            }
            ml[(int64_t)(g0 + t) * 2] = m;
            ml[(int64_t)(g0 + t) * 2 + 1] = l;
        }
        __syncthreads();
        for (int q = t; q < jn * d; q += 256) {   // o[c, h d + i] = sum_r p[r] x[r, h d + i]
            const int jj = q / d, i = q % d;
            const int j = g0 + jj, c = j / H, col = (j % H) * d + i;
            float s = 0.f;
            for (int r = 0; r < nrows; ++r) s = fmaf(sc[r][jj], load1<F32>(x, (row0 + r) * ldx + col), s);   // [pv] row order
            o[(int64_t)c * E + col] = s;
        }
        __syncthreads();
    }
}

// out[s, c, col] = (sum_k a_k o_k) / (sum_k a_k l_k),  a_k = exp2(m_k - max_k m_k), over the sequence's chunks in order;
// one rounding to the output dtype.  Grid (B, ceil(n_cls E / 256)); an empty sequence writes zeros.
template <bool F32>
__global__ __launch_bounds__(256) void attn_pool_combine_kernel(const int32_t* __restrict__ cu, int E, int H, int d, int J,
                                                                int64_t n_slots, const float* __restrict__ ws_ml,
                                                                const float* __restrict__ ws_o, void* __restrict__ out, int64_t ldo) {
    const int s = blockIdx.x;
    const int n_cls = J / H;
    const int q = blockIdx.y * 256 + threadIdx.x;
    if (q >= n_cls * E) return;
    const int c = q / E, col = q % E;
    const int j = c * H + col / d;
    const int64_t len = (int64_t)cu[s + 1] - cu[s];
    const int64_t first = pool_first_slot(cu, s);
    int64_t nch = (len + kPoolRows - 1) / kPoolRows;
    if (first + nch > n_slots) nch = n_slots - first > 0 ? n_slots - first : 0;
    float v = 0.f;
    if (nch > 0) {
        float m = -INFINITY;
        for (int64_t k = 0; k < nch; ++k) m = fmaxf(m, ws_ml[((first + k) * J + j) * 2]);
        float l = 0.f, acc = 0.f;
        for (int64_t k = 0; k < nch; ++k) {
            const float a = exp2f(ws_ml[((first + k) * J + j) * 2] - m);                   // [combine-exp]
            l = fmaf(a, ws_ml[((first + k) * J + j) * 2 + 1], l);                           // [combine-sum]
            acc = fmaf(a, ws_o[((first + k) * n_cls + c) * (int64_t)E + col], acc);
        }
        v = acc / l;                                                                        // [divide]
    }
    const int64_t oo = (int64_t)s * ldo + (int64_t)c * E + col;
    if (F32) ((float*)out)[oo] = v;
    else ((u16*)out)[oo] = f2bf(v);                                                         // [out-round]
}

// y[r, j] = b[j] + sum_k W[j, k] relu(h[r, k]) for j < N <= 64.  One wave per row: lane l owns the k = 8 l + 512 i blocks
// (fp32 fmaf chain in i order), then a fixed butterfly across the wave; one rounding to the output dtype.
template <bool F32>
__global__ __launch_bounds__(256) void relu_linear_kernel(const void* __restrict__ h, int64_t ldh, const u16* __restrict__ w,
                                                          int64_t ldw, const u16* __restrict__ bias, void* __restrict__ y,
                                                          int64_t ldy, int64_t M, int N, int K) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;                            // wave-uniform
    for (int j0 = 0; j0 < N; j0 += 8) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = lane * 8; k < K; k += 512) {
            float f[8];
            load8<F32>(h, r * ldh + k, f);
#pragma unroll
            for (int i = 0; i < 8; ++i) f[i] = f[i] < 0.f ? 0.f : f[i];          // not fmaxf: v_max returns its non-NaN operand, relu(NaN) is NaN
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                if (j0 + jj < N) {
                    float wf[8];
                    unpack8(*reinterpret_cast<const u32x4*>(w + (int64_t)(j0 + jj) * ldw + k), wf);
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[jj] = fmaf(wf[i], f[i], acc[jj]);
                }
            }
        }
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const float s = wave_sum(acc[jj]);
            if (lane == 0 && j0 + jj < N) {
                const float v = s + (bias ? bf2f(bias[j0 + jj]) : 0.f);
                if (F32) ((float*)y)[r * ldy + j0 + jj] = v;
                else ((u16*)y)[r * ldy + j0 + jj] = f2bf(v);
            }
        }
    }
}

}  // namespace esme

using namespace esme;

extern "C" int64_t esme_hip_attn_pool_workspace_bytes(int B, int64_t T, int E, int heads, int n_cls) {
    const int rc = pool_check_geometry(B, T, E, heads, n_cls);
    if (rc != ESME_OK) return rc;
    const int64_t J = (int64_t)n_cls * heads;
    return pool_slots(B, T) * (2 * J + (int64_t)n_cls * E) * (int64_t)sizeof(float);
}

extern "C" int esme_hip_attn_pool_fold(const void* cls, int64_t ldc, const void* w_k, int64_t ldw, int E, int heads, int n_cls,
                                       float* U, void* stream) {
    const int rc = pool_check_geometry(0, 0, E, heads, n_cls);
    if (rc != ESME_OK) return rc;
    ESME_CHECK_ARG(cls && w_k && U && ldc >= E && ldw >= E, "attn_pool_fold: null pointer or bad stride");
    ESME_CHECK_ARG(aligned16(U), "attn_pool_fold: misaligned U");
    const int d = E / heads, J = n_cls * heads;
    const float scale = (float)(1.4426950408889634 / sqrt((double)d));
    const int64_t n = (int64_t)J * E;
    hipLaunchKernelGGL(attn_pool_fold_kernel, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const u16*)cls, ldc, (const u16*)w_k, ldw, E, heads, d, J, scale, U);
    return check_launch("attn_pool_fold");
}

extern "C" int esme_hip_attn_pool(const void* x, int64_t ldx, const int32_t* cu_lens, int B, int64_t T, int E, int heads,
                                  int n_cls, const float* U, void* workspace, int64_t ws_bytes, void* out, int64_t ldo,
                                  int dtype_f32, void* stream) {
    const int rc = pool_check_geometry(B, T, E, heads, n_cls);
    if (rc != ESME_OK) return rc;
    if (B == 0) return ESME_OK;
    ESME_CHECK_ARG(x && cu_lens && U && workspace && out, "attn_pool: null pointer");
    ESME_CHECK_ARG(ldx >= E && ldo >= (int64_t)n_cls * E, "attn_pool: bad stride");
    const int vec = dtype_f32 ? 4 : 8;
    ESME_CHECK_ARG(ldx % vec == 0 && aligned16(x) && aligned16(U) && aligned16(workspace), "attn_pool: misaligned x, U or workspace");
    const int64_t need = esme_hip_attn_pool_workspace_bytes(B, T, E, heads, n_cls);
    ESME_CHECK_ARG(ws_bytes >= need, "attn_pool: workspace too small (see esme_hip_attn_pool_workspace_bytes)");
    const int d = E / heads, J = n_cls * heads;
    const int64_t n_slots = pool_slots(B, T);
    if (n_slots > 0x7fffffffLL) ESME_FAIL(ESME_ERR_UNSUPPORTED, "attn_pool: too many chunks");
    float* ws_ml = (float*)workspace;
    float* ws_o = ws_ml + n_slots * J * 2;
    const unsigned int ycols = (unsigned int)(((int64_t)n_cls * E + 255) / 256);
    if (dtype_f32) {
        hipLaunchKernelGGL(attn_pool_chunk_kernel<true>, dim3((unsigned int)n_slots), dim3(256), 0, (hipStream_t)stream, x, ldx,
                           cu_lens, B, E, heads, d, J, U, ws_ml, ws_o);
        hipLaunchKernelGGL(attn_pool_combine_kernel<true>, dim3((unsigned int)B, ycols), dim3(256), 0, (hipStream_t)stream, cu_lens,
                           E, heads, d, J, n_slots, ws_ml, ws_o, out, ldo);
    } else {
        hipLaunchKernelGGL(attn_pool_chunk_kernel<false>, dim3((unsigned int)n_slots), dim3(256), 0, (hipStream_t)stream, x, ldx,
                           cu_lens, B, E, heads, d, J, U, ws_ml, ws_o);
        hipLaunchKernelGGL(attn_pool_combine_kernel<false>, dim3((unsigned int)B, ycols), dim3(256), 0, (hipStream_t)stream, cu_lens,
                           E, heads, d, J, n_slots, ws_ml, ws_o, out, ldo);
    }
    return check_launch("attn_pool");
}

extern "C" int esme_hip_relu_linear(const void* h, int64_t ldh, const void* w, int64_t ldw, const void* bias, void* y, int64_t ldy,
                                    int64_t M, int N, int K, int dtype_f32, void* stream) {
    ESME_CHECK_ARG(M >= 0 && N > 0 && K > 0, "relu_linear: bad sizes");
    if (N > 64) ESME_FAIL(ESME_ERR_UNSUPPORTED, "relu_linear: more than 64 outputs");
    if (M == 0) return ESME_OK;
    ESME_CHECK_ARG(h && w && y && ldh >= K && ldw >= K && ldy >= N, "relu_linear: null pointer or bad stride");
    ESME_CHECK_ARG(K % 8 == 0 && ldh % (dtype_f32 ? 4 : 8) == 0 && ldw % 8 == 0 && aligned16(h) && aligned16(w),
                   "relu_linear: K % 8 != 0 or misaligned rows");
    if ((M + 3) / 4 > 0x7fffffffLL) ESME_FAIL(ESME_ERR_UNSUPPORTED, "relu_linear: too many rows");
    const dim3 grid((unsigned int)((M + 3) / 4));
    if (dtype_f32)
        hipLaunchKernelGGL(relu_linear_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, h, ldh, (const u16*)w, ldw,
                           (const u16*)bias, y, ldy, M, N, K);
    else
        hipLaunchKernelGGL(relu_linear_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, h, ldh, (const u16*)w, ldw,
                           (const u16*)bias, y, ldy, M, N, K);
    return check_launch("relu_linear");
}
