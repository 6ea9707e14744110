// Fused AdamW with fp32 master weights over a tensor list, the global gradient norm and the fp32 gradient accumulator
// (include/esme_hip_optim.h).
//
// All three are memory-bound streams.  One workgroup of 256 lanes owns one chunk of ESME_OPTIM_CHUNK = 8192 elements of one tensor and
// finds that tensor by bisecting the table's prefix of chunk counts (uniform loads: every lane reads the same words).  Inside a chunk a
// lane owns the groups of 8 consecutive elements g with g % 256 == lane: 16 bytes of a bf16 array, 2 x 16 bytes of an fp32 array.  A full
// group of a tensor whose arrays are all 16-byte aligned moves as vectors; the ragged last group of a tensor, and every group of a tensor
// with a misaligned array (a view at an odd element offset), goes element by element under an index check.  Both forms run the same
// per-element function in the same order, so no result bit depends on an address; nothing outside [0, numel) is touched.
//  - optim_adamw_kernel: the step.  Per element 14 bytes read and 14 written for a bf16 parameter with a bf16 gradient.
//  - optim_sqnorm_kernel / optim_sqnorm_final_kernel: sum of squares, chunk partials in fp32, then one workgroup in float64; no atomics.
//  - optim_accumulate_kernel: fp32 accumulator += gradient.
#include "common.h"
#include "launch.h"
#include "../../include/esme_hip_optim.h"

#include <math.h>

namespace esme {

static constexpr int kOptThreads = 256;
static constexpr int kOptVec = 8;                                   // elements of a lane's group
static constexpr int64_t kOptChunk = ESME_OPTIM_CHUNK;
static_assert(kOptChunk % (kOptThreads * kOptVec) == 0, "a chunk is a whole number of passes");
static_assert(sizeof(esme_optim_row_t) == 64 && sizeof(esme_optim_group_t) == 32, "the table layout of esme_hip_optim.h");

struct OptTable {
    const esme_optim_row_t* rows;
    const esme_optim_group_t* groups;
    const int64_t* prefix;
};
__host__ __device__ inline OptTable opt_table(const void* t, int n, int ng) {
    const esme_optim_row_t* rows = (const esme_optim_row_t*)t;
    const esme_optim_group_t* groups = (const esme_optim_group_t*)(rows + n);
    return {rows, groups, (const int64_t*)(groups + ng)};
}

// the chunk's row: the last r with prefix[r] <= chunk (rows without elements have no chunk and are never found); -1 past the list
__device__ __forceinline__ int opt_find_row(const int64_t* __restrict__ prefix, const int n, const int64_t chunk) {
    if (n <= 0 || chunk >= prefix[n]) return -1;
    int lo = 0, hi = n;                                             // prefix[lo] <= chunk < prefix[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= chunk) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool opt_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// 8 consecutive elements of a bf16 (F32 = false) or fp32 array at a 16-byte aligned address
template <bool F32> __device__ __forceinline__ void opt_load8(const void* base, const int64_t i, float* f) {
    if constexpr (F32) {
        const f32x4 a = *reinterpret_cast<const f32x4*>((const float*)base + i), b = *reinterpret_cast<const f32x4*>((const float*)base + i + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { f[j] = a[j]; f[4 + j] = b[j]; }
    } else {
        unpack8(*reinterpret_cast<const u32x4*>((const u16*)base + i), f);
    }
}
template <bool F32> __device__ __forceinline__ float opt_load1(const void* base, const int64_t i) {
    if constexpr (F32) return ((const float*)base)[i]; else return bf2f(((const u16*)base)[i]);
}
__device__ __forceinline__ void opt_store8_f32(float* base, const int64_t i, const float* f) {
    *reinterpret_cast<f32x4*>(base + i) = f32x4{f[0], f[1], f[2], f[3]};
    *reinterpret_cast<f32x4*>(base + i + 4) = f32x4{f[4], f[5], f[6], f[7]};
}

struct OptHyper { float s, decay, b1, omb1, b2, omb2, eps, step, isbc2; };

// The arithmetic the header states, with its roundings fixed here (no contraction left to the compiler): both the vector and the
// element-wise form call this.
__device__ __forceinline__ void adamw_element(const float gf, float& w, float& m, float& v, const OptHyper& h) {
#pragma clang fp contract(off)
    const float g = gf * h.s;
    m = fmaf(h.b1, m, h.omb1 * g);
    v = fmaf(h.b2, v, (h.omb2 * g) * g);
    const float d = fmaf(sqrtf(v), h.isbc2, h.eps);
    w = fmaf(-h.step, m / d, w * h.decay);
}

template <bool PF32, bool GF32>
__device__ __forceinline__ void adamw_chunk(const esme_optim_row_t& row, const OptHyper& h, const int64_t e0, const int64_t e1) {
    float* const wp = PF32 ? (float*)row.param : (float*)row.master;      // the fp32 weights that are stepped
    u16* const pp = (u16*)row.param;                                       // (bf16 parameters only)
    float* const mp = (float*)row.exp_avg;
    float* const vp = (float*)row.exp_avg_sq;
    const bool vec = opt_aligned16(wp) && opt_aligned16(row.grad) && opt_aligned16(mp) && opt_aligned16(vp) && (PF32 || opt_aligned16(pp));   // (uniform)
    for (int64_t i = e0 + (int64_t)threadIdx.x * kOptVec; i < e1; i += kOptThreads * kOptVec) {
        if (vec && i + kOptVec <= e1) {
            float g[8], w[8], m[8], v[8];
            opt_load8<GF32>(row.grad, i, g);
            opt_load8<true>(wp, i, w);
            opt_load8<true>(mp, i, m);
            opt_load8<true>(vp, i, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) adamw_element(g[j], w[j], m[j], v[j], h);
            opt_store8_f32(wp, i, w);
            opt_store8_f32(mp, i, m);
            opt_store8_f32(vp, i, v);
            if constexpr (!PF32) *reinterpret_cast<u32x4*>(pp + i) = pack8(w);
        } else {
            const int64_t end = i + kOptVec < e1 ? i + kOptVec : e1;
            for (int64_t k = i; k < end; ++k) {
                float w = wp[k], m = mp[k], v = vp[k];
                adamw_element(opt_load1<GF32>(row.grad, k), w, m, v, h);
                wp[k] = w;
                mp[k] = m;
                vp[k] = v;
                if constexpr (!PF32) pp[k] = f2bf(w);
            }
        }
    }
}

__global__ __launch_bounds__(kOptThreads) void optim_adamw_kernel(const void* __restrict__ table, int n, int ng, const float* __restrict__ scale) {
    const OptTable t = opt_table(table, n, ng);
    const int64_t chunk = blockIdx.x;
    const int r = opt_find_row(t.prefix, n, chunk);
    if (r < 0) return;
    const esme_optim_row_t row = t.rows[r];
    const esme_optim_group_t grp = t.groups[row.group];
    const OptHyper h = {*scale, grp.decay, grp.beta1, grp.one_minus_beta1, grp.beta2, grp.one_minus_beta2, grp.eps, row.step_size, row.inv_sqrt_bc2};
    const int64_t e0 = (chunk - t.prefix[r]) * kOptChunk;
    const int64_t e1 = e0 + kOptChunk < row.numel ? e0 + kOptChunk : row.numel;
    const bool pf32 = row.flags & ESME_OPTIM_PARAM_F32, gf32 = row.flags & ESME_OPTIM_GRAD_F32;     // (uniform)
    if (pf32) { if (gf32) adamw_chunk<true, true>(row, h, e0, e1); else adamw_chunk<true, false>(row, h, e0, e1); }
    else      { if (gf32) adamw_chunk<false, true>(row, h, e0, e1); else adamw_chunk<false, false>(row, h, e0, e1); }
}

// sum over the workgroup in a fixed order: the xor butterfly inside each wave, then the 4 waves in order; valid in thread 0
template <class T> __device__ __forceinline__ T opt_block_sum(T v, T* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

template <bool GF32>
__device__ __forceinline__ float sqnorm_chunk(const void* grad, const int64_t e0, const int64_t e1) {
    const bool vec = opt_aligned16(grad);
    float acc = 0.f;
    for (int64_t i = e0 + (int64_t)threadIdx.x * kOptVec; i < e1; i += kOptThreads * kOptVec) {
        if (vec && i + kOptVec <= e1) {
            float g[8];
            opt_load8<GF32>(grad, i, g);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = fmaf(g[j], g[j], acc);
        } else {
            const int64_t end = i + kOptVec < e1 ? i + kOptVec : e1;
            for (int64_t k = i; k < end; ++k) {
                const float g = opt_load1<GF32>(grad, k);
                acc = fmaf(g, g, acc);
            }
        }
    }
    return acc;
}

__global__ __launch_bounds__(kOptThreads) void optim_sqnorm_kernel(const void* __restrict__ table, int n, int ng, float* __restrict__ partial) {
    __shared__ float lds[4];
    const OptTable t = opt_table(table, n, ng);
    const int64_t chunk = blockIdx.x;
    const int r = opt_find_row(t.prefix, n, chunk);
    if (r < 0) return;                                              // (block-uniform)
    const esme_optim_row_t row = t.rows[r];
    const int64_t e0 = (chunk - t.prefix[r]) * kOptChunk;
    const int64_t e1 = e0 + kOptChunk < row.numel ? e0 + kOptChunk : row.numel;
    const float acc = (row.flags & ESME_OPTIM_GRAD_F32) ? sqnorm_chunk<true>(row.grad, e0, e1) : sqnorm_chunk<false>(row.grad, e0, e1);
    const float s = opt_block_sum<float>(acc, lds);
    if (threadIdx.x == 0) partial[chunk] = s;
}

__global__ __launch_bounds__(kOptThreads) void optim_sqnorm_final_kernel(const float* __restrict__ partial, int64_t chunks, float max_norm, float grad_scale,
                                                                         float* __restrict__ out) {
    __shared__ double lds[4];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < chunks; i += kOptThreads) acc += (double)partial[i];
    const double total = opt_block_sum<double>(acc, lds);
    if (threadIdx.x == 0) {
        const float norm = (float)(sqrt(total) * (double)grad_scale);
        float coef = 1.f;
        if (max_norm > 0.f) {
            coef = max_norm / (norm + 1e-6f);
            if (coef > 1.f) coef = 1.f;                             // (a NaN stays a NaN)
        }
        out[0] = norm;
        out[1] = coef;
        out[2] = coef * grad_scale;
    }
}

template <bool GF32>
__device__ __forceinline__ void accumulate_chunk(const esme_optim_row_t& row, const int64_t e0, const int64_t e1) {
    float* const ap = (float*)row.master;
    const bool init = row.flags & ESME_OPTIM_ACC_INIT;
    const bool vec = opt_aligned16(ap) && opt_aligned16(row.grad);
    for (int64_t i = e0 + (int64_t)threadIdx.x * kOptVec; i < e1; i += kOptThreads * kOptVec) {
        if (vec && i + kOptVec <= e1) {
            float g[8], a[8];
            opt_load8<GF32>(row.grad, i, g);
            if (!init) {
                opt_load8<true>(ap, i, a);
#pragma unroll
                for (int j = 0; j < 8; ++j) g[j] += a[j];
            }
            opt_store8_f32(ap, i, g);
        } else {
            const int64_t end = i + kOptVec < e1 ? i + kOptVec : e1;
            for (int64_t k = i; k < end; ++k) {
                const float g = opt_load1<GF32>(row.grad, k);
                ap[k] = init ? g : g + ap[k];
            }
        }
    }
}

__global__ __launch_bounds__(kOptThreads) void optim_accumulate_kernel(const void* __restrict__ table, int n, int ng) {
    const OptTable t = opt_table(table, n, ng);
    const int64_t chunk = blockIdx.x;
    const int r = opt_find_row(t.prefix, n, chunk);
    if (r < 0) return;
    const esme_optim_row_t row = t.rows[r];
    const int64_t e0 = (chunk - t.prefix[r]) * kOptChunk;
    const int64_t e1 = e0 + kOptChunk < row.numel ? e0 + kOptChunk : row.numel;
    if (row.flags & ESME_OPTIM_GRAD_F32) accumulate_chunk<true>(row, e0, e1); else accumulate_chunk<false>(row, e0, e1);
}

enum { kUseParam = 1, kUseGrad = 2, kUseMaster = 4, kUseMoments = 8, kUseGroup = 16 };

static inline bool opt_aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// The checks of the header on the host copy of the table; *total = prefix[n_tensors].
static int optim_check_table(const char* what, const void* table_host, const void* table_dev, int n, int ng, int uses, int64_t* total) {
    char* const err = error_buffer();
    auto bad = [&](int r, const char* msg) {
        if (r >= 0) snprintf(err, kErrorBufferSize, "%s: tensor %d: %s", what, r, msg); else snprintf(err, kErrorBufferSize, "%s: %s", what, msg);
        return ESME_ERR_ARG;
    };
    if (n < 0 || ng < 0) return bad(-1, "n_tensors and n_groups must be >= 0");
    if (!table_host || !table_dev) return bad(-1, "null table");
    if (!opt_aligned_to(table_host, 8) || !opt_aligned_to(table_dev, 8)) return bad(-1, "misaligned table (8 bytes)");
    const OptTable t = opt_table(table_host, n, ng);
    if (t.prefix[0] != 0) return bad(-1, "prefix[0] must be 0");
    const int known = ESME_OPTIM_PARAM_F32 | ESME_OPTIM_GRAD_F32 | ESME_OPTIM_ACC_INIT;
    for (int r = 0; r < n; ++r) {
        const esme_optim_row_t& row = t.rows[r];
        if (row.numel < 0) return bad(r, "negative numel");
        if (row.flags & ~known) return bad(r, "unknown flag");
        if (t.prefix[r + 1] - t.prefix[r] != (row.numel + kOptChunk - 1) / kOptChunk) return bad(r, "prefix does not match numel (ceil(numel / ESME_OPTIM_CHUNK) chunks)");
        if ((uses & kUseGroup) && (row.group < 0 || row.group >= ng)) return bad(r, "group index outside the group table");
        if (row.numel == 0) continue;
        const bool pf32 = row.flags & ESME_OPTIM_PARAM_F32, gf32 = row.flags & ESME_OPTIM_GRAD_F32;
        if ((uses & kUseParam) && !row.param) return bad(r, "null param");
        if ((uses & kUseGrad) && !row.grad) return bad(r, "null grad");
        if ((uses & kUseMaster) && !row.master && !((uses & kUseParam) && pf32)) return bad(r, "null master");
        if ((uses & kUseMoments) && (!row.exp_avg || !row.exp_avg_sq)) return bad(r, "null exp_avg or exp_avg_sq");
        if ((uses & kUseParam) && !opt_aligned_to(row.param, pf32 ? 4 : 2)) return bad(r, "param is not aligned to its element");
        if ((uses & kUseGrad) && !opt_aligned_to(row.grad, gf32 ? 4 : 2)) return bad(r, "grad is not aligned to its element");
        if ((uses & kUseMaster) && !((uses & kUseParam) && pf32) && !opt_aligned_to(row.master, 4)) return bad(r, "master is not aligned to its element");
        if ((uses & kUseMoments) && (!opt_aligned_to(row.exp_avg, 4) || !opt_aligned_to(row.exp_avg_sq, 4))) return bad(r, "exp_avg or exp_avg_sq is not aligned to its element");
    }
    *total = t.prefix[n];
    if (*total >= (1LL << 31)) return bad(-1, "too many chunks (prefix[n_tensors] must be < 2^31)");
    return ESME_OK;
}

}  // namespace esme

using namespace esme;

extern "C" int esme_hip_optim_chunk_elems(void) { return ESME_OPTIM_CHUNK; }

extern "C" int64_t esme_hip_optim_table_bytes(int n_tensors, int n_groups) {
    if (n_tensors < 0 || n_groups < 0) return fail(ESME_ERR_ARG, "optim_table_bytes: n_tensors and n_groups must be >= 0");
    return (int64_t)sizeof(esme_optim_row_t) * n_tensors + (int64_t)sizeof(esme_optim_group_t) * n_groups + 8 * ((int64_t)n_tensors + 1);
}

extern "C" int64_t esme_hip_optim_workspace_bytes(int64_t total_chunks) {
    if (total_chunks < 0 || total_chunks >= (1LL << 31)) return fail(ESME_ERR_ARG, "optim_workspace_bytes: need 0 <= total_chunks < 2^31");
    return 4 * (total_chunks < 4 ? 4 : total_chunks);
}

extern "C" int esme_hip_optim_adamw_step(const void* table_host, const void* table_dev, int n_tensors, int n_groups, const void* scale, void* stream) {
    int64_t total = 0;
    const int rc = optim_check_table("optim_adamw_step", table_host, table_dev, n_tensors, n_groups, kUseParam | kUseGrad | kUseMaster | kUseMoments | kUseGroup, &total);
    if (rc != ESME_OK) return rc;
    ESME_CHECK_ARG(scale && opt_aligned_to(scale, 4), "optim_adamw_step: scale is null or misaligned (4 bytes)");
    if (total == 0) return ESME_OK;
    hipLaunchKernelGGL(optim_adamw_kernel, dim3((unsigned int)total), dim3(kOptThreads), 0, (hipStream_t)stream, table_dev, n_tensors, n_groups, (const float*)scale);
    return check_launch("optim_adamw_step");
}

extern "C" int esme_hip_optim_grad_sqnorm(const void* table_host, const void* table_dev, int n_tensors, int n_groups, float max_norm, float grad_scale,
                                          void* workspace, int64_t ws_bytes, void* out, void* stream) {
    int64_t total = 0;
    const int rc = optim_check_table("optim_grad_sqnorm", table_host, table_dev, n_tensors, n_groups, kUseGrad, &total);
    if (rc != ESME_OK) return rc;
    ESME_CHECK_ARG(out && opt_aligned_to(out, 4), "optim_grad_sqnorm: out is null or misaligned (4 bytes)");
    ESME_CHECK_ARG(workspace && opt_aligned_to(workspace, 4), "optim_grad_sqnorm: workspace is null or misaligned (4 bytes)");
    ESME_CHECK_ARG(ws_bytes >= esme_hip_optim_workspace_bytes(total), "optim_grad_sqnorm: workspace too small (see esme_hip_optim_workspace_bytes)");
    ESME_CHECK_ARG(isfinite(grad_scale) && grad_scale > 0.f && !isnan(max_norm), "optim_grad_sqnorm: grad_scale must be finite and > 0, max_norm not NaN");
    const hipStream_t st = (hipStream_t)stream;
    if (total > 0) hipLaunchKernelGGL(optim_sqnorm_kernel, dim3((unsigned int)total), dim3(kOptThreads), 0, st, table_dev, n_tensors, n_groups, (float*)workspace);
    hipLaunchKernelGGL(optim_sqnorm_final_kernel, dim3(1), dim3(kOptThreads), 0, st, (const float*)workspace, total, max_norm, grad_scale, (float*)out);
    return check_launch("optim_grad_sqnorm");
}

extern "C" int esme_hip_optim_grad_accumulate(const void* table_host, const void* table_dev, int n_tensors, int n_groups, void* stream) {
    int64_t total = 0;
    const int rc = optim_check_table("optim_grad_accumulate", table_host, table_dev, n_tensors, n_groups, kUseGrad | kUseMaster, &total);
    if (rc != ESME_OK) return rc;
    if (total == 0) return ESME_OK;
    hipLaunchKernelGGL(optim_accumulate_kernel, dim3((unsigned int)total), dim3(kOptThreads), 0, (hipStream_t)stream, table_dev, n_tensors, n_groups);
    return check_launch("optim_grad_accumulate");
}
