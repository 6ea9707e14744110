// Backward of the token-embedding lookup (include/esme_hip_embed_bwd.h): dE[v] = the sum of the dX rows whose id is v.
//
// 50 000 packed rows fall onto 33 table rows, so the sum is split by ROWS, not by ids:
//  - embed_bwd_chunk_kernel: a work item is (chunk of kEmbRows rows, 8 columns) and belongs to ONE lane.  The lane walks its chunk's
//    rows in ascending order, kEmbUnroll 16-byte loads of dX (and their ids) in flight at a time, and adds each row into its own fp32
//    accumulators acc[v][8] in LDS.  The accumulators are addressed by the id, which is why they live in LDS: a register array indexed
//    at run time goes to scratch.  A lane never touches another lane's accumulators, so the kernel has no barrier and no atomic.
//    LDS layout acc[v][half][lane] of float4: a wave's 16-byte accesses to one (v, half) are consecutive, i.e. free of bank conflicts
//    whenever the lanes of a wave hold the same id (they do unless the wave straddles two chunks).
//    Work items are numbered chunk-major, so the lanes of a wave read consecutive 16-byte pieces of one dX row, and E / 8 need not
//    divide the wave: no lane idles except in the last workgroup.
//  - embed_bwd_reduce_kernel: one thread per (v, column): the chunks' partials in ascending chunk order, one bf16 rounding.
// Every element of dE is written by the second kernel, every element of the partials by the first: nothing is initialised by the caller.
#include "common.h"
#include "launch.h"
#include "../../include/esme_hip_embed_bwd.h"

namespace esme {

static constexpr int kEmbRows = ESME_HIP_EMBED_BWD_ROWS;
static constexpr int kEmbUnroll = 8;        // dX rows in flight per lane (8 x 16 bytes)
static constexpr int kEmbLanes = 64;        // work items per workgroup (one wave)

__global__ __launch_bounds__(kEmbLanes) void embed_bwd_chunk_kernel(const u16* __restrict__ dx, int64_t ld, const int64_t* __restrict__ tok,
                                                                    int64_t T, int E, int V, int mask_idx, int pad_idx,
                                                                    float* __restrict__ part, int64_t n_items) {
    extern __shared__ __attribute__((aligned(16))) unsigned char emb_smem[];
    f32x4* acc = reinterpret_cast<f32x4*>(emb_smem);                 // [V][2][kEmbLanes]
    const int lane = threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * kEmbLanes + lane;
    if (w >= n_items) return;                                        // (no barrier below)
    const int cgs = E >> 3;
    const int64_t chunk = w / cgs;
    const int col = (int)(w - chunk * cgs) * 8;
    const int64_t r0 = chunk * kEmbRows;
    const int nrows = T - r0 < kEmbRows ? (int)(T - r0) : kEmbRows;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < 2 * V; ++v) acc[v * kEmbLanes + lane] = zero;
    for (int r = 0; r < nrows; r += kEmbUnroll) {
        u32x4 d[kEmbUnroll];
        int64_t id[kEmbUnroll];
#pragma unroll
        for (int i = 0; i < kEmbUnroll; ++i) {
            id[i] = -1;
            d[i] = u32x4{0u, 0u, 0u, 0u};
            if (r + i < nrows) {
                id[i] = tok[r0 + r + i];
                d[i] = *reinterpret_cast<const u32x4*>(dx + (r0 + r + i) * ld + col);
            }
        }
#pragma unroll
        for (int i = 0; i < kEmbUnroll; ++i) {                       // rows in ascending order: [acc] one fp32 add per row and column
            const int64_t v = id[i];
            if (v >= 0 && v < V && v != mask_idx && v != pad_idx) {
                float f[8];
                unpack8(d[i], f);
                f32x4* a = acc + (int)v * 2 * kEmbLanes + lane;
                f32x4 a0 = a[0], a1 = a[kEmbLanes];
#pragma unroll
                for (int j = 0; j < 4; ++j) { a0[j] += f[j]; a1[j] += f[4 + j]; }
                a[0] = a0;
                a[kEmbLanes] = a1;
            }
        }
    }
    float* out = part + (chunk * V) * (int64_t)E + col;
    for (int v = 0; v < V; ++v) {
        f32x4* o = reinterpret_cast<f32x4*>(out + (int64_t)v * E);
        o[0] = acc[(v * 2) * kEmbLanes + lane];
        o[1] = acc[(v * 2 + 1) * kEmbLanes + lane];
    }
}

// dE[idx] = the chunks' partials in chunk order, idx over (v, column).  There are only V * E threads (660 waves at 33 x 1280) and each
// walks every chunk, so the pass is bound by latency, not bytes: kEmbReduceLoads chunks' loads are in flight per thread (a chunk past
// the last enters as +0, which changes no bit of the sum).  No chunk at all (T == 0): zeros.
static constexpr int kEmbReduceLoads = 32;
__global__ __launch_bounds__(64) void embed_bwd_reduce_kernel(const float* __restrict__ part, int64_t n_chunks, int64_t n, u16* __restrict__ de) {
    const int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (idx >= n) return;
    float v = 0.f;
    for (int64_t c0 = 0; c0 < n_chunks; c0 += kEmbReduceLoads) {
        float p[kEmbReduceLoads];
#pragma unroll
        for (int i = 0; i < kEmbReduceLoads; ++i) p[i] = c0 + i < n_chunks ? part[(c0 + i) * n + idx] : 0.f;
#pragma unroll
        for (int i = 0; i < kEmbReduceLoads; ++i) v += p[i];         // [chunk-sum] ascending chunk order
    }
    de[idx] = f2bf(v);                                               // [round]
}

}  // namespace esme

using namespace esme;

static int embed_bwd_check_sizes(int64_t T, int E, int V) {
    ESME_CHECK_ARG(T >= 0 && E > 0 && V > 0, "embed_bwd: bad sizes");
    if (E % 8 != 0) ESME_FAIL(ESME_ERR_UNSUPPORTED, "embed_bwd: E % 8 != 0");
    if (V > ESME_HIP_EMBED_BWD_MAX_V) ESME_FAIL(ESME_ERR_UNSUPPORTED, "embed_bwd: V > 64 (the accumulators of a workgroup are V * 2 KiB of LDS)");
    if (T >= 0x80000000LL) ESME_FAIL(ESME_ERR_UNSUPPORTED, "embed_bwd: T >= 2^31");
    return ESME_OK;
}

extern "C" int64_t esme_hip_embed_bwd_workspace_bytes(int64_t T, int E, int V) {
    const int rc = embed_bwd_check_sizes(T, E, V);
    if (rc != ESME_OK) return rc;
    return (T + kEmbRows - 1) / kEmbRows * V * E * (int64_t)sizeof(float);
}

extern "C" int esme_hip_embed_bwd(const void* d_x, int64_t ld_dx, const int64_t* tokens, int64_t T, int E, int V, int mask_idx, int pad_idx,
                                  void* d_table, void* workspace, int64_t ws_bytes, void* stream) {
    const int rc = embed_bwd_check_sizes(T, E, V);
    if (rc != ESME_OK) return rc;
    ESME_CHECK_ARG(d_table && aligned16(d_table), "embed_bwd: d_table null or misaligned");
    const hipStream_t st = (hipStream_t)stream;
    const int64_t n_chunks = (T + kEmbRows - 1) / kEmbRows, n = (int64_t)V * E;
    if (T > 0) {
        ESME_CHECK_ARG(d_x && tokens && workspace, "embed_bwd: null pointer");
        ESME_CHECK_ARG(ld_dx >= E && ld_dx % 8 == 0, "embed_bwd: bad row stride (need ld_dx >= E, ld_dx % 8 == 0)");
        ESME_CHECK_ARG(aligned16(d_x) && aligned16(workspace), "embed_bwd: misaligned d_x or workspace");
        ESME_CHECK_ARG(ws_bytes >= n_chunks * n * (int64_t)sizeof(float), "embed_bwd: workspace too small (see esme_hip_embed_bwd_workspace_bytes)");
        const int smem = V * 2 * kEmbLanes * (int)sizeof(f32x4);
        if (smem >= 64 * 1024) {
            static std::atomic<unsigned long long> done{0ull};     // dynamic-LDS attribute: per (kernel, device)
            if (const int rc2 = raise_dynamic_lds(done, embed_bwd_chunk_kernel, smem, "embed_bwd")) return rc2;
        }
        const int64_t n_items = n_chunks * (E / 8);
        if ((n_items + kEmbLanes - 1) / kEmbLanes > 0x7fffffffLL) ESME_FAIL(ESME_ERR_UNSUPPORTED, "embed_bwd: grid too large");
        hipLaunchKernelGGL(embed_bwd_chunk_kernel, dim3((unsigned int)((n_items + kEmbLanes - 1) / kEmbLanes)), dim3(kEmbLanes), smem, st,
                           (const u16*)d_x, ld_dx, tokens, T, E, V, mask_idx, pad_idx, (float*)workspace, n_items);
    }
    hipLaunchKernelGGL(embed_bwd_reduce_kernel, dim3((unsigned int)((n + 63) / 64)), dim3(64), 0, st, (const float*)workspace, n_chunks, n,
                       (u16*)d_table);
    return check_launch("embed_bwd");
}
