// What the attention-pooling forward (pool.hip) and its backward (pool_bwd.hip) share: the chunk geometry, the slot numbering of
// (sequence, chunk) work items, the operand loaders and the geometry refusals.
#pragma once
#include "common.h"
#include "launch.h"

namespace esme {

static constexpr int kPoolRows = 64;      // R: rows per chunk
static constexpr int kPoolJ = 64;         // query columns (c, h) per score pass
static constexpr int kPoolK = 32;         // E columns per LDS slab
static constexpr int kPoolMaxJ = 512;     // n_cls * H limit

// First slot of sequence s: s + floor(cu[s] / R).  Strictly increasing in s, and the next sequence's first slot lies past
// this one's last chunk, so slots never collide; there are at most B + floor(T / R) + 1 of them.
__device__ __forceinline__ int64_t pool_first_slot(const int32_t* cu, int s) { return (int64_t)s + cu[s] / kPoolRows; }

template <bool F32>
__device__ __forceinline__ void load8(const void* x, int64_t off, float* f) {
    if (F32) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>((const float*)x + off);
        const f32x4 hi = *reinterpret_cast<const f32x4*>((const float*)x + off + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { f[j] = lo[j]; f[4 + j] = hi[j]; }
    } else {
        unpack8(*reinterpret_cast<const u32x4*>((const u16*)x + off), f);
    }
}

template <bool F32>
__device__ __forceinline__ float load1(const void* x, int64_t off) {
    return F32 ? ((const float*)x)[off] : bf2f(((const u16*)x)[off]);
}

}  // namespace esme

static int64_t pool_slots(int B, int64_t T) { return (int64_t)B + T / esme::kPoolRows + 1; }

static int pool_check_geometry(int B, int64_t T, int E, int heads, int n_cls) {
    ESME_CHECK_ARG(B >= 0 && T >= 0 && E > 0 && heads > 0 && n_cls > 0, "attn_pool: bad sizes");
    ESME_CHECK_ARG(E % heads == 0, "attn_pool: embed_dim is not a multiple of heads");
    ESME_CHECK_ARG(E % 8 == 0, "attn_pool: embed_dim % 8 != 0");
    if ((int64_t)n_cls * heads > esme::kPoolMaxJ) ESME_FAIL(ESME_ERR_UNSUPPORTED, "attn_pool: n_cls * heads > 512");
    return ESME_OK;
}
