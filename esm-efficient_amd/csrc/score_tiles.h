// 64 x 64 score tiles on v_mfma_f32_16x16x32_bf16, shared by the kernels that sweep them (contacts.hip, attn_bwd.hip).
// A wave owns 16 rows of its tile (fragments straight from global memory, 16 bytes per lane) against the 64 rows of the streamed
// tile, which the workgroup stages in LDS once (row pitch D + 8 elements: the 16-byte fragment reads of 16 consecutive rows fall on
// distinct bank groups).  In the accumulator of one MFMA lane (c = lane & 15, g = lane >> 4) holds rows 4 g + 0..3 of column c.
#pragma once
#include "common.h"

namespace esme {

static constexpr int kCT = 64;            // tile edge: rows of a workgroup's own tile and of the streamed tile

template <int D> struct TileDims {
    static constexpr int DS = D <= 32 ? 1 : D / 32;     // MFMA k-steps (head dim 16: the upper half of the one step is zero)
    static constexpr int LD = D + 8;                    // LDS row pitch in elements
};

__device__ __forceinline__ bf16x8 zero_frag() { return __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u}); }

// operand fragment of row `row`: elements 32 ks + 8 g .. + 7 (A and B operands of the 16x16x32 MFMA share this map)
template <int D>
__device__ __forceinline__ bf16x8 global_frag(const u16* base, unsigned int ld, int row, int ks, int g) {
    if (D == 16 && g >= 2) return zero_frag();
    return *reinterpret_cast<const bf16x8*>(base + ((unsigned int)row * ld + (unsigned int)(ks * 32 + g * 8)));
}
template <int D>
__device__ __forceinline__ bf16x8 lds_frag(const u16* tile, int row, int ks, int g) {
    if (D == 16 && g >= 2) return zero_frag();
    return *reinterpret_cast<const bf16x8*>(tile + row * TileDims<D>::LD + ks * 32 + g * 8);
}

// rows row0 .. row0 + 63 of one head's (S, D) operand into LDS; rows past the sequence repeat its last row (their scores are masked)
template <int D>
__device__ __forceinline__ void stage_tile(u16* tile, const u16* base, unsigned int ld, int row0, int S) {
    constexpr int CPR = D / 8, NCH = kCT * CPR;
    for (int ch = threadIdx.x; ch < NCH; ch += 256) {
        const int row = ch / CPR, col = (ch % CPR) * 8;
        int gr = row0 + row;
        gr = gr < S ? gr : S - 1;
        *reinterpret_cast<u32x4*>(tile + row * TileDims<D>::LD + col) =
            *reinterpret_cast<const u32x4*>(base + ((unsigned int)gr * ld + (unsigned int)col));
    }
}

// s[cb][r] = (own row 4 g + r) . (tile row 16 cb + c)
template <int D>
__device__ __forceinline__ void score_tile(const bf16x8* a, const u16* tile, int c, int g, f32x4* s) {
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        s[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < TileDims<D>::DS; ++ks) s[cb] = mfma_16x16x32<false>(a[ks], lds_frag<D>(tile, cb * 16 + c, ks, g), s[cb]);
    }
}

// over the 16 lanes that hold one accumulator row (lane bits 0..3), a fixed butterfly
__device__ __forceinline__ float row16_max(float v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

}  // namespace esme
