// 64 x 64 score tiles on v_mfma_f32_16x16x32_bf16, shared by the kernels that sweep them (contacts.hip, attn_maps.hip, attn_bwd.hip),
// the softmax statistics pass of the first two, and the host checks of their shared (q, k) operand arguments.
// A wave owns 16 rows of its tile (fragments straight from global memory, 16 bytes per lane) against the 64 rows of the streamed
// tile, which the workgroup stages in LDS once (row pitch D + 8 elements: the 16-byte fragment reads of 16 consecutive rows fall on
// distinct bank groups).  In the accumulator of one MFMA lane (c = lane & 15, g = lane >> 4) holds rows 4 g + 0..3 of column c.
#pragma once
#include "common.h"
#include "launch.h"
#include "../../include/esme_hip_contacts.h"

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

// The statistics pass of contacts.hip and attn_maps.hip: query row `own` of one head's (S, D) operand q against all S keys of k, twice.
// Sweep 1 leaves the exact row maximum m of the scores in log2 units (score * cs), sweep 2 the row sum l of exp2(score * cs - m) and,
// with TRIM, the same sum lt over the kept keys f <= key < S - e only.  Each is reduced over the 16 lanes of its accumulator row: every
// lane ends with the statistics of rows 4 g + 0..3 of its wave's 16.  `tile`: the workgroup's kCT x TileDims<D>::LD staging buffer.
struct RowStats { float m[4], l[4], lt[4]; };

template <int D, bool TRIM>
__device__ __forceinline__ RowStats softmax_row_stats(u16* tile, const u16* qb, const u16* kb, unsigned int ld, int own, int S, float cs,
                                                      int f, int e, int c, int g) {
    constexpr int DS = TileDims<D>::DS;
    bf16x8 af[DS];
#pragma unroll
    for (int ks = 0; ks < DS; ++ks) af[ks] = global_frag<D>(qb, ld, own, ks, g);

    f32x4 s[4];
    RowStats st{{-INFINITY, -INFINITY, -INFINITY, -INFINITY}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int kt = 0; kt < S; kt += kCT) {
        __syncthreads();
        stage_tile<D>(tile, kb, ld, kt, S);
        __syncthreads();
        score_tile<D>(af, tile, c, g, s);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            if (kt + cb * 16 + c < S) {
#pragma unroll
                for (int r = 0; r < 4; ++r) st.m[r] = fmaxf(st.m[r], s[cb][r] * cs);                  // [score-scale]
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) st.m[r] = row16_max(st.m[r]);

    for (int kt = 0; kt < S; kt += kCT) {
        __syncthreads();
        stage_tile<D>(tile, kb, ld, kt, S);
        __syncthreads();
        score_tile<D>(af, tile, c, g, s);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const int key = kt + cb * 16 + c;
            const bool kept = TRIM && key >= f && key < S - e;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = key < S ? exp2f(s[cb][r] * cs - st.m[r]) : 0.f;                       // [exp]
                st.l[r] += p;                                                                         // [row-sum]
                if constexpr (TRIM) st.lt[r] += kept ? p : 0.f;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        st.l[r] = row16_sum(st.l[r]);
        if constexpr (TRIM) st.lt[r] = row16_sum(st.lt[r]);
    }
    return st;
}

// ------------------------------------------------------------------ host: the (q, k) operand arguments of the three entries

// What an entry adds to the shared checks, evaluated by the entry: each joins the shared check of its kind, so the first failing check
// and its message are those of the entry's own list.
struct QKEntryChecks {
    bool ptrs;                  // its other pointers are non-null
    const char* stride_err;     // nullptr, or the whole message of a failed stride check of its own (it follows the q / k row stride)
    bool aligned;               // its other pointers are aligned
    bool limits;                // its other size limits hold
    const char* limits_msg;     // the whole message of the limits check: "<entry>: max_len must be > 0, H <= 65535, ..."
};

// Null pointers, row stride, alignment, size limits, head dim and ESME_HIP_CONTACT_MAX_SEQ_ELEMS of esme_hip_contact_layer,
// esme_hip_contact_features and esme_hip_attn_maps, in that order, messages prefixed with `entry`.  ESME_OK: *cs is the factor that
// takes a score to log2 units (1 with a prescaled q).
inline int check_qk_operands(const char* entry, const void* q, const void* k, int64_t ld_qk, const int32_t* cu_lens, int64_t T, int H, int d,
                             int max_len, float softmax_scale, int q_prescaled, const void* workspace, const QKEntryChecks& x, float* cs) {
    const auto refuse = [&](int code, const char* what) {
        snprintf(error_buffer(), kErrorBufferSize, "%s: %s", entry, what);
        return code;
    };
    if (!(q && k && cu_lens && workspace && x.ptrs)) return refuse(ESME_ERR_ARG, "null pointer");
    if (!(ld_qk % 8 == 0 && ld_qk >= (int64_t)H * d)) return refuse(ESME_ERR_ARG, "bad row stride");
    if (x.stride_err) return fail(ESME_ERR_ARG, x.stride_err);
    if (!(aligned16(q) && aligned16(k) && aligned16(workspace) && x.aligned)) return refuse(ESME_ERR_ARG, "misaligned");
    if (!(max_len > 0 && H <= 65535 && T < 0x80000000LL && x.limits)) return fail(ESME_ERR_ARG, x.limits_msg);
    if (d != 16 && d != 32 && d != 64 && d != 128) return refuse(ESME_ERR_UNSUPPORTED, "head dim must be 16, 32, 64 or 128");
    if ((int64_t)max_len * ld_qk >= ESME_HIP_CONTACT_MAX_SEQ_ELEMS)
        return refuse(ESME_ERR_UNSUPPORTED, "max_len * ld_qk passes 2^32 elements (ESME_HIP_CONTACT_MAX_SEQ_ELEMS)");
    *cs = q_prescaled ? 1.0f : softmax_scale * 1.4426950408889634f;
    return ESME_OK;
}

}  // namespace esme
