// Transposing expansion of the 4-bit / int8 weight formats (include/esme_hip_dequant_t.h): out (K, N) bf16 = W^T from the codes of W (N, K).
// Byte-streaming work with an LDS transposition between a coalesced read and a coalesced write.  One workgroup of 256 threads owns a
// tile of kTN = 128 weight rows (n) x kTK = 64 columns (k):
//   read    1024 code words (4 bytes for 4-bit, 8 for int8; 8 elements each), lanes along k as in quant.hip: word i of the tile is
//           (row i / 8, chunk i % 8), so a wave reads 8 rows x 8 chunks per instruction; decoded and rounded exactly as the plain kernels
//           do (the same fp32 expression, pack8), with the 16-entry codebook in LDS;
//   LDS     tile[k][n]: 64 rows of 128 bf16 = 256 bytes, i.e. one row is exactly the 64 banks of 4 bytes once.  A pitch padded by a multiple
//           of 16 bytes (which the 16-byte row reads need) leaves 8 * pitch bytes = 0 mod 128 between the rows of chunks c and c + 1, so
//           padding cannot separate the 8 chunks of a transposed write; instead the 16-byte slot (8 consecutive n) at which row k keeps
//           its data is XOR-swizzled with the chunk of k:  physical slot = (n / 8) ^ ((k / 8) & 7).
//   write   transposed, 2 bytes per element: for element j of the words, the lanes of a wave hold rows k = 8 c + j (c = 0..7) and 8
//           consecutive n of one slot s.  ds_write_b16 is serviced in two groups of 32 lanes (n offsets 0..3 / 4..7) over 32 banks of 4 bytes:
//           bank = 4 ((s ^ c) & 7) + (n & 7) / 2, so a group's 8 chunks take 8 distinct sets of 2 banks and the two lanes that share a
//           dword write its two halves (one address): conflict degree 1.  (Counted as two accesses to one bank it would be 2-way, which a
//           4-byte-class store hides behind its operand transfer.)
//   read    rows of 16 bytes (ds_read_b128, 64 banks of 4 bytes, serviced in groups of 16 lanes): lane l of a wave reads physical slot
//           l & 15 of row l / 16.  Each of the hardware's lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (and the same + 32) holds 16
//           distinct physical slots = all 64 banks once: conflict degree 1, whatever the swizzle; the swizzle only decides which 16 bytes of
//           the row's 256 the lane then stores.
//   store   16 bytes per lane; a wave writes 4 output rows x 256 contiguous bytes.  Tails (N not a multiple of 128, int8: K not of 64) are
//           handled under index checks: rows / chunks outside are neither read nor written, a slot that crosses N is stored element-wise.
// No atomics; the grid is a function of the shape alone (capped, then strided), so nothing depends on the CU count.
#include "common.h"
#include "launch.h"

#include "../../include/esme_hip_dequant_t.h"

namespace esme {

struct CodebookT { float v[16]; };

static constexpr int kTN = 128, kTK = 64;

template <bool INT8>
__global__ __launch_bounds__(256) void dequantize_t_kernel(const void* __restrict__ codes_, const float* __restrict__ absmax, int64_t N,
                                                           int K, CodebookT cb, u16* __restrict__ out, int64_t ldo, int nkt,
                                                           int64_t tiles) {
    __shared__ float lut[16];
    __shared__ __attribute__((aligned(16))) u16 tile[kTK * kTN];
    const int tid = threadIdx.x;
    if (!INT8 && tid < 16) lut[tid] = cb.v[tid];
    const int cpr = K >> 3;                                      // 8-element chunks per weight row
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t n0 = (t / nkt) * kTN;
        const int k0 = (int)(t % nkt) * kTK;
        __syncthreads();                                         // lut visible; the previous tile's reads are done
        u32x2 word[4];
        float a[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int i = it * 256 + tid, r = i >> 3, c = i & 7;
            const int64_t n = n0 + r;
            const int k = k0 + c * 8;
            const bool valid = n < N && k < K;
            word[it] = u32x2{0u, 0u};
            a[it] = 0.f;
            if (valid) {
                if constexpr (INT8) {
                    word[it] = static_cast<const u32x2*>(codes_)[n * cpr + (k >> 3)];
                    a[it] = absmax[n];
                } else {
                    word[it][0] = static_cast<const unsigned int*>(codes_)[n * cpr + (k >> 3)];   // byte j -> elements 2j, 2j+1
                    a[it] = absmax[n * (K >> 6) + (k >> 6)];
                }
            }
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int i = it * 256 + tid, r = i >> 3, c = i & 7;
            float f[8];
            if constexpr (INT8) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int code = (int)(signed char)((j < 4 ? word[it][0] >> (8 * j) : word[it][1] >> (8 * (j - 4))) & 0xffu);
                    f[j] = ((float)code * a[it]) / 127.0f;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned int byte = (word[it][0] >> (8 * j)) & 0xffu;
                    f[2 * j] = lut[byte >> 4] * a[it];
                    f[2 * j + 1] = lut[byte & 15u] * a[it];
                }
            }
            const u32x4 p = pack8(f);
            u16* col = tile + ((((r >> 3) ^ c) << 3) | (r & 7));   // row 8 c + j, physical slot (r / 8) ^ c
#pragma unroll
            for (int j = 0; j < 8; ++j) col[(c * 8 + j) * kTN] = (u16)((p[j >> 1] >> (16 * (j & 1))) & 0xffffu);
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int kr = it * 16 + (tid >> 4), ps = tid & 15;
            const u32x4 v = *reinterpret_cast<const u32x4*>(tile + kr * kTN + ps * 8);
            const int k = k0 + kr;
            const int64_t n = n0 + ((ps ^ ((kr >> 3) & 7)) << 3);
            if (k >= K || n >= N) continue;
            u16* dst = out + (int64_t)k * ldo + n;
            if (n + 8 <= N) {
                *reinterpret_cast<u32x4*>(dst) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (n + e < N) dst[e] = (u16)((v[e >> 1] >> (16 * (e & 1))) & 0xffffu);
            }
        }
    }
}

}  // namespace esme

using namespace esme;

template <bool INT8>
static int launch_t(const void* codes, const float* absmax, int64_t N, int K, const CodebookT& cb, void* out, int64_t ldo, void* stream,
                    const char* what) {
    const int nkt = (K + kTK - 1) / kTK;
    const int64_t tiles = ((N + kTN - 1) / kTN) * nkt;
    const unsigned int grid = (unsigned int)(tiles > 256 * 32 ? 256 * 32 : tiles);
    hipLaunchKernelGGL(dequantize_t_kernel<INT8>, dim3(grid), dim3(256), 0, (hipStream_t)stream, codes, absmax, N, K, cb, (u16*)out, ldo,
                       nkt, tiles);
    return check_launch(what);
}

extern "C" int esme_hip_dequantize_4bit_t(const void* codes, const float* absmax, int64_t N, int K, const float* codebook, void* out,
                                          int64_t ldo, void* stream) {
    ESME_CHECK_ARG(N >= 0 && K > 0, "dequantize_4bit_t: bad sizes");
    if (K % 64 != 0) ESME_FAIL(ESME_ERR_UNSUPPORTED, "dequantize_4bit_t: K must be a multiple of the block size 64");
    ESME_CHECK_ARG(codebook != nullptr, "dequantize_4bit_t: codebook must be 16 host floats in [-1, 1]");
    CodebookT cb;
    for (int i = 0; i < 16; ++i) {
        cb.v[i] = codebook[i];
        ESME_CHECK_ARG(cb.v[i] >= -1.f && cb.v[i] <= 1.f, "dequantize_4bit_t: codebook must be 16 host floats in [-1, 1]");
    }
    if (N == 0) return ESME_OK;
    ESME_CHECK_ARG(codes && absmax && out && ldo >= N, "dequantize_4bit_t: null pointer or bad stride");
    ESME_CHECK_ARG(aligned16(out) && ldo % 8 == 0 && (reinterpret_cast<uintptr_t>(codes) & 3u) == 0,
                   "dequantize_4bit_t: misaligned pointer or stride");
    return launch_t<false>(codes, absmax, N, K, cb, out, ldo, stream, "dequantize_4bit_t");
}

extern "C" int esme_hip_dequantize_8bit_t(const void* codes, const float* scale, int64_t N, int K, void* out, int64_t ldo, void* stream) {
    ESME_CHECK_ARG(N >= 0 && K > 0, "dequantize_8bit_t: bad sizes");
    if (K % 8 != 0) ESME_FAIL(ESME_ERR_UNSUPPORTED, "dequantize_8bit_t: K must be a multiple of 8");
    if (N == 0) return ESME_OK;
    ESME_CHECK_ARG(codes && scale && out && ldo >= N, "dequantize_8bit_t: null pointer or bad stride");
    ESME_CHECK_ARG(aligned16(out) && ldo % 8 == 0 && (reinterpret_cast<uintptr_t>(codes) & 7u) == 0,
                   "dequantize_8bit_t: misaligned pointer or stride");
    return launch_t<true>(codes, scale, N, K, CodebookT{}, out, ldo, stream, "dequantize_8bit_t");
}
