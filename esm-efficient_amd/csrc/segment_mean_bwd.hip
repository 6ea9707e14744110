// Backward of the per-sequence mean (include/esme_hip_segment_mean_bwd.h): dX[t] = dY[s(t)] / len_s, zero rows outside the sequences.
//
// The kernel writes T x E and reads B x E (L2-resident: 256 KB at B = 100, E = 1280), so it is a streaming store, split by ROWS of
// dX, not by sequences: a workgroup owns kSmbRows consecutive rows whatever the sequences' lengths are, so the load is even for one
// long protein among many short ones, and B is no grid dimension.
//  - the first kSmbRows threads bisect cu_lens for one row each: s = (the first index whose offset exceeds the row) - 1, which
//    skips empty sequences (equal offsets) and gives -1 before cu_lens[0] and B from cu_lens[B] on; the row's sequence and its
//    length go to LDS;
//  - then the workgroup's rows are one flat list of 16-byte pieces, numbered row-major: consecutive lanes store consecutive pieces,
//    E / 8 need not divide the wave, and no lane idles except at the tile's end.
// Every piece of the rows [0, T) is stored exactly once (zeros where the row has no sequence): nothing is initialised by the caller.
// (Issuing eight pieces' loads of dY ahead of their stores changed nothing: 55 us against 53 us at T = 50 000, E = 1280 -- the
// stores bound the kernel, not the L2 hits in front of them.)
#include "common.h"
#include "launch.h"
#include "../../include/esme_hip_segment_mean_bwd.h"

namespace esme {

static constexpr int kSmbRows = ESME_HIP_SEGMENT_MEAN_BWD_ROWS;
static constexpr int kSmbThreads = 256;

template <bool F32>
__global__ __launch_bounds__(kSmbThreads) void segment_mean_bwd_kernel(const void* __restrict__ dyv, int64_t ld_dy, const int32_t* __restrict__ cu,
                                                                       int B, void* __restrict__ dxv, int64_t ld_dx, int64_t T, int E) {
    __shared__ int seg[kSmbRows];
    __shared__ float len[kSmbRows];
    constexpr int kVec = F32 ? 4 : 8;                                   // elements per 16-byte piece
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kSmbRows;
    const int nrows = T - r0 < kSmbRows ? (int)(T - r0) : kSmbRows;
    if (tid < nrows) {
        const int64_t r = r0 + tid;
        int s = -1, n = 0;
        if (B > 0) {
            int lo = 0, hi = B + 1;                                      // the first index of cu[0 .. B] whose offset is > r
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if ((int64_t)cu[mid] <= r) lo = mid + 1; else hi = mid;
            }
            s = lo - 1;
            if (s >= 0 && s < B) n = cu[s + 1] - cu[s];
        }
        seg[tid] = n > 0 ? s : -1;
        len[tid] = (float)n;
    }
    __syncthreads();
    const int P = E / kVec;
    const int items = nrows * P;
#pragma unroll 4
    for (int i = tid; i < items; i += kSmbThreads) {
        const int row = i / P;
        const int col = (i - row * P) * kVec;
        const int s = seg[row];
        u32x4 out = {0u, 0u, 0u, 0u};
        if (s >= 0) {
            const float l = len[row];
            if (F32) {
                f32x4 v = *reinterpret_cast<const f32x4*>((const float*)dyv + (int64_t)s * ld_dy + col);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = v[j] / l;             // [div] IEEE fp32
                out = __builtin_bit_cast(u32x4, v);
            } else {
                float f[8];
                unpack8(*reinterpret_cast<const u32x4*>((const u16*)dyv + (int64_t)s * ld_dy + col), f);
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = f[j] / l;             // [div] IEEE fp32
                out = pack8(f);                                          // [round] once, to nearest even
            }
        }
        if (F32) *reinterpret_cast<u32x4*>((float*)dxv + (r0 + row) * ld_dx + col) = out;
        else *reinterpret_cast<u32x4*>((u16*)dxv + (r0 + row) * ld_dx + col) = out;
    }
}

}  // namespace esme

using namespace esme;

extern "C" int esme_hip_segment_mean_bwd(const void* d_y, int64_t ld_dy, const int32_t* cu_lens, int B, int64_t T, int E,
                                         void* d_x, int64_t ld_dx, int dtype_f32, void* stream) {
    ESME_CHECK_ARG(B >= 0 && T >= 0 && E > 0, "segment_mean_bwd: bad sizes");
    if (E % 8 != 0) ESME_FAIL(ESME_ERR_UNSUPPORTED, "segment_mean_bwd: E % 8 != 0");
    if (T >= 0x80000000LL) ESME_FAIL(ESME_ERR_UNSUPPORTED, "segment_mean_bwd: T >= 2^31");
    if (T == 0) return ESME_OK;
    const int vec = dtype_f32 ? 4 : 8;
    ESME_CHECK_ARG(d_x && aligned16(d_x) && ld_dx >= E && ld_dx % vec == 0, "segment_mean_bwd: d_x null, misaligned or bad row stride");
    if (B > 0) {
        ESME_CHECK_ARG(d_y && cu_lens, "segment_mean_bwd: null pointer");
        ESME_CHECK_ARG(aligned16(d_y) && ld_dy >= E && ld_dy % vec == 0, "segment_mean_bwd: d_y misaligned or bad row stride");
    }
    const dim3 grid((unsigned int)((T + kSmbRows - 1) / kSmbRows));
    if (dtype_f32)
        hipLaunchKernelGGL(segment_mean_bwd_kernel<true>, grid, dim3(kSmbThreads), 0, (hipStream_t)stream, d_y, ld_dy, cu_lens, B, d_x, ld_dx, T, E);
    else
        hipLaunchKernelGGL(segment_mean_bwd_kernel<false>, grid, dim3(kSmbThreads), 0, (hipStream_t)stream, d_y, ld_dy, cu_lens, B, d_x, ld_dx, T, E);
    return check_launch("segment_mean_bwd");
}
