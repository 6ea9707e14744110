// Backward of the learned-position lookup (include/esme_hip_embed_positions_bwd.h): dP[p + pos_offset] = the sum over the sequences
// longer than p of their row p of dX.
//
// The fan-in of a table row is at most B (12 - 50 for 50 000 tokens of long proteins) and there are P * E / 8 >= 160 000 independent
// sums, so the sum is split by OUTPUTS, not by rows of dX: a work item is (table row, 8 columns) and belongs to ONE lane, which keeps
// its 8 fp32 sums in registers.  One launch, no workspace, no LDS, no barrier, no atomic.
//  - Work items are numbered row-major, so the lanes of a wave read consecutive 16-byte pieces of one dX row per sequence (two rows
//    where the wave straddles table rows), and E / 8 need not divide the wave: no lane idles except in the last workgroup.
//  - The lane walks b = 0 .. B-1 in ascending order, kPosUnroll sequences at a time: their offsets are wave-uniform loads (one wide
//    load per full round), their 16-byte loads of dX are all issued before the first add.  A sequence too short for the row loads
//    nothing and adds nothing.
//  - A thousand short sequences mean few table rows and a long walk for each: correct, and bound by the latency of B / kPosUnroll
//    rounds of loads, not by bytes.
// Every element of dP is written here (zeros below pos_offset, from pos_offset + max_len on and where no sequence reaches).
#include "common.h"
#include "launch.h"
#include "../../include/esme_hip_embed_positions_bwd.h"

namespace esme {

static constexpr int kPosUnroll = 8;        // sequences in flight per lane (8 x 16 bytes of dX)
static constexpr int kPosThreads = 256;     // work items per workgroup

// One round of the walk: the sequences b .. b + kPosUnroll - 1 (FULL) or b .. B - 1 (the last, ragged round).  `first` = cu[b] comes
// from the round before, and FULL reads the kPosUnroll ends cu[b + 1 .. b + kPosUnroll] with no condition between them, so they arrive
// as ONE wide wave-uniform load and the 16-byte loads of dX leave together: one memory latency per round.  Guarded one by one (the
// ragged round) every offset is a load of its own.
template <bool FULL>
__device__ __forceinline__ void pos_round(const u16* __restrict__ dx, int64_t ld, const int32_t* __restrict__ cu, int32_t& first, int b, int B,
                                          int64_t T, int64_t p, int col, float* acc) {
    int32_t c[kPosUnroll + 1];
    c[0] = first;
#pragma unroll
    for (int i = 1; i <= kPosUnroll; ++i) c[i] = (FULL || b + i <= B) ? cu[b + i] : 0;
    first = c[kPosUnroll];
    u32x4 d[kPosUnroll];
    bool ok[kPosUnroll];
#pragma unroll
    for (int i = 0; i < kPosUnroll; ++i) {
        const int64_t start = c[i], end = c[i + 1];
        const int64_t row = start + p;
        ok[i] = (FULL || b + i < B) && end - start > p && row >= 0 && row < T;
        d[i] = u32x4{0u, 0u, 0u, 0u};
        if (ok[i]) d[i] = *reinterpret_cast<const u32x4*>(dx + row * ld + col);
    }
#pragma unroll
    for (int i = 0; i < kPosUnroll; ++i) {                           // sequences in ascending order: [acc] one fp32 add per sequence and column
        if (ok[i]) {
            float f[8];
            unpack8(d[i], f);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += f[j];
        }
    }
}

__global__ __launch_bounds__(kPosThreads) void embed_positions_bwd_kernel(const u16* __restrict__ dx, int64_t ld, const int32_t* __restrict__ cu,
                                                                          int B, int64_t T, int E, int pos_offset, int max_len,
                                                                          u16* __restrict__ dp, int64_t n_items) {
    const int64_t w = (int64_t)blockIdx.x * kPosThreads + threadIdx.x;
    if (w >= n_items) return;                                        // (no barrier below)
    const int cgs = E >> 3;
    const int64_t r = w / cgs;                                       // table row
    const int col = (int)(w - r * cgs) * 8;
    const int64_t p = r - pos_offset;                                // in-sequence position
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    if (p >= 0 && p < max_len) {
        int b = 0;
        int32_t first = B > 0 ? cu[0] : 0;
        for (; b + kPosUnroll <= B; b += kPosUnroll) pos_round<true>(dx, ld, cu, first, b, B, T, p, col, acc);
        if (b < B) pos_round<false>(dx, ld, cu, first, b, B, T, p, col, acc);
    }
    *reinterpret_cast<u32x4*>(dp + r * (int64_t)E + col) = pack8(acc);   // [round] once, to nearest even
}

}  // namespace esme

using namespace esme;

extern "C" int esme_hip_embed_positions_bwd(const void* d_x, int64_t ld, const int32_t* cu_lens, int B, int64_t T, int E, int P,
                                            int pos_offset, int max_len, void* d_pos, void* stream) {
    ESME_CHECK_ARG(B >= 0 && T >= 0 && E > 0 && P > 0, "embed_positions_bwd: bad sizes (B < 0, T < 0, E <= 0 or P <= 0)");
    ESME_CHECK_ARG(pos_offset >= 0 && max_len >= 0, "embed_positions_bwd: pos_offset < 0 or max_len < 0");
    if (E % 8 != 0) ESME_FAIL(ESME_ERR_UNSUPPORTED, "embed_positions_bwd: E % 8 != 0");
    if (T >= 0x80000000LL) ESME_FAIL(ESME_ERR_UNSUPPORTED, "embed_positions_bwd: T >= 2^31");
    ESME_CHECK_ARG((int64_t)max_len + pos_offset <= P, "embed_positions_bwd: max_len + pos_offset > P (the table has no row for the last position)");
    ESME_CHECK_ARG(d_pos && aligned16(d_pos), "embed_positions_bwd: d_pos null or misaligned");
    if (B == 0 || T == 0) B = 0;                                     // nothing to sum: d_x and cu_lens are not touched
    if (B > 0) {
        ESME_CHECK_ARG(d_x && cu_lens, "embed_positions_bwd: null pointer");
        ESME_CHECK_ARG(ld >= E && ld % 8 == 0, "embed_positions_bwd: bad row stride (need ld >= E, ld % 8 == 0)");
        ESME_CHECK_ARG(aligned16(d_x), "embed_positions_bwd: misaligned d_x");
    }
    const int64_t n_items = (int64_t)P * (E / 8);
    const int64_t blocks = (n_items + kPosThreads - 1) / kPosThreads;
    if (blocks > 0x7fffffffLL) ESME_FAIL(ESME_ERR_UNSUPPORTED, "embed_positions_bwd: grid too large");
    hipLaunchKernelGGL(embed_positions_bwd_kernel, dim3((unsigned int)blocks), dim3(kPosThreads), 0, (hipStream_t)stream, (const u16*)d_x, ld,
                       cu_lens, B, T, E, pos_offset, max_len, (u16*)d_pos, n_items);
    return check_launch("embed_positions_bwd");
}
