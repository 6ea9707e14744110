// Host-side helpers shared by the C-ABI entry points: argument checks, the thread-local
// error string behind esme_hip_last_error(), the post-launch error check, and the launch
// patterns that several entry points share (dynamic-LDS opt-in, LayerNorm-width ladder,
// head-dim and flag ladders, grid-z sequence chunks).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <type_traits>

#include "../../include/esme_hip.h"

namespace esme {

char* error_buffer();                       // thread-local, defined in api.hip
static constexpr int kErrorBufferSize = 512;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int fail(int code, const char* msg) {
    snprintf(error_buffer(), kErrorBufferSize, "%s", msg);
    return code;
}

inline int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return ESME_OK;
    snprintf(error_buffer(), kErrorBufferSize, "%s: launch failed: %s", what, hipGetErrorString(e));
    return ESME_ERR_LAUNCH;
}

// Raises the dynamic-LDS limit of `kern` to `smem` bytes, once per (kernel, device ordinal): `done` is the calling launcher
// template's own static bitmask (one per kernel instantiation, bit = device ordinal mod 64), so any host thread may get here first.
template <class... A>
inline int raise_dynamic_lds(std::atomic<unsigned long long>& done, void (*kern)(A...), int smem, const char* what) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return ESME_OK;
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess) {
        snprintf(error_buffer(), kErrorBufferSize, "%s: cannot raise the dynamic LDS limit", what);
        return ESME_ERR_LAUNCH;
    }
    done.fetch_or(bit, std::memory_order_release);
    return ESME_OK;
}

// The row kernels that keep a whole row of E elements in registers are instantiated for NCH chunks of 512 elements per row:
// calls f(std::integral_constant<int, NCH>{}) with the smallest NCH of 1 / 2 / 3 / 5 / 10 that covers E.
template <class F>
inline int dispatch_row_chunks(int64_t E, const char* what, F&& f) {
    if (E <= 512) return f(std::integral_constant<int, 1>{});
    if (E <= 1024) return f(std::integral_constant<int, 2>{});
    if (E <= 1536) return f(std::integral_constant<int, 3>{});
    if (E <= 2560) return f(std::integral_constant<int, 5>{});
    if (E <= 5120) return f(std::integral_constant<int, 10>{});
    snprintf(error_buffer(), kErrorBufferSize, "%s: E > 5120 unsupported", what);
    return ESME_ERR_UNSUPPORTED;
}

// Head-dim ladder of the attention entries: calls f(std::integral_constant<int, D>{}) for the D of the caller's list Ds... that equals d;
// any other d is refused with `msg`.
template <int... Ds, class F>
inline int dispatch_head_dim(int d, const char* msg, F&& f) {
    int rc = ESME_OK;
    const bool listed = ((d == Ds && ((rc = f(std::integral_constant<int, Ds>{})), true)) || ...);
    return listed ? rc : fail(ESME_ERR_UNSUPPORTED, msg);
}

// Run-time flags to template parameters: calls f(std::bool_constant<b>{}...) for the flags given after it.
template <class F>
inline int dispatch_flags(F&& f) { return f(); }
template <class F, class... B>
inline int dispatch_flags(F&& f, bool b, B... rest) {
    return b ? dispatch_flags([&](auto... c) { return f(std::true_type{}, c...); }, rest...)
             : dispatch_flags([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

// Grid z holds at most `max_z` sequences per launch: calls f(b0, nb) for consecutive chunks of [0, B) and stops at the first
// non-zero return, which it hands back.
template <class F>
inline int for_sequence_chunks(int B, int max_z, F&& f) {
    for (int b0 = 0; b0 < B; b0 += max_z) {
        const int nb = B - b0 < max_z ? B - b0 : max_z;
        if (const int rc = f(b0, nb)) return rc;
    }
    return ESME_OK;
}

}  // namespace esme

#define ESME_FAIL(code, msg) return ::esme::fail((code), (msg))
#define ESME_CHECK_ARG(cond, msg) \
    do { if (!(cond)) return ::esme::fail(ESME_ERR_ARG, (msg)); } while (0)
