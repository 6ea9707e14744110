// Host-side argument validation of esme_hip_contact_features under AddressSanitizer, as a stand-alone program (tools/contact_features_asan.sh):
// built from csrc/contacts.hip and csrc/api.hip with -fsanitize=address on the host half, it calls the entry with bad arguments, the no-op
// sizes and the size query.  Every call here returns before any launch, so the program needs no GPU; it exits 0 when every return code
// and message is the documented one, and AddressSanitizer aborts it on a host-side memory error.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "esme_hip_contact_features.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAILED line %d: %s   (last error: %s)\n", __LINE__, #cond, esme_hip_last_error()); } } while (0)

struct Args {
    const void* q; const void* k; int64_t ld; const int32_t* cu; int B; int64_t T; int H; int d; int max_len; float scale; int qp; int f; int e;
    const int32_t* pairs; int64_t P; float* feat; int64_t ldf; int col0; void* ws; int64_t nb;
};
static int call(const Args& a) {
    return esme_hip_contact_features(a.q, a.k, a.ld, a.cu, a.B, a.T, a.H, a.d, a.max_len, a.scale, a.qp, a.f, a.e, a.pairs, a.P, a.feat, a.ldf, a.col0,
                                     a.ws, a.nb, nullptr);
}

int main() {
    std::vector<char> heap(4096 + 16);                          // host memory standing in for device pointers: never dereferenced
    char* p = (char*)(((uintptr_t)heap.data() + 15) / 16 * 16);
    const Args ok{p, p, 64, (const int32_t*)p, 1, 8, 2, 32, 8, 0.1f, 0, 1, 1, (const int32_t*)p, 4, (float*)p, 6, 4, p, 1 << 20};
    Args a;
    EXPECT(esme_hip_contact_features_workspace_bytes(7, 1000, 20) == (3 * 20 * 1000 + 20 * 7) * 4);
    EXPECT(esme_hip_contact_features_workspace_bytes(0, 0, 1) == 0);
    EXPECT(esme_hip_contact_features_workspace_bytes(1, 10, 0) == ESME_ERR_ARG && std::strstr(esme_hip_last_error(), "bad sizes"));
    EXPECT(esme_hip_contact_features_workspace_bytes(-1, 10, 2) == ESME_ERR_ARG);
    a = ok; a.d = 48; a.H = 1;      EXPECT(call(a) == ESME_ERR_UNSUPPORTED && std::strstr(esme_hip_last_error(), "head dim"));
    a = ok; a.ld = 60;              EXPECT(call(a) == ESME_ERR_ARG && std::strstr(esme_hip_last_error(), "row stride"));
    a = ok; a.ld = 32;              EXPECT(call(a) == ESME_ERR_ARG);
    a = ok; a.q = p + 2;            EXPECT(call(a) == ESME_ERR_ARG && std::strstr(esme_hip_last_error(), "misaligned"));
    a = ok; a.feat = (float*)(p + 2);   EXPECT(call(a) == ESME_ERR_ARG);
    a = ok; a.pairs = (const int32_t*)(p + 1);   EXPECT(call(a) == ESME_ERR_ARG);
    a = ok; a.nb = 8;               EXPECT(call(a) == ESME_ERR_ARG && std::strstr(esme_hip_last_error(), "workspace too small"));
    a = ok; a.pairs = nullptr;      EXPECT(call(a) == ESME_ERR_ARG && std::strstr(esme_hip_last_error(), "null"));
    a = ok; a.feat = nullptr;       EXPECT(call(a) == ESME_ERR_ARG);
    a = ok; a.ws = nullptr;         EXPECT(call(a) == ESME_ERR_ARG);
    a = ok; a.ldf = 5;              EXPECT(call(a) == ESME_ERR_ARG && std::strstr(esme_hip_last_error(), "ld_feat"));
    a = ok; a.col0 = -1;            EXPECT(call(a) == ESME_ERR_ARG);
    a = ok; a.col0 = 0x7fffffff; a.ldf = 0x7fffffff;   EXPECT(call(a) == ESME_ERR_ARG);      // col0 + H in 64 bits
    a = ok; a.P = -1;               EXPECT(call(a) == ESME_ERR_ARG);
    a = ok; a.P = 1LL << 31;        EXPECT(call(a) == ESME_ERR_ARG && std::strstr(esme_hip_last_error(), "P < 2^31"));
    a = ok; a.H = 65536; a.ld = 65536LL * 32; a.ldf = 70000;   EXPECT(call(a) == ESME_ERR_ARG);
    a = ok; a.T = 1LL << 31;        EXPECT(call(a) == ESME_ERR_ARG);
    a = ok; a.f = -1;               EXPECT(call(a) == ESME_ERR_ARG);
    a = ok; a.max_len = 0;          EXPECT(call(a) == ESME_ERR_ARG);
    a = ok; a.max_len = 1 << 27;    EXPECT(call(a) == ESME_ERR_UNSUPPORTED && std::strstr(esme_hip_last_error(), "ESME_HIP_CONTACT_MAX_SEQ_ELEMS"));
    a = ok; a.B = 0;                EXPECT(call(a) == ESME_OK);
    a = ok; a.T = 0;                EXPECT(call(a) == ESME_OK);
    a = ok; a.P = 0; a.pairs = nullptr; a.feat = nullptr;   EXPECT(call(a) == ESME_OK);
    std::printf(failures ? "%d checks failed\n" : "contact_features host checks: all passed\n", failures);
    return failures ? 1 : 0;
}
