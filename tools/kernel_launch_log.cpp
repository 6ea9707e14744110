// Launch log of the GEMM and attention launchers (csrc/gemm.hip, csrc/attn.hip), on the CPU.
//
// Which kernel instantiation a call runs, on which grid, with which argument block, is decided by host code.  This program
// includes ONE of the two sources (host side only: the kernels become host stubs), defines the dozen HIP runtime symbols that
// host code touches as logging stubs, and runs a table of calls on fake pointers through every C entry of that source.  Every
// launch is one line: the demangled kernel instantiation, grid, block, dynamic LDS, and every field of the argument struct by
// name (pointers as "buffer+byte offset", floats as %a); after a call's launches comes its return code (and message).  The log
// of a refactored launcher must equal the log of the one before, byte for byte: tests/test_kernel_launch_log_cpu.py compares
// per-case digests with tests/golden/kernel_launch_log.txt and checks that the launched kernels are ALL the instantiations.
//
//   hipcc --offload-host-only -std=c++17 -O1 -rdynamic -Wl,--unresolved-symbols=ignore-all -I include -I esm-efficient_amd/csrc \
//         -DESME_KLL_GEMM -DESME_SRC='"<abs path>/gemm.hip"' -o kll -x hip tools/kernel_launch_log.cpp esm-efficient_amd/csrc/api.hip -ldl
//   (attention: -DESME_KLL_ATTN and attn.hip.  --unresolved-symbols: only the __hip_fatbin_<hash> reference of a host-only object.)
//   ./kll            every case: "== name launches" line, then its log
//   ./kll --dump C   the log of case C alone (diff it against a build with another gemm.hip / attn.hip)
//   ./kll --cases F  (GEMM build) the launches of the calls listed in file F, one "form M N K tile persist raster_gm raster_gn device" per line
#include ESME_SRC

#include <cxxabi.h>
#include <dlfcn.h>
#include <stdarg.h>
#include <string.h>

#include <functional>
#include <set>
#include <string>
#include <utility>
#include <vector>

#if defined(ESME_KLL_GEMM) == defined(ESME_KLL_ATTN)
#error "define exactly one of ESME_KLL_GEMM / ESME_KLL_ATTN"
#endif

namespace kll {

// ---- fake device buffers: named address ranges that are never dereferenced
constexpr uintptr_t kBase = uintptr_t(1) << 44;
constexpr int kShift = 36;                               // 64 GiB per buffer
std::vector<std::string> g_names;
std::string g_log;
int g_launches = 0;
int g_dev = 0;                                           // what hipGetDevice answers
std::set<std::pair<std::string, int>> g_lds;             // (kernel, bytes) of every hipFuncSetAttribute

template <class T = void> T* buf(const std::string& name, int64_t byte_off = 0) {
    size_t i = 0;
    while (i < g_names.size() && g_names[i] != name) ++i;
    if (i == g_names.size()) g_names.push_back(name);
    return reinterpret_cast<T*>(kBase + (uintptr_t(i) << kShift) + byte_off);
}

std::string P(const void* p) {
    if (!p) return "null";
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    char tmp[96];
    if (a >= kBase && ((a - kBase) >> kShift) < g_names.size()) {
        snprintf(tmp, sizeof tmp, "+%llu", (unsigned long long)((a - kBase) & ((uintptr_t(1) << kShift) - 1)));
        return g_names[(a - kBase) >> kShift] + tmp;
    }
    snprintf(tmp, sizeof tmp, "?%llx", (unsigned long long)a);
    return tmp;
}
#define S(p) kll::P(p).c_str()
typedef long long ll;

void emit(const char* fmt, ...) {
    char line[8192];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    g_log += line;
    g_log += '\n';
}

std::string kernel_name(const void* f) {
    Dl_info info;
    if (!dladdr(f, &info) || !info.dli_sname) return "?";
    int st = 0;
    char* d = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &st);
    std::string n = d ? d : info.dli_sname;
    free(d);
    const size_t stub = n.find("__device_stub__");
    if (stub != std::string::npos) n.erase(stub, strlen("__device_stub__"));
    return n;
}

#ifdef ESME_KLL_GEMM
std::string args_of(const std::string&, const void* p) {
    const esme::GemmArgs& a = *static_cast<const esme::GemmArgs*>(p);
    char t[4096];
    snprintf(t, sizeof t,
             "A=%s lda=%lld W=%s bias=%s resid=%s ldr=%lld C=%s ldc=%lld M=%lld N=%d K=%d alpha=%a tiles_n=%d vec_ok=%d cosT=%s sinT=%s pos=%s "
             "max_len=%d rot_cols=%d tiles_m=%d gm=%d gn=%d nt_store=%d stagger=%d ln_partial=%s ln_nblk=%d ln_dim=%d ln_eps=%a ln_c1=%s ln_c2=%s "
             "stats_out=%s stat_ld=%lld trace=%s opt_gm=%d opt_gn=%d opt_persist=%d q_scale=%a q_cols=%d resid32=%s ld32=%lld kt_wrap=%d "
             "pair_off=%lld c32=%s ldc32=%lld f16=%d ps_in=%s ps_out=%s ext_sel=%s ext_n=%d ext_off=%lld ext_base=%d ovf=%s pair_cols=%d "
             "col_absmax=%s qk_sumsq=%s stream_out=%d",
             S(a.A), (ll)a.lda, S(a.W), S(a.bias), S(a.resid), (ll)a.ldr, S(a.C), (ll)a.ldc, (ll)a.M, a.N, a.K, a.alpha, a.tiles_n, a.vec_ok, S(a.cosT),
             S(a.sinT), S(a.pos), a.max_len, a.rot_cols, a.tiles_m, a.gm, a.gn, a.nt_store, a.stagger, S(a.ln_partial), a.ln_nblk, a.ln_dim, a.ln_eps,
             S(a.ln_c1), S(a.ln_c2), S(a.stats_out), (ll)a.stat_ld, S(a.trace), a.opt_gm, a.opt_gn, a.opt_persist, a.q_scale, a.q_cols, S(a.resid32),
             (ll)a.ld32, a.kt_wrap, (ll)a.pair_off, S(a.c32), (ll)a.ldc32, a.f16, S(a.ps_in), S(a.ps_out), S(a.ext_sel), a.ext_n, (ll)a.ext_off, a.ext_base,
             S(a.ovf), a.pair_cols, S(a.col_absmax), S(a.qk_sumsq), a.stream_out);
    return t;
}
#else
std::string attn_args(const AttnArgs& a) {
    char t[1024];
    snprintf(t, sizeof t, "q=%s k=%s v=%s ld=%lld o=%s ldo=%lld cu=%s H=%d scale_log2=%a nqt=%d nhb=%d thr=%a spec=%d order=%s", S(a.q), S(a.k), S(a.v),
             (ll)a.ld, S(a.o), (ll)a.ldo, S(a.cu), a.H, a.scale_log2, a.nqt, a.nhb, a.thr, a.spec, S(a.order));
    return t;
}
std::string args_of(const std::string& kernel, const void* p) {
    if (kernel.find("AttnSplitArgs") == std::string::npos) return attn_args(*static_cast<const AttnArgs*>(p));
    const AttnSplitArgs& sa = *static_cast<const AttnSplitArgs*>(p);
    char t[128];
    snprintf(t, sizeof t, " lo_in=%lld lo_out=%lld", (ll)sa.lo_in, (ll)sa.lo_out);
    return attn_args(sa.a) + t;
}
#endif

struct CallConfig { dim3 grid, block; size_t smem; hipStream_t stream; } g_cfg;

}  // namespace kll

// ---- the runtime symbols host code touches (they interpose on the runtime library)
extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned int, void*, void*, void*, void*, int*) {}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void**) {}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t smem, hipStream_t stream) {
    kll::g_cfg = {grid, block, smem, stream};
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* smem, hipStream_t* stream) {
    *grid = kll::g_cfg.grid; *block = kll::g_cfg.block; *smem = kll::g_cfg.smem; *stream = kll::g_cfg.stream;
    return hipSuccess;
}
hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t smem, hipStream_t stream) {
    const std::string k = kll::kernel_name(f);
    ++kll::g_launches;
    kll::emit("launch %s grid=%u,%u,%u block=%u,%u,%u smem=%zu stream=%s %s", k.c_str(), grid.x, grid.y, grid.z, block.x, block.y, block.z, smem, S(stream),
              kll::args_of(k, args[0]).c_str());
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipFuncSetAttribute(const void* f, hipFuncAttribute, int value) {
    kll::g_lds.insert({kll::kernel_name(f), value});
    return hipSuccess;
}
hipError_t hipGetDevice(int* dev) { *dev = kll::g_dev; return hipSuccess; }
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t, int dev) {          // compute units by ordinal
    *v = dev == 1 ? 4 : dev == 2 ? 300 : 256;
    return hipSuccess;
}
}  // extern "C"

namespace kll {

typedef std::function<void()> Body;
std::vector<std::pair<std::string, Body>> g_cases;
void add(const std::string& name, Body b) { g_cases.push_back({name, std::move(b)}); }
void rc_line(int rc) {
    if (rc) emit("rc=%d err=%s", rc, esme_hip_last_error());
    else emit("rc=0");
}

#ifdef ESME_KLL_GEMM
// ================================================================ GEMM
struct GC {
    const void *A = buf("A"), *W = buf("W"), *bias = buf("bias"), *resid = nullptr;
    void* C = buf("C");
    int64_t lda = -1, ldr = -1, ldc = -1, M = 300;       // -1: derived at the call (lda = K; ldc = ldr = n_out, or room for a pair)
    int N = 768, K = 256, epi = ESME_EPI_NONE;
    float alpha = 0.75f;
    esme_gemm_fusion_t fu{};
    bool use_fu = false;
    esme_gemm_opts_t op{(int)sizeof(esme_gemm_opts_t), 0, 0, 0, -1};
    bool use_op = false;
    int dev = 0;
    int entry = 0;                                        // 0 _opts, 1 _fused, 2 plain, 3 _qkv_rotary
};

int call(const GC& c) {
    g_dev = c.dev;
    const int n_out = c.epi == ESME_EPI_SWIGLU ? c.N / 2 : c.N;
    const int64_t lda = c.lda >= 0 ? c.lda : c.K;
    const int64_t wide = c.use_fu && c.fu.pair_off ? 2 * c.fu.pair_off + 2 * c.N : n_out;
    const int64_t ldc = c.ldc >= 0 ? c.ldc : wide, ldr = c.ldr >= 0 ? c.ldr : wide;
    void* st = buf("stream");
    int rc;
    if (c.entry == 0) rc = esme_hip_gemm_bf16_opts(c.A, lda, c.W, c.bias, c.resid, ldr, c.C, ldc, c.M, c.N, c.K, c.epi, c.alpha, c.use_fu ? &c.fu : nullptr, c.use_op ? &c.op : nullptr, st);
    else if (c.entry == 1) rc = esme_hip_gemm_bf16_fused(c.A, lda, c.W, c.bias, c.resid, ldr, c.C, ldc, c.M, c.N, c.K, c.epi, c.alpha, c.use_fu ? &c.fu : nullptr, st);
    else if (c.entry == 2) rc = esme_hip_gemm_bf16(c.A, lda, c.W, c.bias, c.resid, ldr, c.C, ldc, c.M, c.N, c.K, c.epi, c.alpha, st);
    else rc = esme_hip_gemm_qkv_rotary(c.A, lda, c.W, c.bias, c.C, ldc, c.M, c.N, c.K, c.fu.cos, c.fu.sin, c.fu.pos, c.fu.head_dim, c.fu.max_len, c.fu.rot_cols, st);
    rc_line(rc);
    return rc;
}

// the fusion fields of one feature, valid for the call's N / K as they are when the helper runs
void tile(GC& c, int t) { c.use_op = true; c.op.tile = t; }
void ln(GC& c) {
    c.use_fu = true;
    c.fu.ln_partial = buf<float>("ln_partial"); c.fu.ln_nblk = 2; c.fu.ln_dim = c.K; c.fu.ln_eps = 1e-5f;
    c.fu.ln_c1 = buf<float>("ln_c1"); c.fu.ln_c2 = buf<float>("ln_c2"); c.fu.overflow_flag = buf<int>("overflow_flag");
}
void rot(GC& c, int d) {
    c.use_fu = true;
    c.fu.cos = buf("cos"); c.fu.sin = buf("sin"); c.fu.pos = buf<int32_t>("pos"); c.fu.head_dim = d; c.fu.max_len = 1026;
    c.fu.rot_cols = c.N / 64 * 2 / 3 * 64;
}
void qscale(GC& c) { c.fu.q_scale = 0.125f; c.fu.q_cols = c.fu.rot_cols / 2 / 64 * 64; }
void stats(GC& c) { c.use_fu = true; c.fu.stats_out = buf<float>("stats_out"); }
void residual(GC& c) { c.epi = ESME_EPI_RESIDUAL; c.resid = buf("resid"); }
void r32(GC& c) { c.use_fu = true; c.epi = ESME_EPI_RESIDUAL; c.fu.resid32 = buf<float>("resid32"); c.fu.ld32 = c.N; }
void f16(GC& c) { c.use_fu = true; c.fu.f16 = 1; }
void pair_out(GC& c) { c.use_fu = true; c.fu.pair_off = (c.epi == ESME_EPI_SWIGLU ? c.N / 2 : c.N) + 128; }     // bf16 (hi, lo) output; with f16 + ln: the fp16 pair output
void pair_stream(GC& c) { f16(c); residual(c); c.fu.pair_off = c.N + 128; }
void pair_stream_all(GC& c) {                            // every optional operand of the pair stream's epilogue
    pair_stream(c); stats(c);
    c.fu.pair_scale_in = buf<float>("ps_in"); c.fu.pair_scale_out = buf<float>("ps_out");
    c.fu.ext_sel = buf<int32_t>("ext_sel"); c.fu.ext_n = 5; c.fu.ext_off = c.N;
    c.fu.col_absmax = buf<uint32_t>("col_absmax");
}
void split_a(GC& c, int mult) { c.use_fu = true; c.fu.w_k = c.K; c.K *= mult; }
void c32(GC& c) { c.use_fu = true; c.fu.c32 = buf<float>("c32"); c.fu.ldc32 = c.N; }

// the 38 shipped forms: 16 bf16, 6 bf16 pair output, 4 fp16 pair output, 12 fp16
struct Form { const char* name; void (*set)(GC&); };
const Form kForms[] = {
    {"bf16_none", [](GC&) {}},
    {"bf16_none_ln", [](GC& c) { ln(c); }},
    {"bf16_rot16", [](GC& c) { rot(c, 16); }},
    {"bf16_rot32", [](GC& c) { rot(c, 32); }},
    {"bf16_rot64", [](GC& c) { rot(c, 64); qscale(c); }},
    {"bf16_rot16_ln", [](GC& c) { rot(c, 16); ln(c); }},
    {"bf16_rot32_ln", [](GC& c) { rot(c, 32); ln(c); }},
    {"bf16_rot64_ln", [](GC& c) { rot(c, 64); qscale(c); ln(c); }},
    {"bf16_gelu", [](GC& c) { c.epi = ESME_EPI_GELU; }},
    {"bf16_gelu_ln", [](GC& c) { c.epi = ESME_EPI_GELU; ln(c); }},
    {"bf16_swiglu", [](GC& c) { c.epi = ESME_EPI_SWIGLU; }},
    {"bf16_swiglu_ln", [](GC& c) { c.epi = ESME_EPI_SWIGLU; ln(c); }},
    {"bf16_resid", [](GC& c) { residual(c); }},
    {"bf16_resid_stats", [](GC& c) { residual(c); stats(c); }},
    {"bf16_r32", [](GC& c) { r32(c); }},
    {"bf16_r32_stats", [](GC& c) { r32(c); stats(c); }},
    {"pair_none", [](GC& c) { pair_out(c); }},
    {"pair_rot16", [](GC& c) { rot(c, 16); pair_out(c); }},
    {"pair_rot32", [](GC& c) { rot(c, 32); pair_out(c); }},
    {"pair_rot64", [](GC& c) { rot(c, 64); pair_out(c); split_a(c, 2); }},
    {"pair_gelu", [](GC& c) { c.epi = ESME_EPI_GELU; pair_out(c); split_a(c, 2); }},
    {"pair_swiglu", [](GC& c) { c.epi = ESME_EPI_SWIGLU; pair_out(c); }},
    {"f16pair_none", [](GC& c) { f16(c); ln(c); pair_out(c); }},
    {"f16pair_rot16", [](GC& c) { f16(c); ln(c); rot(c, 16); pair_out(c); }},
    {"f16pair_rot32", [](GC& c) { f16(c); ln(c); rot(c, 32); pair_out(c); c.fu.pair_cols = 512; }},
    {"f16pair_rot64", [](GC& c) { f16(c); ln(c); rot(c, 64); pair_out(c); c.fu.pair_cols = 256; }},
    {"f16_none", [](GC& c) { f16(c); }},
    {"f16_none_ln", [](GC& c) { f16(c); ln(c); }},
    {"f16_rot16_ln", [](GC& c) { f16(c); ln(c); rot(c, 16); }},
    {"f16_rot32_ln", [](GC& c) { f16(c); ln(c); rot(c, 32); qscale(c); }},
    {"f16_rot64_ln", [](GC& c) { f16(c); ln(c); rot(c, 64); qscale(c); c.fu.qk_sumsq = buf<uint32_t>("qk_sumsq"); }},
    {"f16_gelu", [](GC& c) { f16(c); c.epi = ESME_EPI_GELU; }},
    {"f16_gelu_ln", [](GC& c) { f16(c); c.epi = ESME_EPI_GELU; ln(c); }},
    {"f16_swiglu_ln", [](GC& c) { f16(c); c.epi = ESME_EPI_SWIGLU; ln(c); }},
    {"f16_r32", [](GC& c) { f16(c); r32(c); }},
    {"f16_r32_stats", [](GC& c) { f16(c); r32(c); stats(c); }},
    {"f16_stream", [](GC& c) { pair_stream(c); }},
    {"f16_stream_stats", [](GC& c) { pair_stream_all(c); }},
};

void refuse(const std::string& name, std::function<void(GC&)> f) {
    add("gemm_refuse_" + name, [f] { GC c; f(c); call(c); });
}

void cases() {
    // every form x {heuristic, tile 1, tile 2} x M = 300 (6 big tiles), 25 600 (300: one workgroup per tile), 51 200 (600: persistent where it exists)
    for (const Form& f : kForms)
        for (int t = 0; t <= 2; ++t)
            add(std::string("gemm_") + f.name + "_tile" + std::to_string(t), [&f, t] {
                for (int64_t M : {300, 25600, 51200}) {
                    GC c; c.M = M; f.set(c); if (t) tile(c, t);
                    call(c);
                }
            });
    // persistence: option -1 / 0 / 1 on both sides of blocks >= 2 * ncu, at 256, 4 and 300 compute units (3 tile columns)
    for (int dev = 0; dev <= 2; ++dev)
        for (int p = -1; p <= 1; ++p)
            add("gemm_persist_dev" + std::to_string(dev) + "_opt" + std::to_string(p), [dev, p] {
                for (int tm : {170, 171, 197, 198}) {
                    GC c; c.dev = dev; c.M = 256 * tm - 3; c.epi = ESME_EPI_GELU; ln(c); tile(c, 2); c.op.persist = p;
                    call(c);
                }
            });
    add("gemm_persist_needs_vec_ok", [] {
        GC c; c.M = 256 * 600; c.N = 33; c.ldc = 40; tile(c, 2); call(c);
        GC d; d.M = 256 * 600; d.N = 512; c32(d); tile(d, 2); call(d);
    });
    add("gemm_heuristic_tile", [] {
        for (auto mn : {std::pair<int, int>{53, 768}, {54, 768}, {39, 1024}, {40, 1024}, {1000, 192}, {1000, 255}, {160, 256}}) {
            GC c; c.M = 256 * mn.first; c.N = mn.second; call(c);
        }
    });
    add("gemm_stats_blocks", [] {
        esme_gemm_opts_t o{(int)sizeof(esme_gemm_opts_t), 0, 0, 0, -1};
        for (auto mn : {std::pair<int, int>{300, 768}, {256 * 54, 768}, {256 * 53, 768}, {256 * 1000, 192}, {300, 1152}, {32064, 1152}}) {
            std::string l = "stats_blocks M=" + std::to_string(mn.first) + " N=" + std::to_string(mn.second) + ":";
            l += " " + std::to_string(esme_hip_gemm_stats_blocks(mn.first, mn.second));
            for (int t = 0; t <= 2; ++t) { o.tile = t; l += " " + std::to_string(esme_hip_gemm_stats_blocks_opts(mn.first, mn.second, &o)); }
            emit("%s", l.c_str());
        }
    });
    add("gemm_raster", [] {
        struct R { int N, K, tile, gm, gn; int64_t M; };
        for (R r : {R{1792, 960, 2, 0, 0, 5000}, R{1792, 1024, 2, 0, 0, 5000}, R{1792, 960, 1, 0, 0, 5000}, R{1792, 1024, 1, 0, 0, 5000},   // w_bytes either side of 3.5e6
                    R{1536, 2048, 2, 0, 0, 5000}, R{1536, 2048, 1, 0, 0, 5000},                                                        // tiles_n <= 6 (and 12)
                    R{2560, 1024, 2, 0, 0, 5000}, R{5120, 1280, 2, 0, 0, 5000}, R{5120, 1280, 1, 0, 0, 5000}, R{1280, 2048, 1, 0, 0, 5000},  // tiles_n % 5 == 0
                    R{2048, 1024, 2, 0, 0, 5000}, R{2048, 1024, 2, 0, 0, 300},                                                          // neither; gm clamped to tiles_m
                    R{2048, 1024, 2, 3, 2, 5000}, R{2048, 1024, 2, 3, 0, 5000}, R{2048, 1024, 2, 100, 100, 300}, R{2048, 1024, 1, 1, 1, 300},
                    R{2048, 1024, 2, -1, 2, 5000}, R{2048, 1024, 2, 0, 3, 5000}, R{2560, 1024, 0, 2, 2, 256 * 200}}) {
            GC c; c.N = r.N; c.K = r.K; c.M = r.M; tile(c, r.tile); c.op.raster_gm = r.gm; c.op.raster_gn = r.gn;
            call(c);
        }
    });
    add("gemm_vec_ok", [] {
        { GC c; c.N = 33; c.ldc = 40; call(c); }
        { GC c; c.N = 33; c.ldc = 33; call(c); }
        { GC c; c.N = 4; c.ldc = 8; call(c); }
        { GC c; c.N = 64; c.ldc = 68; call(c); }
        { GC c; c.C = buf("C", 8); call(c); }
        { GC c; residual(c); c.resid = buf("resid", 8); call(c); }
        { GC c; residual(c); c.ldr = 772; call(c); }
        { GC c; residual(c); c.N = 36; c.ldc = 40; c.ldr = 40; c.bias = nullptr; call(c); }
        { GC c; c.epi = ESME_EPI_GELU; c.N = 100; c.ldc = 104; c.M = 256 * 700; tile(c, 2); call(c); }      // N % 8 != 0
    });
    add("gemm_stream_out", [] {                              // bytes written against 256 MiB
        { GC c; c.N = 1024; c.M = 131072; call(c); }
        { GC c; c.N = 1024; c.M = 131073; call(c); }
        { GC c; c.N = 1024; c.M = 65537; pair_out(c); call(c); }
        { GC c; c.N = 1024; c.M = 65536; pair_out(c); call(c); }
        { GC c; c.N = 1024; c.M = 43691; r32(c); call(c); }
        { GC c; c.N = 1024; c.M = 43690; r32(c); call(c); }
        { GC c; c.N = 1024; c.M = 262145; c.epi = ESME_EPI_SWIGLU; call(c); }
        { GC c; c.N = 1024; c.M = 262144; c.epi = ESME_EPI_SWIGLU; call(c); }
        { GC c; c.N = 1024; c.M = 65537; pair_stream(c); call(c); }
    });
    // the column split: fp16 pair stream, N % 256 == 128, heuristic tile, and a whole round of 256-tiles saved
    for (int dev = 0; dev <= 2; ++dev)
        add("gemm_colsplit_dev" + std::to_string(dev), [dev] {
            for (int64_t M : {32064, 25600, 9000}) {            // 126 tile rows: 504 / 630 tiles; 100: 400 / 500; 36: main tiles < 160
                GC c; c.dev = dev; c.M = M; c.N = 1152; c.K = 1152; pair_stream_all(c); call(c);
            }
            { GC c; c.dev = dev; c.M = 32064; c.N = 1152; c.K = 1152; pair_stream(c); c.bias = nullptr; call(c); }     // no optional operand
            { GC c; c.dev = dev; c.M = 256 * 300; c.N = 384; pair_stream_all(c); c.fu.ext_n = 0; c.fu.ext_sel = nullptr; call(c); }
            { GC c; c.dev = dev; c.M = 32064; c.N = 1152; pair_stream_all(c); tile(c, 2); call(c); }                     // explicit tile: never split
            { GC c; c.dev = dev; c.M = 32064; c.N = 1152; pair_stream_all(c); tile(c, 0); c.op.persist = 1; c.op.raster_gm = 2; c.op.raster_gn = 2; call(c); }
            { GC c; c.dev = dev; c.M = 32064; c.N = 1280; pair_stream_all(c); call(c); }                                 // N % 256 == 0
            { GC c; c.dev = dev; c.M = 256 * 300; c.N = 128; pair_stream_all(c); call(c); }                              // N <= 256
            { GC c; c.dev = dev; c.M = 32064; c.N = 1152; residual(c); stats(c); call(c); }                              // bf16: one launch
            { GC c; c.dev = dev; c.M = 32064; c.N = 1152; f16(c); r32(c); stats(c); call(c); }                           // fp16 on the fp32 stream: one launch
        });
    add("gemm_split_operand", [] {
        { GC c; split_a(c, 1); call(c); }
        { GC c; split_a(c, 2); call(c); }
        { GC c; split_a(c, 2); c.epi = ESME_EPI_GELU; pair_out(c); c.M = 51200; call(c); }
        { GC c; split_a(c, 2); residual(c); call(c); }
        { GC c; c32(c); call(c); }
        { GC c; c32(c); c.N = 33; c.fu.ldc32 = 33; c.ldc = 40; split_a(c, 2); call(c); }
        { GC c; c32(c); c.epi = ESME_EPI_GELU; call(c); }
        { GC c; c32(c); residual(c); call(c); }
        { GC c; c32(c); r32(c); c.M = 51200; tile(c, 2); call(c); }
    });
    add("gemm_entries", [] {
        { GC c; c.M = 0; call(c); }
        { GC c; c.M = 0; c.A = c.W = nullptr; c.C = nullptr; c.K = 100; call(c); }            // M = 0 returns before the pointer and K checks
        { GC c; c.entry = 1; ln(c); call(c); }
        { GC c; c.entry = 1; call(c); }
        { GC c; c.entry = 2; residual(c); call(c); }
        { GC c; c.entry = 2; c.epi = ESME_EPI_SWIGLU; c.M = 51200; call(c); }
        { GC c; c.entry = 3; rot(c, 64); call(c); }
        { GC c; c.entry = 3; rot(c, 16); c.M = 51200; call(c); }
        { GC c; c.entry = 3; rot(c, 0); call(c); }
        { GC c; c.entry = 3; rot(c, 128); call(c); }
        { GC c; c.bias = nullptr; c.alpha = -2.5f; residual(c); call(c); }
        { GC c; rot(c, 64); c.fu.rot_cols = 0; call(c); }
        { GC c; rot(c, 64); c.fu.rot_cols = c.N; qscale(c); c.fu.q_cols = c.N; call(c); }
        { GC c; f16(c); ln(c); c.fu.overflow_flag = nullptr; call(c); }
    });

    // ---- refusals, in the order the entry checks them; "a+b" violates both (the golden fixes which message wins)
    refuse("opts_abi", [](GC& c) { tile(c, 1); c.op.struct_bytes -= 4; });
    refuse("opts_tile3", [](GC& c) { tile(c, 3); });
    refuse("opts_tile_neg", [](GC& c) { tile(c, -1); });
    refuse("opts_abi+sizes", [](GC& c) { tile(c, 3); c.N = 0; });
    refuse("sizes_M", [](GC& c) { c.M = -1; });
    refuse("sizes_N", [](GC& c) { c.N = 0; });
    refuse("sizes_K", [](GC& c) { c.K = 0; });
    refuse("sizes+epilogue", [](GC& c) { c.K = -64; c.epi = 7; });
    refuse("epilogue_hi", [](GC& c) { c.epi = ESME_EPI_SWIGLU + 1; });
    refuse("epilogue_lo", [](GC& c) { c.epi = -1; });
    refuse("epilogue+null", [](GC& c) { c.epi = 9; c.A = nullptr; });
    refuse("null_A", [](GC& c) { c.A = nullptr; });
    refuse("null_W", [](GC& c) { c.W = nullptr; });
    refuse("null_C", [](GC& c) { c.C = nullptr; });
    refuse("null+K", [](GC& c) { c.C = nullptr; c.K = 100; });
    refuse("K", [](GC& c) { c.K = 100; });
    refuse("K+swiglu_N", [](GC& c) { c.K = 100; c.epi = ESME_EPI_SWIGLU; c.N = 800; });
    refuse("swiglu_N", [](GC& c) { c.epi = ESME_EPI_SWIGLU; c.N = 800; });
    refuse("swiglu_N+ld", [](GC& c) { c.epi = ESME_EPI_SWIGLU; c.N = 800; c.lda = 8; });
    refuse("lda_small", [](GC& c) { c.lda = 248; });
    refuse("lda_mod8", [](GC& c) { c.lda = 260; });
    refuse("ldc_small", [](GC& c) { c.ldc = 760; });
    refuse("ldc_small_swiglu", [](GC& c) { c.epi = ESME_EPI_SWIGLU; c.ldc = 376; });
    refuse("ld+align", [](GC& c) { c.ldc = 760; c.A = buf("A", 8); });
    refuse("align_A", [](GC& c) { c.A = buf("A", 8); });
    refuse("align_W", [](GC& c) { c.W = buf("W", 4); });
    refuse("align+bias", [](GC& c) { c.W = buf("W", 4); c.bias = buf("bias", 2); });
    refuse("bias", [](GC& c) { c.bias = buf("bias", 4); });
    refuse("bias+r32_epilogue", [](GC& c) { c.bias = buf("bias", 4); r32(c); c.epi = ESME_EPI_NONE; });
    refuse("r32_epilogue", [](GC& c) { r32(c); c.epi = ESME_EPI_GELU; });
    refuse("r32_epilogue+ld32", [](GC& c) { r32(c); c.epi = ESME_EPI_NONE; c.fu.ld32 = 8; });
    refuse("r32_ld32_small", [](GC& c) { r32(c); c.fu.ld32 = 764; });
    refuse("r32_ld32_mod4", [](GC& c) { r32(c); c.fu.ld32 = 770; });
    refuse("r32_align", [](GC& c) { r32(c); c.fu.resid32 = buf<float>("resid32", 8); });
    refuse("r32_ld32+vec", [](GC& c) { r32(c); c.fu.ld32 = 770; c.C = buf("C", 8); });
    refuse("r32_vec", [](GC& c) { r32(c); c.C = buf("C", 8); });
    refuse("r32_vec_N", [](GC& c) { r32(c); c.N = 36; c.fu.ld32 = 36; c.ldc = 40; });
    refuse("r32_vec+stats", [](GC& c) { r32(c); c.ldc = 772; stats(c); c.fu.pair_cols = 256; });
    refuse("resid_null", [](GC& c) { c.epi = ESME_EPI_RESIDUAL; });
    refuse("resid_ldr", [](GC& c) { residual(c); c.ldr = 760; });
    refuse("resid+pair_scale", [](GC& c) { c.epi = ESME_EPI_RESIDUAL; c.use_fu = true; c.fu.pair_scale_in = buf<float>("ps_in"); });
    refuse("swiglu_vec_ldc", [](GC& c) { c.epi = ESME_EPI_SWIGLU; c.ldc = 388; });
    refuse("swiglu_vec_C", [](GC& c) { c.epi = ESME_EPI_SWIGLU; c.C = buf("C", 8); });
    refuse("swiglu_vec+pair_cols", [](GC& c) { c.epi = ESME_EPI_SWIGLU; c.C = buf("C", 8); c.use_fu = true; c.fu.pair_cols = 256; });
    refuse("pair_scale_in_bf16", [](GC& c) { c.use_fu = true; c.fu.pair_scale_in = buf<float>("ps_in"); });
    refuse("pair_scale_out_f16_plain", [](GC& c) { f16(c); c.fu.pair_scale_out = buf<float>("ps_out"); });
    refuse("ext_off_r32", [](GC& c) { f16(c); r32(c); c.fu.ext_off = c.N; });
    refuse("pair_scale_pair_output", [](GC& c) { f16(c); ln(c); pair_out(c); c.fu.pair_scale_in = buf<float>("ps_in"); });
    refuse("pair_scale+pair_cols", [](GC& c) { c.use_fu = true; c.fu.pair_scale_in = buf<float>("ps_in"); c.fu.pair_cols = 256; });
    refuse("pair_cols_bf16", [](GC& c) { pair_out(c); c.fu.pair_cols = 256; });
    refuse("pair_cols_stream", [](GC& c) { pair_stream(c); c.fu.pair_cols = 256; });
    refuse("pair_cols_f16_plain", [](GC& c) { f16(c); ln(c); c.fu.pair_cols = 256; });
    refuse("pair_cols+col_absmax", [](GC& c) { f16(c); ln(c); c.fu.pair_cols = 256; c.fu.col_absmax = buf<uint32_t>("col_absmax"); });
    refuse("col_absmax_bf16", [](GC& c) { residual(c); c.use_fu = true; c.fu.col_absmax = buf<uint32_t>("col_absmax"); });
    refuse("col_absmax_r32", [](GC& c) { f16(c); r32(c); c.fu.col_absmax = buf<uint32_t>("col_absmax"); });
    refuse("col_absmax_pair_output", [](GC& c) { f16(c); ln(c); pair_out(c); c.fu.col_absmax = buf<uint32_t>("col_absmax"); });
    refuse("col_absmax+qk_sumsq", [](GC& c) { f16(c); ln(c); rot(c, 64); pair_out(c); c.fu.col_absmax = buf<uint32_t>("col_absmax"); c.fu.qk_sumsq = buf<uint32_t>("qk_sumsq"); });
    refuse("qk_sumsq_bf16", [](GC& c) { ln(c); rot(c, 64); c.fu.qk_sumsq = buf<uint32_t>("qk_sumsq"); });
    refuse("qk_sumsq_no_ln", [](GC& c) { f16(c); rot(c, 64); c.fu.qk_sumsq = buf<uint32_t>("qk_sumsq"); });
    refuse("qk_sumsq_no_rotary", [](GC& c) { f16(c); ln(c); c.fu.qk_sumsq = buf<uint32_t>("qk_sumsq"); });
    refuse("qk_sumsq_pair_output", [](GC& c) { f16(c); ln(c); rot(c, 64); pair_out(c); c.fu.qk_sumsq = buf<uint32_t>("qk_sumsq"); });
    refuse("qk_sumsq+f16pair_ln", [](GC& c) { f16(c); pair_out(c); c.fu.qk_sumsq = buf<uint32_t>("qk_sumsq"); });
    refuse("qk_sumsq+f16_w_k", [](GC& c) { f16(c); ln(c); rot(c, 64); split_a(c, 2); c.fu.qk_sumsq = buf<uint32_t>("qk_sumsq"); });
    refuse("qk_sumsq+f16_c32", [](GC& c) { f16(c); ln(c); rot(c, 64); c32(c); c.fu.qk_sumsq = buf<uint32_t>("qk_sumsq"); });
    refuse("qk_sumsq+bad_w_k", [](GC& c) { f16(c); ln(c); rot(c, 64); c.fu.w_k = 100; c.fu.qk_sumsq = buf<uint32_t>("qk_sumsq"); });
    refuse("qk_sumsq_align+f16_c32", [](GC& c) { f16(c); ln(c); rot(c, 64); c32(c); c.fu.qk_sumsq = buf<uint32_t>("qk_sumsq", 2); });
    refuse("qk_sumsq+stream_epilogue", [](GC& c) { f16(c); pair_out(c); c.epi = ESME_EPI_GELU; c.fu.qk_sumsq = buf<uint32_t>("qk_sumsq"); });
    // the fp16 pair output
    refuse("f16pair_no_ln", [](GC& c) { f16(c); pair_out(c); });
    refuse("f16pair_w_k", [](GC& c) { f16(c); ln(c); pair_out(c); c.fu.w_k = c.K; });
    refuse("f16pair_c32", [](GC& c) { f16(c); ln(c); pair_out(c); c32(c); });
    refuse("f16pair_stats", [](GC& c) { f16(c); ln(c); pair_out(c); stats(c); });
    refuse("f16pair_no_ln+pair_off", [](GC& c) { f16(c); pair_out(c); c.fu.pair_off = 4; });
    refuse("f16pair_off_small", [](GC& c) { f16(c); ln(c); pair_out(c); c.fu.pair_off = 760; c.ldc = 4096; });
    refuse("f16pair_off_mod8", [](GC& c) { f16(c); ln(c); pair_out(c); c.fu.pair_off = 900; c.ldc = 4096; });
    refuse("f16pair_ldc", [](GC& c) { f16(c); ln(c); pair_out(c); c.ldc = c.fu.pair_off + c.N - 8; });
    refuse("f16pair_ldc_pair_cols", [](GC& c) { f16(c); ln(c); pair_out(c); c.fu.pair_cols = 512; c.ldc = c.fu.pair_off + 504; });
    refuse("f16pair_cols_neg", [](GC& c) { f16(c); ln(c); pair_out(c); c.fu.pair_cols = -256; });
    refuse("f16pair_cols_mod", [](GC& c) { f16(c); ln(c); pair_out(c); c.fu.pair_cols = 128; });
    refuse("f16pair_off+vec", [](GC& c) { f16(c); ln(c); pair_out(c); c.fu.pair_off = 900; c.ldc = 4100; });
    refuse("f16pair_vec", [](GC& c) { f16(c); ln(c); pair_out(c); c.C = buf("C", 8); });
    refuse("f16pair_vec+rotary_tables", [](GC& c) { f16(c); ln(c); rot(c, 64); pair_out(c); c.C = buf("C", 8); c.fu.cos = nullptr; });
    // the fp16 pair stream
    refuse("stream_epilogue", [](GC& c) { f16(c); pair_out(c); c.epi = ESME_EPI_GELU; });
    refuse("stream_swiglu", [](GC& c) { f16(c); c.epi = ESME_EPI_SWIGLU; pair_out(c); });
    refuse("stream_r32", [](GC& c) { pair_stream(c); c.fu.resid32 = buf<float>("resid32"); c.fu.ld32 = c.N; });
    refuse("stream_w_k", [](GC& c) { pair_stream(c); c.fu.w_k = c.K; });
    refuse("stream_c32", [](GC& c) { pair_stream(c); c32(c); });
    refuse("stream_ln", [](GC& c) { pair_stream(c); ln(c); });
    refuse("stream_ln+pair_off", [](GC& c) { pair_stream(c); ln(c); c.fu.pair_off = 12; });
    refuse("stream_off_small", [](GC& c) { pair_stream(c); c.fu.pair_off = 760; c.ldc = c.ldr = 4096; });
    refuse("stream_off_mod8", [](GC& c) { pair_stream(c); c.fu.pair_off = 900; c.ldc = c.ldr = 4096; });
    refuse("stream_ldc", [](GC& c) { pair_stream(c); c.ldc = c.fu.pair_off + c.N - 8; c.ldr = 4096; });
    refuse("stream_ldr", [](GC& c) { pair_stream(c); c.ldr = c.fu.pair_off + c.N - 8; c.ldc = 4096; });
    refuse("stream_off+vec", [](GC& c) { pair_stream(c); c.fu.pair_off = 900; c.ldc = c.ldr = 4096; c.C = buf("C", 8); });
    refuse("stream_vec_C", [](GC& c) { pair_stream(c); c.C = buf("C", 8); });
    refuse("stream_vec_resid", [](GC& c) { pair_stream(c); c.resid = buf("resid", 8); });
    refuse("stream_vec+scale_align", [](GC& c) { pair_stream_all(c); c.resid = buf("resid", 8); c.fu.pair_scale_in = buf<float>("ps_in", 4); });
    refuse("stream_scale_in_align", [](GC& c) { pair_stream_all(c); c.fu.pair_scale_in = buf<float>("ps_in", 4); });
    refuse("stream_scale_out_align", [](GC& c) { pair_stream_all(c); c.fu.pair_scale_out = buf<float>("ps_out", 8); });
    refuse("stream_scale+ext", [](GC& c) { pair_stream_all(c); c.fu.pair_scale_out = buf<float>("ps_out", 8); c.fu.ext_n = 65; });
    refuse("stream_ext_off_small", [](GC& c) { pair_stream_all(c); c.fu.ext_off = c.N - 64; });
    refuse("stream_ext_off_large", [](GC& c) { pair_stream_all(c); c.fu.ext_off = c.N + 128; });
    refuse("stream_ext_n_neg", [](GC& c) { pair_stream_all(c); c.fu.ext_n = -1; });
    refuse("stream_ext_n_65", [](GC& c) { pair_stream_all(c); c.fu.ext_n = 65; });
    refuse("stream_ext_sel_null", [](GC& c) { pair_stream_all(c); c.fu.ext_sel = nullptr; });
    refuse("stream_ext+col_absmax", [](GC& c) { pair_stream_all(c); c.fu.ext_n = 65; c.fu.col_absmax = buf<uint32_t>("col_absmax", 2); });
    refuse("stream_col_absmax_align", [](GC& c) { pair_stream_all(c); c.fu.col_absmax = buf<uint32_t>("col_absmax", 2); });
    refuse("stream_col_absmax+stats_align", [](GC& c) { pair_stream_all(c); c.fu.col_absmax = buf<uint32_t>("col_absmax", 2); c.fu.stats_out = buf<float>("stats_out", 4); });
    refuse("stream_rotary", [](GC& c) { pair_stream(c); rot(c, 64); });
    // split-operand mode
    refuse("w_k_neg", [](GC& c) { c.use_fu = true; c.fu.w_k = -64; });
    refuse("w_k_mod", [](GC& c) { c.use_fu = true; c.fu.w_k = 100; });
    refuse("w_k_3x", [](GC& c) { split_a(c, 3); });
    refuse("w_k_larger", [](GC& c) { c.use_fu = true; c.fu.w_k = 512; });
    refuse("w_k+pair_epilogue", [](GC& c) { split_a(c, 3); residual(c); pair_out(c); });
    refuse("pair_residual", [](GC& c) { residual(c); pair_out(c); });
    refuse("pair_ln", [](GC& c) { ln(c); pair_out(c); });
    refuse("pair_stats", [](GC& c) { pair_out(c); stats(c); });
    refuse("pair_epilogue+off", [](GC& c) { ln(c); pair_out(c); c.fu.pair_off = 12; });
    refuse("pair_off_small", [](GC& c) { pair_out(c); c.fu.pair_off = 760; c.ldc = 4096; });
    refuse("pair_off_mod8", [](GC& c) { pair_out(c); c.fu.pair_off = 900; c.ldc = 4096; });
    refuse("pair_off_swiglu", [](GC& c) { c.epi = ESME_EPI_SWIGLU; pair_out(c); c.ldc = c.fu.pair_off + 376; });
    refuse("pair_off+vec", [](GC& c) { pair_out(c); c.fu.pair_off = 900; c.ldc = 4100; });
    refuse("pair_vec", [](GC& c) { pair_out(c); c.C = buf("C", 8); });
    refuse("pair_vec+c32", [](GC& c) { pair_out(c); c.C = buf("C", 8); c32(c); });
    refuse("c32_pair", [](GC& c) { pair_out(c); c32(c); });
    refuse("c32_swiglu", [](GC& c) { c.epi = ESME_EPI_SWIGLU; c32(c); });
    refuse("c32_ldc32", [](GC& c) { c32(c); c.fu.ldc32 = 760; });
    refuse("c32_align", [](GC& c) { c32(c); c.fu.c32 = buf<float>("c32", 2); });
    refuse("c32+f16", [](GC& c) { c32(c); c.fu.ldc32 = 760; f16(c); });
    // fp16 operands
    refuse("f16_w_k", [](GC& c) { f16(c); split_a(c, 2); });
    refuse("f16_c32", [](GC& c) { f16(c); c32(c); });
    refuse("f16_split+residual", [](GC& c) { f16(c); c32(c); residual(c); });
    refuse("f16_residual_bf16_stream", [](GC& c) { f16(c); residual(c); });
    refuse("f16_residual+vec", [](GC& c) { f16(c); residual(c); c.C = buf("C", 8); });
    refuse("f16_vec", [](GC& c) { f16(c); c.C = buf("C", 8); });
    refuse("f16_vec_N", [](GC& c) { f16(c); c.N = 36; c.ldc = 40; });
    refuse("f16_vec+rotary_epilogue", [](GC& c) { f16(c); c.C = buf("C", 8); c.epi = ESME_EPI_GELU; rot(c, 64); });
    refuse("f16_rotary_no_ln", [](GC& c) { f16(c); rot(c, 32); });
    refuse("f16_swiglu_no_ln", [](GC& c) { f16(c); c.epi = ESME_EPI_SWIGLU; });
    // fused rotary
    refuse("rot_epilogue", [](GC& c) { c.epi = ESME_EPI_GELU; rot(c, 64); });
    refuse("rot_epilogue+tables", [](GC& c) { c.epi = ESME_EPI_GELU; rot(c, 64); c.fu.sin = nullptr; });
    refuse("rot_no_cos", [](GC& c) { rot(c, 64); c.fu.cos = nullptr; });
    refuse("rot_no_sin", [](GC& c) { rot(c, 64); c.fu.sin = nullptr; });
    refuse("rot_no_pos", [](GC& c) { rot(c, 64); c.fu.pos = nullptr; });
    refuse("rot_max_len", [](GC& c) { rot(c, 64); c.fu.max_len = 0; });
    refuse("rot_tables+head_dim", [](GC& c) { rot(c, 128); c.fu.pos = nullptr; });
    refuse("rot_head_dim_128", [](GC& c) { rot(c, 128); });
    refuse("rot_head_dim_48", [](GC& c) { rot(c, 48); ln(c); });
    refuse("rot_head_dim_neg", [](GC& c) { rot(c, -64); });
    refuse("rot_head_dim+cols", [](GC& c) { rot(c, 128); c.fu.rot_cols = 100; });
    refuse("rot_N", [](GC& c) { c.N = 800; rot(c, 64); });
    refuse("rot_cols_mod", [](GC& c) { rot(c, 64); c.fu.rot_cols = 100; });
    refuse("rot_cols_neg", [](GC& c) { rot(c, 64); c.fu.rot_cols = -64; });
    refuse("rot_cols_large", [](GC& c) { rot(c, 64); c.fu.rot_cols = c.N + 64; });
    refuse("rot_vec", [](GC& c) { rot(c, 64); c.C = buf("C", 8); });
    refuse("rot_cols+tables_align", [](GC& c) { rot(c, 64); c.fu.rot_cols = 100; c.fu.cos = buf("cos", 8); });
    refuse("rot_cos_align", [](GC& c) { rot(c, 64); c.fu.cos = buf("cos", 8); });
    refuse("rot_sin_align", [](GC& c) { rot(c, 64); c.fu.sin = buf("sin", 4); });
    refuse("rot_tables_align+pair_q_scale", [](GC& c) { rot(c, 64); pair_out(c); c.fu.q_scale = 0.5f; c.fu.sin = buf("sin", 4); });
    refuse("rot_pair_q_scale", [](GC& c) { rot(c, 64); pair_out(c); qscale(c); });
    refuse("rot_f16pair_q_scale", [](GC& c) { f16(c); ln(c); rot(c, 64); pair_out(c); qscale(c); });
    refuse("rot_q_cols_zero", [](GC& c) { rot(c, 64); c.fu.q_scale = 0.5f; });
    refuse("rot_q_cols_mod", [](GC& c) { rot(c, 64); c.fu.q_scale = 0.5f; c.fu.q_cols = 100; });
    refuse("rot_q_cols_large", [](GC& c) { rot(c, 64); c.fu.q_scale = 0.5f; c.fu.q_cols = c.fu.rot_cols + 64; });
    refuse("rot_q_cols+ln", [](GC& c) { rot(c, 64); c.fu.q_scale = 0.5f; ln(c); c.fu.ln_c1 = nullptr; });
    // LayerNorm fold
    refuse("ln_residual", [](GC& c) { residual(c); ln(c); });
    refuse("ln_residual+operands", [](GC& c) { residual(c); ln(c); c.fu.ln_c2 = nullptr; });
    refuse("ln_c1_null", [](GC& c) { ln(c); c.fu.ln_c1 = nullptr; });
    refuse("ln_c2_null", [](GC& c) { ln(c); c.fu.ln_c2 = nullptr; });
    refuse("ln_c1_align", [](GC& c) { ln(c); c.fu.ln_c1 = buf<float>("ln_c1", 8); });
    refuse("ln_c2_align", [](GC& c) { ln(c); c.fu.ln_c2 = buf<float>("ln_c2", 4); });
    refuse("ln_partial_align", [](GC& c) { ln(c); c.fu.ln_partial = buf<float>("ln_partial", 4); });
    refuse("ln_nblk", [](GC& c) { ln(c); c.fu.ln_nblk = 0; });
    refuse("ln_dim", [](GC& c) { ln(c); c.fu.ln_dim = 0; });
    refuse("ln_operands+vec", [](GC& c) { ln(c); c.fu.ln_dim = 0; c.C = buf("C", 8); });
    refuse("ln_vec", [](GC& c) { ln(c); c.C = buf("C", 8); });
    refuse("ln_N", [](GC& c) { ln(c); c.N = 770; c.ldc = 776; });
    refuse("ln_vec+stats_epilogue", [](GC& c) { ln(c); c.C = buf("C", 8); stats(c); });
    refuse("ln_qk_sumsq_align", [](GC& c) { f16(c); ln(c); rot(c, 64); c.fu.qk_sumsq = buf<uint32_t>("qk_sumsq", 2); });
    refuse("ln_qk_sumsq_align+stats", [](GC& c) { f16(c); ln(c); rot(c, 64); c.fu.qk_sumsq = buf<uint32_t>("qk_sumsq", 2); stats(c); });
    // row statistics
    refuse("stats_epilogue", [](GC& c) { stats(c); });
    refuse("stats_epilogue_gelu", [](GC& c) { c.epi = ESME_EPI_GELU; stats(c); c.fu.stats_out = buf<float>("stats_out", 4); });
    refuse("stats_N", [](GC& c) { residual(c); c.N = 800; stats(c); });
    refuse("stats_vec", [](GC& c) { residual(c); stats(c); c.resid = buf("resid", 8); });
    refuse("stats_vec+align", [](GC& c) { residual(c); stats(c); c.resid = buf("resid", 8); c.fu.stats_out = buf<float>("stats_out", 4); });
    refuse("stats_align", [](GC& c) { residual(c); stats(c); c.fu.stats_out = buf<float>("stats_out", 4); });
    refuse("stats_align+grid", [](GC& c) { residual(c); stats(c); c.fu.stats_out = buf<float>("stats_out", 4); c.M = 400000000; c.N = 128000; tile(c, 1); });
    // the launch
    refuse("grid_tile1", [](GC& c) { c.M = 400000000; c.N = 128000; tile(c, 1); });
    refuse("grid_tile2", [](GC& c) { c.M = 1600000000; c.N = 128000 * 4; tile(c, 2); });
    refuse("grid_colsplit", [](GC& c) { c.M = 1600000000; c.N = 128000 * 4 + 128; pair_stream_all(c); });
}

#else
// ================================================================ attention
struct AC {
    int entry = 0;                                        // 0 fwd, 1 _exact, 2 _opts, 3 _split, 4 _qkpair_f16_opts, 5 _qkpair_f16
    const void *q, *k, *v;
    void* o = buf("o");
    const int32_t* cu = buf<int32_t>("cu_lens");
    int64_t ld_qkv, ld_o, lo_in, lo_o, T = 1000;
    int B = 3, H = 4, d, max_len = 500;
    float scale = 0.125f;
    esme_attn_opts_t op{(int)sizeof(esme_attn_opts_t), 0, 0, 8.0f, 1, nullptr, 0, 0};
    bool use_op = false;
    const int32_t* order = nullptr;                       // entries 3 and 5
    AC(int entry_, int d_, int H_ = 4) : entry(entry_), H(H_), d(d_) {
        const int64_t E = (int64_t)H * d;
        const bool pair = entry >= 3;                     // [hi | lo] rows: q, k, v of each half side by side
        q = buf("qkv"); k = buf("qkv", 2 * E); v = buf("qkv", 4 * E);
        ld_qkv = (pair ? 6 : 3) * E; lo_in = 3 * E;
        ld_o = entry == 3 ? 2 * E : E; lo_o = E;
        use_op = entry == 2 || entry == 4;
    }
};

int call(const AC& c) {
    void* st = buf("stream");
    const esme_attn_opts_t* op = c.use_op ? &c.op : nullptr;
    int rc;
    switch (c.entry) {
        case 0: rc = esme_hip_attn_varlen_fwd(c.q, c.k, c.v, c.ld_qkv, c.o, c.ld_o, c.cu, c.B, c.T, c.H, c.d, c.max_len, c.scale, st); break;
        case 1: rc = esme_hip_attn_varlen_fwd_exact(c.q, c.k, c.v, c.ld_qkv, c.o, c.ld_o, c.cu, c.B, c.T, c.H, c.d, c.max_len, c.scale, st); break;
        case 2: rc = esme_hip_attn_varlen_fwd_opts(c.q, c.k, c.v, c.ld_qkv, c.o, c.ld_o, c.cu, c.B, c.T, c.H, c.d, c.max_len, c.scale, op, st); break;
        case 3: rc = esme_hip_attn_varlen_fwd_split(c.q, c.k, c.v, c.ld_qkv, c.lo_in, c.o, c.ld_o, c.lo_o, c.cu, c.B, c.T, c.H, c.d, c.max_len, c.scale, c.order, st); break;
        case 4: rc = esme_hip_attn_varlen_fwd_qkpair_f16_opts(c.q, c.k, c.v, c.ld_qkv, c.lo_in, c.o, c.ld_o, c.cu, c.B, c.T, c.H, c.d, c.max_len, c.scale, op, st); break;
        default: rc = esme_hip_attn_varlen_fwd_qkpair_f16(c.q, c.k, c.v, c.ld_qkv, c.lo_in, c.o, c.ld_o, c.cu, c.B, c.T, c.H, c.d, c.max_len, c.scale, c.order, st); break;
    }
    rc_line(rc);
    return rc;
}

const int kDims[] = {16, 32, 64, 128, 48};
const int kLens[] = {50, 191, 192, 500};
const char* kEntry[] = {"fwd", "exact", "opts", "split", "qkpair_opts", "qkpair"};

void set_order(AC& c) { c.order = buf<int32_t>("seq_order"); c.op.seq_order = c.order; }

void refuse(const std::string& name, int entry, std::function<void(AC&)> f, int d = 64, int H = 4) {
    add(std::string("attn_refuse_") + kEntry[entry] + "_" + name, [=] { AC c(entry, d, H); f(c); call(c); });
}

void cases() {
    for (int e : {0, 1, 3, 5})
        add(std::string("attn_") + kEntry[e] + "_plain", [e] {
            for (int d : kDims) for (int L : kLens) { AC c(e, d); c.max_len = L; call(c); }
        });
    add("attn_opts_null", [] { for (int d : kDims) for (int L : kLens) { AC c(2, d); c.use_op = false; c.max_len = L; call(c); } });
    for (int var : {0, 1, 2, 4, 8})
        for (int f16 = 0; f16 <= 1; ++f16)
            for (int qp = 0; qp <= 1; ++qp)
                add("attn_opts_v" + std::to_string(var) + (f16 ? "_f16" : "") + (qp ? "_qp" : ""), [=] {
                    for (int d : kDims)
                        for (int L : kLens)
                            for (int qb = 0; qb <= 2; ++qb) {
                                if (qb && L != 50 && L != 192) continue;
                                AC c(2, d); c.max_len = L; c.op.variant = var; c.op.f16 = f16; c.op.q_prescaled = qp; c.op.q_blocks = qb;
                                call(c);
                            }
                });
    add("attn_opts_thr_spec", [] {
        for (int var : {0, 1, 2, 8})
            for (int d : {32, 64, 128}) {
                AC c(2, d); c.op.variant = var; c.op.defer_max_thr = 3.5f; c.op.speculative = 0; call(c);
                AC x(2, d); x.op.variant = var; x.op.defer_max_thr = 0.f; x.op.speculative = 2; x.op.f16 = 1; call(x);
            }
    });
    // what keeps a call off the pipelined kernels: ld_o % 8, a 16-byte misaligned o, 32-bit byte offsets; and the generic kernels' own limit
    for (int f16 = 0; f16 <= 1; ++f16)
        for (int qp = 0; qp <= 1; ++qp)
            add(std::string("attn_not_pipelined") + (f16 ? "_f16" : "") + (qp ? "_qp" : ""), [=] {
                for (int var : {0, 1, 2, 4, 8})
                    for (int d : {16, 32, 64, 128})
                        for (int why = 0; why < 4; ++why) {
                            AC c(2, d); c.op.variant = var; c.op.f16 = f16; c.op.q_prescaled = qp;
                            if (why == 0) c.ld_o = c.H * d + 4;
                            if (why == 1) c.o = buf("o", 8);
                            if (why == 2) { c.ld_qkv = 1 << 21; c.max_len = 1000; }       // fails fits32 only
                            if (why == 3) { c.ld_qkv = 1 << 22; c.max_len = 1000; }       // fails the generic kernels' 2^32-element limit too
                            call(c);
                        }
            });
    add("attn_stride_limits_pair_entries", [] {
        for (int e : {3, 4, 5})
            for (int var : {0, 2})
                for (int d : {16, 32, 64, 128})
                    for (int sh : {21, 22, 25}) {
                        if (var && e != 4) continue;
                        AC c(e, d); c.op.variant = var; c.ld_qkv = 1LL << sh; c.max_len = sh == 25 ? 100 : 1000; call(c);
                    }
        for (int d : {32, 64}) {
            { AC c(4, d); c.op.variant = 2; c.ld_o = c.H * d + 4; call(c); }
            { AC c(4, d); c.op.variant = 2; c.o = buf("o", 8); call(c); }
        }
    });
    for (int ord = 0; ord <= 1; ++ord)
        add(std::string("attn_many_sequences") + (ord ? "_order" : ""), [ord] {
            for (int B : {65535, 65536, 70000, 131071}) {
                for (int var : {0, 1, 2})
                    for (int d : {16, 64, 128}) {
                        AC c(2, d); c.B = B; c.T = 2LL * B; c.max_len = 60; c.op.variant = var; if (ord) set_order(c);
                        call(c);
                    }
                for (int e : {0, 3, 4, 5}) { AC c(e, 32); c.B = B; c.T = 2LL * B; c.max_len = 200; if (ord) set_order(c); call(c); }
                { AC c(4, 64); c.B = B; c.op.variant = 2; if (ord) set_order(c); call(c); }
            }
        });
    add("attn_seq_order", [] {
        for (int e : {2, 3, 4, 5})
            for (int d : {16, 32, 64, 128})
                for (int var : {0, 1, 2}) {
                    if (var && e != 2 && e != 4) continue;
                    AC c(e, d); c.op.variant = var; set_order(c); call(c);
                }
    });
    add("attn_empty", [] {
        for (int e = 0; e < 6; ++e) {
            { AC c(e, 64); c.B = 0; call(c); }
            { AC c(e, 64); c.T = 0; call(c); }
            { AC c(e, 48); c.T = 0; c.q = nullptr; c.ld_qkv = 3; c.max_len = 0; call(c); }     // empty returns before every later check
        }
    });
    add("attn_shapes", [] {
        for (int e = 0; e < 6; ++e)
            for (int d : {16, 32, 64, 128}) {
                if (d == 128 && e >= 4) continue;
                { AC c(e, d, 20); c.B = 1; c.max_len = 1; c.T = 1; c.scale = 0.25f; call(c); }
                { AC c(e, d, 33); c.B = 1025; c.max_len = 4097; c.T = 50000; call(c); }
                { AC c(e, d, 65535); c.B = 2; c.max_len = 129; call(c); }
            }
    });
    add("attn_qkpair_opts", [] {
        for (int var : {0, 1, 2, 4})
            for (int d : {16, 32, 64, 128, 48})
                for (int L : {50, 500}) { AC c(4, d); c.op.variant = var; c.max_len = L; call(c); }
        { AC c(4, 64); c.use_op = false; call(c); }
    });

    // ---- refusals; "a+b" violates both (the golden fixes which message wins)
    for (int e = 0; e < 6; ++e) {
        if (e == 2 || e == 4) {
            refuse("opts_abi", e, [](AC& c) { c.op.struct_bytes += 8; });
            refuse("opts_abi+sizes", e, [](AC& c) { c.op.struct_bytes = 0; c.H = 0; });
        }
        refuse("sizes_B", e, [](AC& c) { c.B = -1; });
        refuse("sizes_T", e, [](AC& c) { c.T = -1; });
        refuse("sizes_H", e, [](AC& c) { c.H = 0; });
        refuse("sizes_d", e, [](AC& c) { c.d = 0; });
        refuse("sizes_max_len", e, [](AC& c) { c.max_len = -1; });
        refuse("sizes+null", e, [](AC& c) { c.d = -64; c.q = nullptr; });
        refuse("null_q", e, [](AC& c) { c.q = nullptr; });
        refuse("null_k", e, [](AC& c) { c.k = nullptr; });
        refuse("null_v", e, [](AC& c) { c.v = nullptr; });
        refuse("null_o", e, [](AC& c) { c.o = nullptr; });
        refuse("null_cu", e, [](AC& c) { c.cu = nullptr; });
        refuse("null+strides", e, [](AC& c) { c.cu = nullptr; c.ld_qkv = 12; });
        refuse("ld_qkv_mod8", e, [](AC& c) { c.ld_qkv += 4; });
        refuse("ld_o_mod4", e, [](AC& c) { c.ld_o += 2; });
        refuse("ld_o_small", e, [](AC& c) { c.ld_o -= 4; });
        if (e < 3) refuse("ld_qkv_small", e, [](AC& c) { c.ld_qkv = c.H * c.d - 8; });
        if (e >= 3) {
            refuse("lo_in_mod8", e, [](AC& c) { c.lo_in += 4; });
            refuse("lo_in_zero", e, [](AC& c) { c.lo_in = 0; });
            refuse("lo_in_neg", e, [](AC& c) { c.lo_in = -8; });
        }
        if (e == 3) {
            refuse("lo_o_mod4", e, [](AC& c) { c.lo_o += 2; c.ld_o += 8; });
            refuse("lo_o_small", e, [](AC& c) { c.lo_o -= 4; });
        }
        refuse("strides+misaligned", e, [](AC& c) { c.ld_o -= 4; c.k = buf("qkv", 8); });
        refuse("misaligned_q", e, [](AC& c) { c.q = buf("qkv", 8); });
        refuse("misaligned_k", e, [](AC& c) { c.k = buf("qkv", 8); });
        refuse("misaligned_v", e, [](AC& c) { c.v = buf("qkv", 4); });
        refuse("misaligned_o", e, [](AC& c) { c.o = buf("o", 4); });
        refuse("misaligned+max_len", e, [](AC& c) { c.o = buf("o", 4); c.max_len = 0; });
        refuse("max_len_zero", e, [](AC& c) { c.max_len = 0; });
        refuse("H_65536", e, [](AC& c) { c.H = 65536; c.ld_qkv *= 16384; c.ld_o *= 16384; c.lo_in *= 16384; c.lo_o *= 16384; });
        refuse("max_len+head_dim", e, [](AC& c) { c.max_len = 0; }, 48);
        refuse("head_dim_48", e, [](AC& c) {}, 48);
        refuse("head_dim_8", e, [](AC& c) {}, 8);
        refuse("head_dim_256", e, [](AC& c) {}, 256);
        if (e >= 4) refuse("head_dim_128", e, [](AC& c) {}, 128);
        refuse("head_dim+stride_limit", e, [](AC& c) { c.ld_qkv = 1 << 22; c.max_len = 1000; }, 48);
        refuse("stride_limit", e, [](AC& c) { c.ld_qkv = 1 << 22; c.max_len = 1000; }, 16);
        refuse("stride_limit_two_blocks", e, [](AC& c) { c.ld_qkv = 1 << 23; c.max_len = 300; }, 16);        // (300 + 128) rows pass, (300 + 256) do not
        refuse("stride_limit+order", e, [](AC& c) { c.ld_qkv = 1 << 22; c.max_len = 1000; c.B = 70000; set_order(c); }, 16);
        if (e >= 2) refuse("order_many_sequences", e, [](AC& c) { c.B = 65536; set_order(c); }, 16);
    }
    refuse("f16_qp_d16", 2, [](AC& c) { c.op.f16 = c.op.q_prescaled = 1; }, 16);
    refuse("f16_qp_d128", 2, [](AC& c) { c.op.f16 = c.op.q_prescaled = 1; }, 128);
    refuse("f16_qp_d48", 2, [](AC& c) { c.op.f16 = c.op.q_prescaled = 1; }, 48);
    refuse("f16_qp_ld_o", 2, [](AC& c) { c.op.f16 = c.op.q_prescaled = 1; c.ld_o += 4; });
    refuse("f16_qp_o_align", 2, [](AC& c) { c.op.f16 = c.op.q_prescaled = 1; c.o = buf("o", 8); }, 32);
    refuse("f16_qp_v1_ld_o", 2, [](AC& c) { c.op.f16 = c.op.q_prescaled = 1; c.op.variant = 1; c.ld_o += 4; });
    refuse("f16_qp+stride_limit", 2, [](AC& c) { c.op.f16 = c.op.q_prescaled = 1; c.ld_qkv = 1 << 22; c.max_len = 1000; }, 16);
    refuse("f16_qp_stride_limit", 2, [](AC& c) { c.op.f16 = c.op.q_prescaled = 1; c.ld_qkv = 1 << 22; c.max_len = 1000; });
    refuse("f16_qp_order_many_sequences", 2, [](AC& c) { c.op.f16 = c.op.q_prescaled = 1; c.op.variant = 1; c.B = 65536; set_order(c); });
    // the pipelined kernels' one-dimensional grid: query tiles x (H * B rounded up to 8)
    auto big = [](AC& c, int B) { c.B = B; c.max_len = 100000; c.ld_qkv = (int64_t)c.H * c.d; c.k = buf("k"); c.v = buf("v"); };
    refuse("grid_pp", 2, [=](AC& c) { big(c, 20000); }, 64, 300);
    refuse("grid_pp8", 2, [=](AC& c) { big(c, 40000); c.op.variant = 8; }, 64, 300);
    refuse("grid_pp_d32_f16", 2, [=](AC& c) { big(c, 10000); c.op.f16 = 1; }, 32, 600);
    refuse("grid_sb", 2, [=](AC& c) { big(c, 5000); c.op.variant = 2; }, 32, 600);
    refuse("grid_sb_qkpair", 4, [=](AC& c) { big(c, 10000); c.op.variant = 2; }, 64, 300);
}
#endif

}  // namespace kll

#ifdef ESME_KLL_GEMM
// --cases FILE: one call per line, "form M N K tile persist raster_gm raster_gn device" (form: a name of kForms; tile 0 / 1 / 2; persist -1 / 0 / 1;
// device: the ordinal hipGetDevice answers -- 0, 1, 2 = 256, 4, 300 compute units; '#' opens a comment).  Prints "== line<N> <launches>" and the
// call's log, as the table's cases are printed.  tests/test_gemm_path_cpu.py pins tests/gemm_path.py (which kernel a call runs) with it.
static int run_case_file(const char* path) {
    using namespace kll;
    FILE* f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    char line[512], form[64];
    for (int no = 1; fgets(line, sizeof line, f); ++no) {
        if (line[0] == '#' || line[0] == '\n') continue;
        ll M;
        int N, K, t, persist, gm, gn, dev;
        if (sscanf(line, "%63s %lld %d %d %d %d %d %d %d", form, &M, &N, &K, &t, &persist, &gm, &gn, &dev) != 9 || t < 0 || t > 2 || dev < 0 || dev > 2) {
            fprintf(stderr, "%s:%d: want 'form M N K tile persist raster_gm raster_gn device'\n", path, no); fclose(f); return 2;
        }
        const Form* fm = nullptr;
        for (const Form& k : kForms) if (!strcmp(k.name, form)) fm = &k;
        if (!fm) { fprintf(stderr, "%s:%d: no form %s\n", path, no, form); fclose(f); return 2; }
        g_names.clear(); g_log.clear(); g_launches = 0;
        esme::error_buffer()[0] = 0;
        GC c; c.dev = dev; c.M = M; c.N = N; c.K = K; fm->set(c);
        tile(c, t); c.op.persist = persist; c.op.raster_gm = gm; c.op.raster_gn = gn;
        call(c);
        printf("== line%d %d\n", no, g_launches);
        fputs(g_log.c_str(), stdout);
    }
    fclose(f);
    return 0;
}
#endif

int main(int argc, char** argv) {
    using namespace kll;
#ifdef ESME_KLL_GEMM
    if (argc == 3 && !strcmp(argv[1], "--cases")) return run_case_file(argv[2]);
#endif
    const char* only = argc == 3 && !strcmp(argv[1], "--dump") ? argv[2] : nullptr;
    if (argc != 1 && !only) { fprintf(stderr, "usage: %s [--dump CASE]\n", argv[0]); return 2; }
    cases();
    bool found = false;
    for (const auto& c : g_cases) {                          // every case runs (the dynamic-LDS set depends on all of them); --dump prints one
        g_names.clear(); g_log.clear(); g_launches = 0; g_dev = 0;
        esme::error_buffer()[0] = 0;
        c.second();
        if (only && c.first != only) continue;
        found = true;
        if (!only) printf("== %s %d\n", c.first.c_str(), g_launches);
        fputs(g_log.c_str(), stdout);
    }
    // the dynamic-LDS opt-ins happen once per kernel and device, so which case makes them depends on the order of the cases: one case of their own
    if (!only || !strcmp(only, "dynamic_lds")) {
        found = true;
        if (!only) printf("== dynamic_lds %zu\n", g_lds.size());
        for (const auto& kb : g_lds) printf("lds %s bytes=%d\n", kb.first.c_str(), kb.second);
    }
    if (!found) { fprintf(stderr, "no case %s\n", only); return 2; }
    return 0;
}
