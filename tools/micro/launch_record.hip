// Records what the orchestration of a source tree WOULD enqueue, without a GPU: dispatch_record.hip's idea carried from the
// K5 / K8 files to all of csrc.  Every csrc source is compiled with launch_record_shim.h force-included, which turns every
// kernel launch, copy, memset, event and stream call into a record; this driver calls the extern "C" entry points with
// fixed fake pointers for the rows of CASES in tests/dispatch_table.py (tools/micro/launch_record_cases.py prints them).
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -w -ftrivial-auto-var-init=zero -include launch_record_shim.h \
//         -I$TREE/include -I$TREE/evcont_amd/csrc launch_record.hip $TREE/evcont_amd/csrc/*.hip -rdynamic -ldl -o launch_record
//   python launch_record_cases.py ./launch_record > records.txt     (CASES, then each row of KNOB_CASES in its own process)
// A record line: stream (main / side), kernel instantiation, grid, block, dynamic LDS and a hash of the bytes of every
// by-value argument (-ftrivial-auto-var-init=zero: struct padding compares equal); copies and events with their operands.
// Two trees enqueue alike if their outputs are equal, line for line.
#include <cxxabi.h>
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "evcont_hip.h"

int g_shim_cus = 256;
static const hipStream_t kMain = (hipStream_t)0x5717000, kSide = (hipStream_t)0x51de000;
static long g_launches = 0, g_calls = 0;
static uintptr_t g_next_event = 0xe0000;

static const char *stream_name(hipStream_t st) {
    static char buf[32];
    if (st == kMain) return "main";
    if (st == kSide) return "side";
    snprintf(buf, sizeof buf, "%p", (void *)st);
    return buf;
}
void shim_record_launch(const char *pretty, const void *stub, dim3 g, dim3 b, size_t lds, hipStream_t st, uint64_t h) {
    const char *k = strstr(pretty, "K = ");   // "... [K = &evc::name]": without the template arguments
    std::string name = k ? k + 4 : pretty;
    if (!name.empty() && name.back() == ']') name.pop_back();
    // the instantiation from the host stub's symbol (-rdynamic); a kernel with internal linkage keeps the name above
    Dl_info info;
    if (dladdr(stub, &info) && info.dli_sname && info.dli_saddr == stub) {
        int status = 0;
        char *d = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &status);
        if (status == 0 && d) {
            name = d;
            const size_t paren = name.find('(');
            if (paren != std::string::npos) name.resize(paren);
        }
        free(d);
    }
    printf("L %s %s grid=%u,%u,%u block=%u,%u,%u lds=%zu args=%016llx\n", stream_name(st), name.c_str(), g.x, g.y, g.z, b.x,
           b.y, b.z, lds, (unsigned long long)h);
    ++g_launches;
}
void shim_record_call(const char *what, hipStream_t st, const char *fmt, ...) {
    printf("C %s %s ", stream_name(st), what);
    va_list ap;
    va_start(ap, fmt);
    vprintf(fmt, ap);
    va_end(ap);
    printf("\n");
    ++g_calls;
}
hipError_t shim_hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
    shim_record_call("memcpy", st, "dst=%p src=%p bytes=%zu kind=%d", dst, src, bytes, (int)kind);
    return hipSuccess;
}
hipError_t shim_hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height,
                                 hipMemcpyKind kind, hipStream_t st) {
    shim_record_call("memcpy2d", st, "dst=%p dpitch=%zu src=%p spitch=%zu width=%zu height=%zu kind=%d", dst, dpitch, src,
                     spitch, width, height, (int)kind);
    return hipSuccess;
}
hipError_t shim_hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t st) {
    shim_record_call("memset", st, "dst=%p value=%d bytes=%zu", dst, value, bytes);
    return hipSuccess;
}
hipError_t shim_hipEventRecord(hipEvent_t e, hipStream_t st) {
    shim_record_call("event_record", st, "event=%p", (void *)e);
    return hipSuccess;
}
hipError_t shim_hipStreamWaitEvent(hipStream_t st, hipEvent_t e, unsigned flags) {
    shim_record_call("wait_event", st, "event=%p flags=%u", (void *)e, flags);
    return hipSuccess;
}
hipError_t shim_hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) {
    *e = (hipEvent_t)(g_next_event += 0x10);
    shim_record_call("event_create", nullptr, "event=%p flags=%u", (void *)*e, flags);
    return hipSuccess;
}
hipError_t shim_hipEventSynchronize(hipEvent_t e) {
    shim_record_call("event_sync", nullptr, "event=%p", (void *)e);
    return hipSuccess;
}
hipError_t shim_hipEventDestroy(hipEvent_t e) {
    shim_record_call("event_destroy", nullptr, "event=%p", (void *)e);
    return hipSuccess;
}
hipError_t shim_hipStreamCreateWithFlags(hipStream_t *s, unsigned flags) {
    *s = kSide;
    shim_record_call("stream_create", kSide, "flags=%u", flags);
    return hipSuccess;
}
hipError_t shim_hipStreamDestroy(hipStream_t s) {
    shim_record_call("stream_destroy", s, "");
    return hipSuccess;
}

static double *fake(uintptr_t k) { return (double *)(0x100000000ull * k); }   // 4 GiB apart, 16-byte aligned

static void report(const char *what, int rc) {
    if (rc)
        printf("RC %s = %d: %s\n", what, rc, evc_last_error());
    else
        printf("RC %s = 0\n", what);
    printf("STAGES");
    for (int s = 0; s < 8; ++s) printf(" | %s", evc_profile_kernel(s));
    printf("\n");
}

// case line: id n T A G layout packed energy_only warm nroots api keep npairs k l k l ...
int main() {
    char id[128], api[32];
    int n, T, A, G, layout, packed, energy_only, warm, nroots, keep, npairs, ncases = 0;
    while (scanf("%127s %d %d %d %d %d %d %d %d %d %31s %d %d", id, &n, &T, &A, &G, &layout, &packed, &energy_only, &warm,
                 &nroots, api, &keep, &npairs) == 13) {
        std::vector<int32_t> pairs(2 * (size_t)npairs);
        for (int i = 0; i < 2 * npairs; ++i)
            if (scanf("%d", &pairs[i]) != 1) return 2;
        printf("CASE %s\n", id);
        ++ncases;
        const int64_t n2 = (int64_t)n * n, ns = (int64_t)n * (n + 1) / 2;
        const bool tri = layout == 5 || layout == 2 || layout == 8;
        evc_trdm_set t;
        memset(&t, 0, sizeof t);
        t.n = n;
        t.ntrain = T;
        t.layout = layout;
        t.cols2 = layout == 8 ? ns * (ns + 1) / 2 : (layout == 3 || layout == 2) ? n2 * (n2 + 1) / 2 : n2 * n2;
        t.rows2 = t.rows2_total = tri ? (int64_t)T * (T + 1) / 2 : (int64_t)T * T;
        t.ld2 = (t.cols2 + 15) / 16 * 16;
        t.ld1 = (n2 + 1) / 2 * 2;
        t.two_rdm = fake(1);
        t.one_rdm = fake(2);
        t.s_train = fake(3);
        const bool single = !strcmp(api, "single") || !strcmp(api, "roots");
        const bool roots = !strncmp(api, "roots", 5);
        evc_geometry g1;
        memset(&g1, 0, sizeof g1);
        g1.natm = A;
        g1.enuc = 1.25;
        g1.S = fake(4);
        g1.hcore = fake(5);
        g1.eri = fake(6);
        g1.ipovlp = fake(7);
        g1.dhcore = fake(8);
        g1.eri_ip1 = fake(9);
        g1.gnuc = fake(10);
        g1.aoslices = (const int64_t *)fake(11);
        evc_geometry_batch gb;
        memset(&gb, 0, sizeof gb);
        gb.natm = A;
        gb.count = G;
        gb.enuc = fake(12);
        gb.S = g1.S;
        gb.hcore = g1.hcore;
        gb.eri = g1.eri;
        gb.ipovlp = g1.ipovlp;
        gb.dhcore = g1.dhcore;
        gb.eri_ip1 = g1.eri_ip1;
        gb.gnuc = g1.gnuc;
        gb.aoslices = g1.aoslices;
        evc_outputs o1 = {fake(13), fake(14), fake(15), keep ? fake(16) : nullptr, keep ? fake(17) : nullptr, nullptr};
        evc_outputs_batch ob = {o1.energy, o1.coeffs, o1.grad, o1.d_pred, o1.g_pred, nullptr};
        evc_outputs_roots orr = {o1.grad, o1.d_pred, o1.g_pred};
        void *ws = fake(32);
        const size_t bytes = !roots    ? evc_workspace_bytes_batch(&t, A, G)
                             : single ? evc_workspace_bytes_roots(&t, A, npairs)
                                      : evc_workspace_bytes_roots_batch(&t, A, G, npairs);
        printf("WS %zu\n", bytes);
        const int fpacked = packed ? (EVC_FLAG_ERI_S4 | EVC_FLAG_IP1_S2KL) : 0;
        auto full = [&](int flags) {
            return single ? evc_energy_with_grad(&t, &g1, &o1, nroots, flags, ws, bytes, kMain)
                          : evc_energy_with_grad_batch(&t, &gb, &ob, nroots, flags, ws, bytes, kMain);
        };
        if (roots) {
            report("energy_only", full(fpacked | EVC_FLAG_ENERGY_ONLY));
            const int fl = packed ? EVC_FLAG_IP1_S2KL : 0;
            report("gradient_roots",
                   single ? evc_phase_gradient_roots(&t, &g1, o1.coeffs, nroots, pairs.data(), npairs, &orr, fl, ws, bytes, kMain)
                          : evc_phase_gradient_roots_batch(&t, &gb, o1.coeffs, nroots, pairs.data(), npairs, &orr, fl, ws,
                                                           bytes, kMain));
        } else if (energy_only) {
            report("energy_only", full(fpacked | EVC_FLAG_ENERGY_ONLY));
            const int fl = packed ? EVC_FLAG_IP1_S2KL : 0;
            report("phase_gradient", single ? evc_phase_gradient(&t, &g1, &o1, fl, ws, bytes, kMain)
                                            : evc_phase_gradient_batch(&t, &gb, &ob, fl, ws, bytes, kMain));
        } else {
            report("full", full(fpacked));
            if (warm) report("full_warm", full(fpacked | EVC_FLAG_WARM_START));
        }
        report("release", evc_release_workspace(ws));
    }
    printf("TOTAL cases=%d launches=%ld copies_and_events=%ld\n", ncases, g_launches, g_calls);
    return 0;
}
