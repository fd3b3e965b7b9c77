// Error string, ABI version, the stage records (which kernel each stage launched last) and the event profiler.
#include <atomic>
#include <mutex>

#include "pipeline.hpp"

namespace evc {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// Optional in-stream timing of the two streaming kernels (bench.py's roofline leg): hipEvents are
// recorded on the launch stream right before/after the kernel, so the figure is the kernel's own
// duration inside the real per-geometry DAG.  Process-wide, off by default.
// Stages: EVC_PROF_* of include/evcont_hip.h.
static char g_kernel_ran[kProfStages][kKernelRanLen];
void note_kernel(int stage, const char *fmt, ...) {
    if (stage < 0 || stage >= kProfStages) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_kernel_ran[stage], sizeof(g_kernel_ran[stage]), fmt, ap);
    va_end(ap);
}
const char *kernel_ran(int stage) { return (stage >= 0 && stage < kProfStages) ? g_kernel_ran[stage] : ""; }
void clear_kernels(unsigned mask) {
    for (int s = 0; s < kProfStages; ++s)
        if (mask >> s & 1u) g_kernel_ran[s][0] = '\0';
}
void clear_fci_kernels(int stage) { clear_kernels((1u << EVC_PROF_FCI_EXCITE) | (1u << stage)); }
constexpr int kProfPerSample = 16;   // event pairs one evaluation can record
struct Prof {
    std::atomic<bool> on{false};
    int cap = 0, n = 0;          // records: capacity, used
    hipEvent_t *ev = nullptr;    // [cap][2]: start, stop
    int *stage = nullptr;        // [cap]
    double ms[kProfStages] = {0};   // results of the last evc_profile_end
    int cnt[kProfStages] = {0};
    unsigned mask = (1u << EVC_PROF_ROWS) | (1u << EVC_PROF_COLS);   // stages that are timed (evc_profile_select)
};
static Prof g_prof;
static std::mutex g_prof_mu;   // record allocation and begin/end/select: host threads may share the hook
// start of a timed launch: returns the record index or -1
int prof_start(int stage, hipStream_t st) {
    if (!g_prof.on || stage < 0) return -1;   // the common case: no lock taken
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (!g_prof.on || !(g_prof.mask >> stage & 1u) || g_prof.n >= g_prof.cap) return -1;
    const int i = g_prof.n++;
    g_prof.stage[i] = stage;
    (void)hipEventRecord(g_prof.ev[2 * i], st);
    return i;
}
void prof_stop(int i, hipStream_t st) {
    if (i >= 0) (void)hipEventRecord(g_prof.ev[2 * i + 1], st);
}

}  // namespace evc

using namespace evc;

extern "C" int evc_abi_version(void) { return EVC_ABI_VERSION; }
extern "C" const char *evc_last_error(void) { return g_err; }

extern "C" int evc_profile_begin(int max_samples) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    EVC_REQUIRE(!g_prof.on, "evc_profile_begin: already profiling");
    EVC_REQUIRE(max_samples > 0 && max_samples <= 1 << 16, "evc_profile_begin: max_samples=%d", max_samples);
    const int cap = max_samples * kProfPerSample;
    g_prof.ev = new hipEvent_t[2 * (size_t)cap];
    g_prof.stage = new int[cap];
    for (int i = 0; i < 2 * cap; ++i) {
        hipError_t e = hipEventCreate(&g_prof.ev[i]);
        if (e != hipSuccess) {
            set_error("evc_profile_begin: hipEventCreate: %s", hipGetErrorString(e));
            return (int)e;
        }
    }
    g_prof.cap = cap;
    g_prof.n = 0;
    g_prof.on = true;
    return 0;
}

extern "C" int evc_profile_end(double *rows_ms, int *rows_n, double *cols_ms, int *cols_n) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    EVC_REQUIRE(g_prof.on, "evc_profile_end: not profiling");
    for (int k = 0; k < kProfStages; ++k) {
        g_prof.ms[k] = 0.0;
        g_prof.cnt[k] = 0;
    }
    for (int i = 0; i < g_prof.n; ++i) {
        float ms = 0.f;
        (void)hipEventSynchronize(g_prof.ev[2 * i + 1]);
        (void)hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]);
        const int k = g_prof.stage[i];
        g_prof.ms[k] += ms;
        g_prof.cnt[k] += 1;
    }
    if (rows_ms) *rows_ms = g_prof.ms[EVC_PROF_ROWS];
    if (rows_n) *rows_n = g_prof.cnt[EVC_PROF_ROWS];
    if (cols_ms) *cols_ms = g_prof.ms[EVC_PROF_COLS];
    if (cols_n) *cols_n = g_prof.cnt[EVC_PROF_COLS];
    for (int i = 0; i < 2 * g_prof.cap; ++i) (void)hipEventDestroy(g_prof.ev[i]);
    delete[] g_prof.ev;
    delete[] g_prof.stage;
    g_prof.ev = nullptr;
    g_prof.stage = nullptr;
    g_prof.cap = g_prof.n = 0;
    g_prof.on = false;
    return 0;
}

extern "C" const char *evc_profile_kernel(int stage) { return kernel_ran(stage); }

extern "C" int evc_profile_select(unsigned stage_mask) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    EVC_REQUIRE(!g_prof.on, "evc_profile_select: not while profiling");
    g_prof.mask = stage_mask & ((1u << kProfStages) - 1u);
    return 0;
}

extern "C" int evc_profile_stage(int stage, double *ms, int *launches) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    EVC_REQUIRE(stage >= 0 && stage < kProfStages, "evc_profile_stage: stage=%d", stage);
    EVC_REQUIRE(!g_prof.on, "evc_profile_stage: call evc_profile_end first");
    if (ms) *ms = g_prof.ms[stage];
    if (launches) *launches = g_prof.cnt[stage];
    return 0;
}
