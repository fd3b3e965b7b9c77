// Records what launch_gemv_rows / launch_gemv_cols of a source tree WOULD launch, without a GPU: the tree's K5 / K8 files
// are compiled with dispatch_record_shim.h force-included, which turns every kernel launch and HIP query into a record.
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -w -include dispatch_record_shim.h -I$TREE/evcont_amd/csrc \
//         dispatch_record.hip $TREE/evcont_amd/csrc/gemv_{dispatch,stream,mfma,lds}.hip -o dispatch_record
//   ./dispatch_record CUS golden|detail < cases      case line: rows2 cols2 ld2 T n ld1 count wt part
// "golden" prints the lines of evc_trdm_plan_describe, "detail" adds grid, dynamic LDS, spans and the block bookkeeping.
// tests/golden/trdm_plan.json was recorded from the last commit before gemv_dispatch.hip existed (-DPRE_PLAN_TREE, without
// gemv_dispatch.hip on the command line: that tree's replan() is copied below); tests/golden/make_trdm_plan.py drives it.
// Two trees decide alike if their "detail" outputs are equal.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"

int g_shim_cus = 256;
static bool g_detail = false;
static const double *const kA2 = (const double *)0x10000, *const kA1 = (const double *)0x50000;

struct Pending {
    bool live = false, rows = false, cols = false;
    std::string k;
    unsigned grid[3], block[3];
    size_t lds;
    std::vector<int> ints;
    evc::GemvRowsLaunch R;
    evc::GemvColsLaunch C;
    evc::ColProblem CP;
    bool have_cp = false;
} g_p;
static bool g_skip_note = false;

static void emit(const char *name) {
    Pending &p = g_p;
    int g0 = 0, G = 0;
    const bool is_rows = strncmp(name, "gemv_rows", 9) == 0;
    if (!strncmp(name, "gemv_rows_kernel", 16) || !strncmp(name, "gemv_rows_wr_kernel", 19)) {
        g0 = p.ints.at(0);
        G = atoi(strstr(name, "G=") + 2);
    } else if (!strncmp(name, "gemv_cols_kernel", 16) || !strncmp(name, "gemv_cols_rs_kernel", 19)) {
        g0 = p.ints.at(0);
        G = atoi(strchr(name, '<') + 1);
    } else if (!strcmp(name, "gemv_cols_slab_kernel")) {
        g0 = 0;
        G = p.ints.at(0);
    } else {
        g0 = p.ints.at(p.ints.size() - 2);
        G = p.ints.at(p.ints.size() - 1);
    }
    if (is_rows) {
        int ns[2] = {0, 0};
        long long sc[2] = {0, 0};
        for (int k = 0; k < 2; ++k)
            if (p.R.p[k].nblocks) {
                const int which = p.R.p[k].A == kA2 ? 0 : 1;
                ns[which] = p.R.p[k].nspans;
                sc[which] = (long long)p.R.p[k].span_cols;
            }
        printf("K5 g0=%d G=%d %s nspans=%d,%d", g0, G, name, ns[0], ns[1]);
        if (g_detail) {
            printf(" | grid=%u block=%u lds=%zu span_cols=%lld,%lld", p.grid[0], p.block[0], p.lds, sc[0], sc[1]);
            const bool mc = strstr(name, "mfma") || strstr(name, "lds");
            printf(" slot0=%s slot1=%s", p.R.p[0].nblocks ? (p.R.p[0].A == kA2 ? "big" : "small") : "-",
                   p.R.p[1].nblocks ? (p.R.p[1].A == kA2 ? "big" : "small") : "-");
            printf(" nblk0=%d", p.R.nblk0);
            if (mc)
                printf(" nblk1=%d nrg=%d,%d tpg=%d,%d trem=%d,%d nsp=%d,%d", p.R.nblk1, p.R.nrg[0], p.R.nrg[1], p.R.tpg[0],
                       p.R.tpg[1], p.R.trem[0], p.R.trem[1], p.R.p[0].nspans, p.R.p[1].nspans);
            else
                printf(" nb=%d,%d", p.R.p[0].nblocks, p.R.p[1].nblocks);
        }
    } else {
        printf("K8 g0=%d G=%d %s", g0, G, name);
        if (g_detail) {
            printf(" | grid=%u,%u block=%u lds=%zu ints=", p.grid[0], p.grid[1], p.block[0], p.lds);
            for (int v : p.ints) printf("%d,", v);
            if (p.cols) printf(" nblk0=%d cols=%lld,%lld", p.C.nblk0, (long long)p.C.p[0].cols, (long long)p.C.p[1].cols);
            if (p.have_cp) printf(" slabcols=%lld", (long long)p.CP.cols);
        }
    }
    printf("\n");
    p = Pending();
}

void shim_begin(const char *k, dim3 g, dim3 b, size_t lds) {
    g_p = Pending();
    g_p.live = true;
    g_p.k = k;
    g_p.grid[0] = g.x; g_p.grid[1] = g.y; g_p.grid[2] = g.z;
    g_p.block[0] = b.x;
    g_p.lds = lds;
}
void shim_arg(int v) { g_p.ints.push_back(v); }
void shim_arg(const evc::GemvRowsLaunch &L) { g_p.R = L; g_p.rows = true; }
void shim_arg(const evc::GemvColsLaunch &L) { g_p.C = L; g_p.cols = true; }
void shim_arg(const evc::ColProblem &P) { g_p.CP = P; g_p.have_cp = true; }
void shim_end() {
    if (g_p.k.find("reduce") != std::string::npos) {
        if (g_detail) printf("   + %s grid=%u,%u\n", g_p.k.c_str(), g_p.grid[0], g_p.grid[1]);
        g_p = Pending();
        return;
    }
    if (g_p.k == "gemv_cols_slab_kernel") {
        emit("gemv_cols_slab_kernel");
        g_skip_note = true;
    }
}

namespace evc {
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    printf("ERROR ");
    vprintf(fmt, ap);
    va_end(ap);
    printf("\n");
}
void note_kernel(int, const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (!g_p.live) {
        if (g_skip_note && !strcmp(buf, "gemv_cols_slab_kernel")) { g_skip_note = false; return; }
        printf("NOTE WITHOUT LAUNCH %s\n", buf);
        return;
    }
    emit(buf);
}
}  // namespace evc

using namespace evc;

#ifdef PRE_PLAN_TREE
static void replan(int64_t rows2, RowProblem &rp2, RowProblem &rp1, int count) {
    const bool batched = count > 1;
    if (rows2 > 0 && rows_groups_all_mfma(count) && rows_lds_applicable(rp2, rp1)) {
        plan_rows_lds(rp2, rp1);
        return;
    }
    if (rows2 > 0) plan_rows(rp2, batched);
    plan_rows(rp1, batched);
}
#endif

int main(int argc, char **argv) {
    g_shim_cus = atoi(argv[1]);
    g_detail = !strcmp(argv[2], "detail");
    long long rows2, cols2, ld2, T, n, ld1;
    int count, wt, part;
    const int64_t sw = 1 << 20;
    for (long long rc : {1LL, 7LL, 210LL, 5000LL})
        for (long long cc : {1LL, 63LL, 4097LL, 108345LL, 405450LL}) {
            const long long ld = (cc + 15) / 16 * 16;
            printf("ABI rows %lld x %lld\n", rc, cc);
            if (evc_gemv_rows(kA2, rc, cc, ld, (const double *)0x20000, 1.0, (double *)0x30000, (void *)0x40000,
                              evc_gemv_rows_ws_bytes(rc, cc), nullptr))
                printf("evc_gemv_rows FAILED\n");
            if (evc_gemv_cols(kA2, rc, cc, ld, (const double *)0x20000, (double *)0x30000, nullptr)) printf("evc_gemv_cols FAILED\n");
        }
    while (scanf("%lld %lld %lld %lld %lld %lld %d %d %d", &rows2, &cols2, &ld2, &T, &n, &ld1, &count, &wt, &part) == 9) {
        printf("CASE %lld %lld %lld %lld %lld %lld %d %d %d cus=%d\n", rows2, cols2, ld2, T, n, ld1, count, wt, part, g_shim_cus);
        RowProblem rp2{}, rp1{};
        rp2.rows = rows2; rp2.cols = cols2; rp2.ld = ld2;
        rp1.rows = T * T; rp1.cols = n * n; rp1.ld = ld1;
#ifdef PRE_PLAN_TREE
        if (rows2 > 0) plan_rows(rp2, true);
        plan_rows(rp1, true);
        replan(rows2, rp2, rp1, count);
        const int cap2 = rows2 > 0 ? rows_max_spans(rp2, false) : 1, cap1 = rows_max_spans(rp1, true);
#else
        {
            const RowsPlan plan = plan_gemv_rows(gemv_shape(rp2), gemv_shape(rp1), count, lds_device_cus(), gemv_knobs());
            plan.apply(rp2, rp1);
        }
        const int cap2 = rows2 > 0 ? rows_max_spans(gemv_shape(rp2), false) : 1, cap1 = rows_max_spans(gemv_shape(rp1), true);
#endif
        if (g_detail)
            printf("PLAN nspans=%d,%d span_cols=%lld,%lld cap=%d,%d ws=%zu\n", rp2.nspans, rp1.nspans, (long long)rp2.span_cols,
                   (long long)rp1.span_cols, cap2, cap1, rows2 > 0 ? rows_ws_doubles(rows2, cols2) : (size_t)0);
        RowProblem p2 = rp2, p1 = rp1;
        p2.A = kA2; p2.v = (const double *)0x20000; p2.partial = (double *)0x30000; p2.vstride = p2.pstride = sw;
        if (rows2 == 0) p2.nblocks = 0;
        p1.A = kA1; p1.v = (const double *)0x60000; p1.partial = (double *)0x70000; p1.vstride = p1.pstride = sw;
        if (launch_gemv_rows(p2, p1, count, 0)) printf("K5 FAILED\n");
        ColProblem c2{}, c1{};
        c2.A = kA2; c2.w = (const double *)0x20000; c2.wt = wt ? (const double *)0x80000 : nullptr; c2.wstride = sw;
        c2.rows = rows2; c2.cols = cols2; c2.ld = ld2; c2.out = (double *)0x90000; c2.ostride = sw;
        c1.A = kA1; c1.w = (const double *)0x60000; c1.wt = wt ? (const double *)0xa0000 : nullptr; c1.wstride = sw;
        c1.rows = T * T; c1.cols = n * n; c1.ld = ld1; c1.out = (double *)0xb0000; c1.ostride = sw;
        c1.part = part ? (double *)0xc0000 : nullptr; c1.pstride = sw;
        if (launch_gemv_cols(c2, c1, count, 0)) printf("K8 FAILED\n");
    }
    return 0;
}
