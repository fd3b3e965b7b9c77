// Which kernel runs the streaming t-RDM contractions of a call (host code only):
//   K5  rows GEMV  y[g][r]   = sum_c A[r,c] v[g][c]     kernels in gemv_stream.hip, gemv_mfma.hip, gemv_lds.hip
//   K8  cols GEMV  out[g][c] = sum_r w[g][r] A[r,c]   kernels in gemv_stream.hip, gemv_mfma.hip, gemv_cols_lds.hip
// The plan of a call is a value -- plan_gemv_rows / plan_gemv_cols, pure functions of the two matrix shapes, the batch
// size, the CU count of the device and the knobs: the span decomposition of K5 and a list of passes, each naming the
// geometries it takes, the problems it carries and ONE kernel instantiation.  launch_gemv_rows / launch_gemv_cols ask for
// the plan and hand every pass to the launcher of its kernel family; evc_trdm_plan_describe prints it (no device needed).
#include <stdlib.h>
#include <string.h>

#include "common.hpp"
#include "kernels.hpp"

namespace evc {

// Matrices of up to this many columns (the 8-fold compressed layout: 108 345 columns at N = 30) give the column-tiled K8
// kernels too few workgroups and weigh no more than the vectors of 32 geometries in K5: they take the row-split K8
// kernels and the <2,7,1> shape of the fragment-shaped K5 kernel.
constexpr int64_t kNarrowMaxCols = 200000;

const GemvKnobs &gemv_knobs() {
    static const GemvKnobs knobs = [] {
        auto num = [](const char *name, long long unset) { return getenv(name) ? atoll(getenv(name)) : unset; };
        return GemvKnobs{num("EVC_ROWS_LDS", 1) != 0, num("EVC_COLS_LDS", 1) != 0, (int)num("EVC_ROWS_LDS_NT", 0),
                         (int64_t)num("EVC_ROWS_LDS_MINCOLS", 4096)};
    }();
    return knobs;
}

int lds_device_cus() {
    static std::atomic<int> known[64];   // per device: 0 = not asked yet, -1 = the query failed
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int cus = known[dev].load(std::memory_order_acquire);
    if (!cus) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = -1;
        known[dev].store(cus, std::memory_order_release);
    }
    return cus > 0 ? cus : 0;
}
static bool lds_device_fits(int cus) { return cus >= kLdsBlocks + kLdsBlocksSmall; }
// 32-bit lane offsets inside a 16-row tile
static bool lds_pitch_fits(const GemvShape &p0, const GemvShape &p1) {
    return 16 * p0.ld * 8 < ((int64_t)1 << 31) && 16 * p1.ld * 8 < ((int64_t)1 << 31);
}

// ------------------------------------------------------------------ K5: span plans
using Spans = GemvSpans;
constexpr int kChunk = 512;  // columns per workgroup step of the VALU kernels
constexpr int kRBPlan = 8;   // row-block height the VALU span plan assumes

// Span plan of the VALU and the fragment-shaped kernels.  `batched` selects the finer decomposition the batched (G > 1)
// kernels want (they own whole row groups, so they need more spans for the same number of workgroups).
static Spans valu_spans(const GemvShape &P, bool batched) {
    const int64_t nchunks = ceil_div(P.cols, kChunk);
    const int64_t nrb = ceil_div(P.rows, kRBPlan);
    // aim at `target` 8-row blocks (span count = target / row blocks) while keeping spans >= min_cps chunks
    const int target = batched ? 8192 : 2048;
    const int min_cps = batched ? 2 : 4;
    int64_t want_spans = ceil_div(target, nrb);
    int64_t cps = nchunks / want_spans;
    if (cps < min_cps) cps = nchunks < min_cps ? nchunks : min_cps;
    if (cps < 1) cps = 1;
    return {cps * kChunk, (int)ceil_div(P.cols, cps * kChunk)};
}

static int lds_row_groups(int64_t rows, int nt) { return (int)ceil_div(ceil_div(rows > 0 ? rows : 1, 16), nt); }

// Span plan of the LDS-staged kernel: spans of 64 m columns (m 16-column chunks for each of the four waves), as many as
// fit `budget` workgroups in one round; row groups of `ntg` tiles.
static Spans lds_spans(const GemvShape &P, int budget, int ntg) {
    int spans = budget / lds_row_groups(P.rows, ntg);
    if (spans < 1) spans = 1;
    int64_t m = ceil_div(ceil_div(P.cols, kLdsChunkCols), 4 * (int64_t)spans);
    if (m < 1) m = 1;
    return {4 * kLdsChunkCols * m, (int)ceil_div(P.cols, 4 * kLdsChunkCols * m)};
}

// Chunks per image NCH of the LDS-staged kernel with NT = 14, 7, 4, 2 tiles per row group: 1, 2, 3, 4; with four sets of
// geometries (33 .. 64 per pass) 0 (no such kernel), 1, 2, 2.  Fewer tiles per row group = more row groups = fewer column spans for the same number of workgroups:
// the partial sums (spans x rows x geometries, written by every workgroup at the same moment and flushed at the end of
// the launch) shrink -- measured at H30 / T = 20 / 32 geometries they cost 3 us in the epilogue and 3 us at the kernel
// boundary with 242 spans -- while the geometry vectors are fetched once per row group (the row groups of a span share an
// XCD: L2 hits).
static int lds_nch(int nt, bool four_sets) {
    return four_sets ? (nt == 7 ? 1 : (nt == 14 ? 0 : 2)) : (nt == 14 ? 1 : (nt == 7 ? 2 : (nt == 4 ? 3 : 4)));
}

// Tiles per row group for a matrix of `rows` rows (`forced`, EVC_ROWS_LDS_NT, names a shape): the largest shape that makes
// at least two row groups and pads the matrix by less than 1/8 (tiles fetched beyond its rows), else the largest one that
// pads by less than 1/8.  Measured at H30 / T = 20 (14 tiles), 32 geometries, rocprofv3 averages of the launch and of
// rows_reduce_kernel behind it: 14 tiles per group 52.7 + 5.9 us, 7: 50.1 + 4.6, 4: 51.2 + 4.5, 2: 51.5 + 0 (33 spans:
// summed inside the eigensolver kernel, +2 us there); the fragment-shaped kernel 57.4 + 4.6.
static int lds_pick_nt(int64_t rows, int forced) {
    const int nt = (int)ceil_div(rows > 0 ? rows : 1, 16);
    static const int order[] = {7, 4, 2, 14};
    int best = 0;
    for (int want_groups = 2; want_groups >= 1 && !best; --want_groups)
        for (int cand : order) {
            const int nrg = (int)ceil_div(nt, cand);
            if (!best && nrg >= want_groups && nrg * cand * 8 <= nt * 9 && nrg <= kLdsBlocks / 8) best = cand;
        }
    if (!best) {   // few tiles: the shape that fetches the fewest tiles, the larger one on a tie
        int fewest = 1 << 30;
        for (int cand : order) {
            const int tiles = (int)ceil_div(nt, cand) * cand;
            if (tiles < fewest || (tiles == fewest && cand > best)) {
                fewest = tiles;
                best = cand;
            }
        }
    }
    return forced == 14 || forced == 7 || forced == 4 || forced == 2 ? forced : best;
}

// How the small (one-body) problem travels when the large one takes the LDS-staged kernel: in the same launch if its row
// groups fit a few workgroups; a tall one (T^2 rows: large training sets) in a launch of its own -- of the LDS-staged
// kernel too if its row groups leave room for a few spans, else of the fragment-shaped kernel.
enum SmallRoute { kRides, kOwnLds, kOwnMfma };
static SmallRoute lds_small_route(const GemvShape &p1) {
    const int nrg = lds_row_groups(p1.rows, 14);
    if (nrg <= kLdsBlocksSmall) return kRides;
    return p1.cols >= 4 * kLdsChunkCols && nrg <= (kLdsBlocks + kLdsBlocksSmall) / 4 ? kOwnLds : kOwnMfma;
}

int rows_max_spans(const GemvShape &P, bool small) {
    if (P.rows <= 0 || P.cols <= 0) return 0;   // (no such problem: no plan gives it a span)
    // (the workspace must not depend on the device or the knobs: both span plans, whether or not the LDS-staged kernel
    //  would take this problem.  The finer VALU plan; of the LDS shapes the 14-tile one has the fewest row groups, hence
    //  the most spans, and a tall small problem is planned for a whole round of its own)
    const int budget = small && lds_small_route(P) == kRides ? kLdsBlocksSmall : kLdsBlocks + kLdsBlocksSmall;
    const int a = valu_spans(P, true).nspans, b = lds_spans(P, budget, 14).nspans;
    return a > b ? a : b;
}

size_t rows_ws_doubles(int64_t rows, int64_t cols) { return (size_t)rows * rows_max_spans({rows, cols, cols}, false); }

void RowsPlan::apply(RowProblem &p0, RowProblem &p1) const {
    RowProblem *p[2] = {&p0, &p1};
    for (int k = 0; k < 2; ++k) {
        p[k]->span_cols = spans[k].span_cols;
        p[k]->nspans = p[k]->nblocks = spans[k].nspans;
    }
}

// ------------------------------------------------------------------ K5: the plan
static GemvPass make_pass(int g0, int G, GemvKernel kernel, int t0, int t1, int t2, int t3, int slot0, int slot1) {
    return GemvPass{g0, G, kernel, {t0, t1, t2, t3}, {slot0, slot1}};
}

// the fragment-shaped kernel for G geometries: one geometry set <1,4,2>, two sets <2,3,2>, on narrow matrices <2,7,1>
static GemvPass rows_mfma_pass(int g0, int G, int64_t cols0, int slot0, int slot1) {
    if (G <= 16) return make_pass(g0, G, kRowsMfma, 1, 4, 2, 1, slot0, slot1);
    return cols0 <= kNarrowMaxCols ? make_pass(g0, G, kRowsMfma, 2, 7, 1, 1, slot0, slot1)
                                   : make_pass(g0, G, kRowsMfma, 2, 3, 2, 1, slot0, slot1);
}

RowsPlan plan_gemv_rows(const GemvShape &p0, const GemvShape &p1, int count, int device_cus, const GemvKnobs &knobs) {
    RowsPlan plan{};
    const bool have[2] = {p0.rows > 0 && p0.cols > 0, p1.rows > 0 && p1.cols > 0};
    const int s0 = have[0] ? 0 : -1, s1 = have[1] ? 1 : -1;
    // The LDS-staged kernel: every group of the batch on the matrix cores (no remainder of fewer than kMfmaMinG), a
    // device it fills, a matrix worth streaming whose row groups (14 tiles) leave room for spans.
    const int rest = count % kMaxBatchG;
    const bool lds = have[0] && count >= kMfmaMinG && (rest == 0 || rest >= kMfmaMinG) && knobs.rows_lds &&
                     lds_device_fits(device_cus) && p0.cols >= knobs.lds_min_cols && lds_pitch_fits(p0, p1) &&
                     lds_row_groups(p0.rows, 14) <= kLdsBlocks / 8;
    const int ntg = lds ? lds_pick_nt(p0.rows, knobs.rows_lds_nt) : 0;
    const SmallRoute route = lds && have[1] ? lds_small_route(p1) : kRides;
    Spans(&sp)[2] = plan.spans;
    if (lds) {
        // both problems of ONE launch run in one kernel shape (the large problem's); together they fill one round
        if (have[1])
            sp[1] = route == kRides    ? lds_spans(p1, kLdsBlocksSmall, ntg)
                    : route == kOwnLds ? lds_spans(p1, kLdsBlocks + kLdsBlocksSmall, 14)
                                       : valu_spans(p1, true);
        const int riding = have[1] && route == kRides ? lds_row_groups(p1.rows, ntg) * sp[1].nspans : 0;
        sp[0] = lds_spans(p0, kLdsBlocks + kLdsBlocksSmall - riding, ntg);
    } else {
        if (have[0]) sp[0] = valu_spans(p0, count > 1);
        if (have[1]) sp[1] = valu_spans(p1, count > 1);
    }
    if (!have[0] && !have[1]) return plan;
    for (int g0 = 0; g0 < count;) {
        const int left = count - g0;
        int G;
        if (left >= kMfmaMinG && lds) {
            // (up to 64 geometries, four sets, per pass with row groups of <= 7 tiles when both problems share the launch)
            const int gmax = route == kRides && lds_nch(ntg, true) ? 2 * kMaxBatchG : kMaxBatchG;
            G = left < gmax ? left : gmax;
            const int gs = G > 32 ? 4 : (G > 16 ? 2 : 1);
            plan.passes.push_back(make_pass(g0, G, kRowsLds, gs, ntg, lds_nch(ntg, G > 32), 0, 0, route == kRides ? s1 : -1));
            if (route == kOwnLds) plan.passes.push_back(make_pass(g0, G, kRowsLds, gs, 14, 1, 0, 1, -1));
            if (route == kOwnMfma) plan.passes.push_back(rows_mfma_pass(g0, G, p0.cols, -1, 1));
        } else if (left >= kMfmaMinG) {
            G = left < kMaxBatchG ? left : kMaxBatchG;
            plan.passes.push_back(rows_mfma_pass(g0, G, p0.cols, s0, s1));
        } else {
            G = left >= 8 ? 8 : (left >= 4 ? 4 : (left >= 2 ? 2 : 1));
            plan.passes.push_back(G >= 4 ? make_pass(g0, G, kRowsWaveRows, 32 / G, G, G / 2, 0, s0, s1)
                                         : make_pass(g0, G, kRowsValu, 8, G, 0, 0, s0, s1));
        }
        g0 += G;
    }
    return plan;
}

// ------------------------------------------------------------------ K8: the plan
// ring depth of the LDS-staged kernel for a problem with `rows` rows and eight waves per workgroup: 24, 12 or 6 pieces,
// 0: the weights (rows x 32) and the rings do not fit the LDS
static int cols_lds_depth(int64_t rows) {
    const int64_t rows_w = ((rows + 15) / 16) * 16;
    const int64_t d = (160 * 1024 - rows_w * 256) / (8 * 1024);
    return d >= 24 ? 24 : (d >= 12 ? 12 : (d >= 6 ? 6 : 0));
}

// The LDS-staged pass for G geometries from g0 on, if there is one (else false): gemv_cols_lds_kernel with the weights
// of all rows in LDS, gemv_cols_lds_slab_kernel for a tall matrix.
static bool cols_lds_pass(const GemvShape &p0, const GemvShape &p1, int g0, int G, bool wt, bool part, int device_cus,
                          const GemvKnobs &knobs, int s1, GemvPass &ps) {
    if (!knobs.cols_lds || !lds_device_fits(device_cus) || p0.cols < knobs.lds_min_cols || p0.rows <= 0 ||
        p0.rows > (1 << 20) || !lds_pitch_fits(p0, p1))
        return false;
    // one set of geometries (G <= 16): the row-split kernel of gemv_mfma.hip is faster (31.8 against 36.1 us at H30)
    if (G <= 16) return false;
    if (cols_lds_depth(p0.rows) >= 12) {
        if (s1 >= 0 && (cols_lds_depth(p1.rows) < 6 || part)) return false;
        ps = make_pass(g0, G, kColsLds, 2, 12, s1 >= 0 && cols_lds_depth(p1.rows) < 12 ? 6 : 12, 8, 0, s1);
        return true;
    }
    // slab kernel: every wave's tiles in one round of <= 4, transposed weights of a whole group of kMaxBatchG for the
    // LDS-DMA staging, a small second problem (<= 128 tiles: one per wave of <= 16 workgroups)
    const int64_t rounds = ceil_div(ceil_div(p0.cols, 16), (int64_t)8 * kLdsBlocks);
    if (!wt || g0 % kMaxBatchG != 0 || rounds > 4 || (s1 >= 0 && p1.cols > 2048)) return false;
    ps = make_pass(g0, G, kColsLdsSlab, 2, (int)rounds, 0, 0, 0, s1);
    return true;
}

std::vector<GemvPass> plan_gemv_cols(const GemvShape &p0, const GemvShape &p1, int count, bool wt, bool part,
                                     int device_cus, const GemvKnobs &knobs) {
    std::vector<GemvPass> passes;
    if (count <= 0) return passes;
    int s1 = p1.cols > 0 ? 1 : -1;
    if (part && s1 >= 0 && p1.rows >= 1024 && p1.cols <= 16384 && count < kMfmaMinG) {
        // (groups of >= 12 geometries go through the matrix-core kernels, whose waves split the rows of a tile)
        // the narrow second problem in row slabs, a pass of its own for the whole batch; the wide one alone below
        passes.push_back(make_pass(0, count, kColsSlab, 0, 0, 0, 0, -1, 1));
        s1 = -1;
    }
    if (p0.cols <= 0 && s1 < 0) return passes;
    const bool narrow = p0.cols <= kNarrowMaxCols;
    for (int g0 = 0; g0 < count;) {
        const int left = count - g0;
        int G;
        GemvPass ps;
        if (left >= kMfmaMinG) {
            G = left < kMaxBatchG ? left : kMaxBatchG;
            if (!cols_lds_pass(p0, p1, g0, G, wt, part, device_cus, knobs, s1, ps)) {
                if (narrow) ps = G > 16 ? make_pass(g0, G, kColsMfmaRs, 8, 3, 2, 0, 0, s1) : make_pass(g0, G, kColsMfmaRs, 2, 6, 1, 0, 0, s1);
                else ps = G > 16 ? make_pass(g0, G, kColsMfma, 2, 2, 4, 2, 0, s1) : make_pass(g0, G, kColsMfma, 1, 2, 6, 1, 0, s1);
            }
        } else {
            G = left >= 8 ? 8 : (left >= 4 ? 4 : (left >= 2 ? 2 : 1));
            ps = make_pass(g0, G, narrow ? kColsValuRs : kColsValu, G, 0, 0, 0, 0, s1);
        }
        passes.push_back(ps);
        g0 += G;
    }
    return passes;
}

// ------------------------------------------------------------------ names, launches
const char *gemv_pass_name(const GemvPass &ps) {
    static thread_local char buf[96];
    const int *t = ps.t;
    switch (ps.kernel) {
        case kRowsValu: snprintf(buf, sizeof(buf), "gemv_rows_kernel<%d,%d> G=%d", t[0], t[1], ps.G); break;
        case kRowsWaveRows: snprintf(buf, sizeof(buf), "gemv_rows_wr_kernel<%d,%d,%d> G=%d", t[0], t[1], t[2], ps.G); break;
        case kRowsMfma: snprintf(buf, sizeof(buf), "gemv_rows_mfma_pipe_kernel<%d,%d,%d,%d> G=%d", t[0], t[1], t[2], t[3], ps.G); break;
        case kRowsLds: snprintf(buf, sizeof(buf), "gemv_rows_lds_kernel<%d,%d,%d> G=%d", t[0], t[1], t[2], ps.G); break;
        case kColsValu: snprintf(buf, sizeof(buf), "gemv_cols_kernel<%d>", t[0]); break;
        case kColsValuRs: snprintf(buf, sizeof(buf), "gemv_cols_rs_kernel<%d>", t[0]); break;
        case kColsSlab: snprintf(buf, sizeof(buf), "gemv_cols_slab_kernel"); break;
        case kColsMfma: snprintf(buf, sizeof(buf), "gemv_cols_mfma_kernel<%d,%d,%d,%d>", t[0], t[1], t[2], t[3]); break;
        case kColsMfmaRs: snprintf(buf, sizeof(buf), "gemv_cols_mfma_rs_kernel<%d,%d,%d>", t[0], t[1], t[2]); break;
        case kColsLds: snprintf(buf, sizeof(buf), "gemv_cols_lds_kernel<%d,%d,%d,%d>", t[0], t[1], t[2], t[3]); break;
        case kColsLdsSlab: snprintf(buf, sizeof(buf), "gemv_cols_lds_slab_kernel<%d,%d>", t[0], t[1]); break;
    }
    return buf;
}

int launch_gemv_rows(RowProblem p0, RowProblem p1, int count, hipStream_t st) {
    static RowsLauncher *const launcher[] = {launch_rows_valu, launch_rows_wave_rows, launch_rows_mfma, launch_rows_lds};
    const RowProblem *P[2] = {&p0, &p1};
    GemvShape sh[2] = {gemv_shape(p0), gemv_shape(p1)};
    for (int k = 0; k < 2; ++k)
        if (!P[k]->nblocks) sh[k].rows = 0;
    for (const GemvPass &ps : plan_gemv_rows(sh[0], sh[1], count, lds_device_cus(), gemv_knobs()).passes) {
        GemvRowsLaunch L;
        for (int k = 0; k < 2; ++k) {
            L.p[k] = *P[ps.slot[k] >= 0 ? ps.slot[k] : k];
            if (ps.slot[k] < 0) L.p[k].nblocks = 0;
        }
        if (int rc = launcher[ps.kernel - kRowsValu](L, ps, st)) return rc;
        note_kernel(EVC_PROF_ROWS, "%s", gemv_pass_name(ps));
    }
    return 0;
}

int launch_gemv_cols(ColProblem p0, ColProblem p1, int count, hipStream_t st) {
    static ColsLauncher *const launcher[] = {launch_cols_valu,    launch_cols_valu_rs, launch_cols_slab,    launch_cols_mfma,
                                             launch_cols_mfma_rs, launch_cols_lds,     launch_cols_lds_slab};
    for (const GemvPass &ps : plan_gemv_cols({p0.rows, p0.cols, p0.ld}, {p1.rows, p1.cols, p1.ld}, count,
                                             p0.wt && aligned16(p0.wt), p1.part != nullptr, lds_device_cus(), gemv_knobs())) {
        GemvColsLaunch L{{p0, p1}, 0};
        if (ps.slot[1] < 0) L.p[1].cols = 0;
        if (int rc = launcher[ps.kernel - kColsValu](L, ps, st)) return rc;
        note_kernel(EVC_PROF_COLS, "%s", gemv_pass_name(ps));
    }
    return 0;
}

}  // namespace evc

// ------------------------------------------------------------------ C ABI
using namespace evc;

extern "C" size_t evc_gemv_rows_ws_bytes(int64_t rows, int64_t cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return rows_ws_doubles(rows, cols) * sizeof(double);
}

extern "C" int evc_gemv_rows(const double *A, int64_t rows, int64_t cols, int64_t ld, const double *v,
                             double alpha, double *y, void *ws, size_t ws_bytes, void *stream) {
    EVC_REQUIRE(rows > 0 && cols > 0, "evc_gemv_rows: rows=%lld cols=%lld must be positive",
                (long long)rows, (long long)cols);
    EVC_REQUIRE(A && v && y && ws, "evc_gemv_rows: null pointer");
    EVC_REQUIRE(ld >= cols && (ld % 2) == 0, "evc_gemv_rows: ld=%lld must be even and >= cols=%lld",
                (long long)ld, (long long)cols);
    EVC_REQUIRE(aligned16(A) && aligned16(v), "evc_gemv_rows: A and v must be 16-byte aligned");
    EVC_REQUIRE(ws_bytes >= evc_gemv_rows_ws_bytes(rows, cols), "evc_gemv_rows: workspace too small");
    RowProblem P{A, v, static_cast<double *>(ws), rows, cols, ld}, none{};
    plan_gemv_rows(gemv_shape(P), gemv_shape(none), 1, lds_device_cus(), gemv_knobs()).apply(P, none);
    if (int rc = launch_gemv_rows(P, none, 1, as_stream(stream))) return rc;
    return launch_rows_reduce(P.partial, rows, P.nspans, alpha, y, as_stream(stream));
}

extern "C" int evc_gemv_cols(const double *A, int64_t rows, int64_t cols, int64_t ld, const double *w,
                             double *out, void *stream) {
    EVC_REQUIRE(rows > 0 && cols > 0, "evc_gemv_cols: rows=%lld cols=%lld must be positive",
                (long long)rows, (long long)cols);
    EVC_REQUIRE(A && w && out, "evc_gemv_cols: null pointer");
    EVC_REQUIRE(ld >= cols && (ld % 2) == 0, "evc_gemv_cols: ld=%lld must be even and >= cols=%lld",
                (long long)ld, (long long)cols);
    EVC_REQUIRE(aligned16(A) && aligned16(out), "evc_gemv_cols: A and out must be 16-byte aligned");
    return launch_gemv_cols(ColProblem{A, w, nullptr, out, rows, cols, ld}, ColProblem{}, 1, as_stream(stream));
}

// One line per pass, K5 first:  "K5 g0=<g0> G=<G> <kernel name> nspans=<two-body>,<one-body>" (0: the pass does not carry
// that problem) and "K8 g0=<g0> G=<G> <kernel name>".  Returns the length of the whole text (truncated to buf_len - 1
// characters in buf), -1 on an invalid argument.
extern "C" int evc_trdm_plan_describe(const evc_trdm_set *t, int count, int device_cus, char *buf, size_t buf_len) {
    EVC_REQUIRE(t && buf && buf_len > 0, "evc_trdm_plan_describe: trdm_set / buf is NULL");
    EVC_REQUIRE(t->n >= 1 && t->ntrain >= 1 && t->rows2 >= 0 && t->cols2 >= 1 && count >= 1,
                "evc_trdm_plan_describe: n=%d ntrain=%d rows2=%lld cols2=%lld count=%d", t->n, t->ntrain,
                (long long)t->rows2, (long long)t->cols2, count);
    const int cus = device_cus > 0 ? device_cus : lds_device_cus();
    const int64_t T2 = (int64_t)t->ntrain * t->ntrain;
    const GemvShape p0{t->rows2, t->cols2, t->ld2}, p1{T2, (int64_t)t->n * t->n, t->ld1};
    const RowsPlan rows = plan_gemv_rows(p0, p1, count, cus, gemv_knobs());
    size_t len = 0;
    buf[0] = 0;
    auto line = [&](const char *stage, const GemvPass &ps, const char *tail) {
        char text[192];
        const int n = snprintf(text, sizeof(text), "%s g0=%d G=%d %s%s\n", stage, ps.g0, ps.G, gemv_pass_name(ps), tail);
        if (len + 1 < buf_len) snprintf(buf + len, buf_len - len, "%s", text);
        len += (size_t)n;
    };
    for (const GemvPass &ps : rows.passes) {
        int ns[2] = {0, 0};
        for (int s : ps.slot)
            if (s >= 0) ns[s] = rows.spans[s].nspans;
        char tail[48];
        snprintf(tail, sizeof(tail), " nspans=%d,%d", ns[0], ns[1]);
        line("K5", ps, tail);
    }
    // (the operands phase_gradient brings: transposed weights for more than one geometry, slab scratch from T^2 = 1024 on)
    for (const GemvPass &ps : plan_gemv_cols(p0, p1, count, count > 1, T2 >= 1024, cus, gemv_knobs())) line("K8", ps, "");
    return (int)len;
}
