// Host-only check of the pure parts of the orchestration, meant for a sanitizer build: the route functions (route.hpp),
// carve and every workspace byte count, over n = 1, 2, 3, 32, 33, 64, 65, T = 1, 32, 33, 129 and the five layouts; the
// plans of the pair steps and of Y2 (pair_plan.hpp) against the predicates and launcher arithmetic they replaced, over
// n = 1 .. 64, 14 batch sizes, the 16 knob sets and every form of the step the pipeline builds.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I$TREE/evcont_amd/csrc \
//         route_check.hip $TREE/evcont_amd/csrc/*.hip -fsanitize=address,undefined -o route_check
//   ./route_check > counts.txt            prints every byte count
//   ./route_check other_counts.txt        ... and asserts that they equal those of another tree's build
// -DBYTE_COUNTS_ONLY builds the byte-count part alone (extern "C" entry points only): a tree from before route.hpp.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../include/evcont_hip.h"
#ifndef BYTE_COUNTS_ONLY
#include "pipeline.hpp"
using namespace evc;
#endif

static int g_failed = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            printf("FAILED " __VA_ARGS__); \
            printf("\n");                 \
            ++g_failed;                   \
        }                                 \
    } while (0)

static const int kN[] = {1, 2, 3, 32, 33, 64, 65}, kT[] = {1, 32, 33, 129}, kLayouts[] = {6, 5, 3, 2, 8};

static evc_trdm_set make_set(int n, int T, int layout) {
    const int64_t n2 = (int64_t)n * n, ns = (int64_t)n * (n + 1) / 2;
    evc_trdm_set t;
    memset(&t, 0, sizeof t);
    t.n = n;
    t.ntrain = T;
    t.layout = layout;
    t.cols2 = layout == 8 ? ns * (ns + 1) / 2 : (layout == 3 || layout == 2) ? n2 * (n2 + 1) / 2 : n2 * n2;
    t.rows2 = t.rows2_total = (layout == 5 || layout == 2 || layout == 8) ? (int64_t)T * (T + 1) / 2 : (int64_t)T * T;
    t.ld2 = (t.cols2 + 15) / 16 * 16;
    t.ld1 = (n2 + 1) / 2 * 2;
    t.two_rdm = t.one_rdm = t.s_train = (const double *)0x1000;
    return t;
}

#ifndef BYTE_COUNTS_ONLY
static void check_routes() {
    for (int layout : kLayouts)
        for (int n : kN)
            for (int packed = 0; packed < 2; ++packed) {
                const Route r = transform_route(layout, n, packed != 0);
                // the predicates the orchestration used to re-derive at every site
                const bool pair = n <= 32, pair64 = layout == EVC_LAYOUT_SYM8 && n > 32 && n <= 64 && packed;
                const bool pairs = pair || pair64, sym = layout == EVC_LAYOUT_SYM8 && pairs;
                CHECK(r.steps == (pair ? Steps::Pair : pair64 ? Steps::Pair64 : Steps::Quarter), "steps layout=%d n=%d packed=%d",
                      layout, n, packed);
                CHECK(r.pairs() == pairs && r.symmetric == sym, "symmetric layout=%d n=%d packed=%d", layout, n, packed);
                CHECK(r.k3_is_dense_mid() == sym, "k3 layout=%d n=%d packed=%d", layout, n, packed);
                CHECK(r.k3_doubles == (sym ? (int64_t)pair_ld(n) * pair_ld(n) : (int64_t)n * n * n * n),
                      "k3_doubles layout=%d n=%d packed=%d", layout, n, packed);
                CHECK(pair_ld(n) % 16 == 0 && pair_ld(n) >= n * (n + 1) / 2, "pair_ld n=%d", n);
                for (int p2 = 0; p2 < 2; ++p2)
                    CHECK(phases_agree(n, packed != 0, p2 != 0) == (n <= 32 || packed == p2), "phases_agree n=%d", n);
                // the symmetric pipeline keeps the dense intermediate for the fused Y2 kernels: they must cover its range
                if (r.symmetric)
                    CHECK(plan_y2(kY2FromPairs, n, 1, PairKnobs{true, true, true, true}).kernel != kY2Unsupported, "fused Y2 at n=%d", n);
            }
}

// every buffer of a slot: inside the slot, in carving order, on a 256-byte boundary, none overlapping the next
static void check_carve(const evc_trdm_set &t, int natm) {
    char *base = (char *)0x100000;   // (never dereferenced)
    const Ws w = carve(&t, natm, base);
    const double *b[] = {w.X, w.U, w.s, w.lflag, w.h1, w.Dpred, w.Pao, w.Y1, w.B1, w.B2, w.K3, w.G, w.vec2, w.h2part, w.h1part,
                         w.h2rows, w.w2, w.w2t, w.w1, w.w1t, w.d1part, w.y2part, w.y2, w.t2part, w.term3, w.evals, w.evecs,
                         w.vstd, w.bcache, w.sbig};
    const int nb = sizeof b / sizeof b[0];
    CHECK((const char *)b[0] == base && w.base == base, "carve: X at the base");
    for (int i = 0; i < nb; ++i) {
        CHECK(((const char *)b[i] - base) % 256 == 0, "carve: buffer %d misaligned (n=%d T=%d layout=%d)", i, t.n, t.ntrain,
              t.layout);
        CHECK((const char *)b[i] >= base && (const char *)b[i] <= base + w.bytes, "carve: buffer %d outside the slot", i);
        if (i) CHECK(b[i] >= b[i - 1], "carve: buffer %d out of order", i);
    }
    const size_t n4 = (size_t)t.n * t.n * t.n * t.n, ldp = pair_ld(t.n);
    CHECK((size_t)(w.B2 - w.B1) >= n4 && (size_t)(w.B2 - w.B1) >= ldp * ldp && (size_t)(w.G - w.K3) >= ldp * ldp,
          "carve: N^4 buffers too small (n=%d)", t.n);
    CHECK(w.stride * (int64_t)sizeof(double) == (int64_t)w.bytes && w.bytes % 256 == 0, "carve: stride");
    CHECK(w.bytes == evc_workspace_bytes(&t, natm), "carve: bytes != evc_workspace_bytes (n=%d T=%d layout=%d)", t.n, t.ntrain,
          t.layout);
    CHECK(carve(&t, natm, nullptr).bytes == w.bytes && carve(&t, natm, nullptr).X == nullptr, "carve: NULL base");
}

// ---- the plans of pair_plan.hpp against what they replaced: the *_applicable predicates and the launchers' arithmetic,
//      restated here as they stood (knobs as arguments)
namespace old {
constexpr int kPdMaxN = 30;
static bool pair_transform_dma_applicable(const PairTransformArgs &a, int count, bool on) {
    const int npairs = a.n * (a.n + 1) / 2;
    return on && a.n > 16 && a.n <= kPdMaxN && count >= 4 && a.lead_sym && a.in_lower && a.rs_lower && a.in_pairs &&
           !a.k3 && (a.in_ld == 0 || a.in_ld >= npairs) &&
           ((a.out && a.out_pairs && !a.packed && a.out_ld >= 8 * ((npairs + 7) / 8) && a.out_ld % 2 == 0) ||
            (a.packed && a.sym8 && !a.out));
}
static bool pair_transform_dot_applicable(const PairTransformArgs &a, int count, const PairKnobs &k) {
    return k.ip1_pairstep && pair_transform_dma_applicable(a, count, k.pt_dma) && a.out && !a.packed;
}
static bool y2_dma_applicable(int n, bool on) { return on && n > 16 && n <= kPdMaxN; }
static int y2_pairstep_tiles(int count) { return count >= 32 ? 8 : count >= 8 ? 4 : 2; }
static int y2_pairstep_slabs(int n, int count) {
    const int ntiles = (n * (n + 1) / 2 + 7) / 8, t = y2_pairstep_tiles(count);
    return (ntiles + t - 1) / t;
}
static int y2_slab_capacity(int n) { return n > 32 ? 256 : (64 > 128 ? 64 : 128); }
static bool y2_pairstep_applicable(const PairTransformArgs &a, const double *M1, int64_t sws, int count, const PairKnobs &k) {
    const int npairs = a.n * (a.n + 1) / 2;
    const bool aligned = ((reinterpret_cast<uintptr_t>(a.in) | reinterpret_cast<uintptr_t>(M1)) & 15) == 0 &&
                         a.in_ld >= npairs && a.in_ld % 2 == 0 && a.sin % 2 == 0 && sws % 2 == 0;
    return k.y2_pairstep && y2_dma_applicable(a.n, k.pt_dma) && pair_transform_dma_applicable(a, count, k.pt_dma) && a.out &&
           a.ct == 1 && aligned && a.in != a.out && y2_pairstep_slabs(a.n, count) <= y2_slab_capacity(a.n);
}
static bool pair64_applicable(const PairTransformArgs &a) {
    return a.n > 32 && a.n <= 64 && a.lead_sym && a.in_lower && a.rs_lower && a.in_pairs && !a.k3 &&
           ((a.packed && a.sym8 && !a.out) || (a.out && a.out_pairs && !a.packed));
}
static bool y2_64_applicable(int n) { return n > 32 && n <= 64; }
static int y2_64_slabs(int n, int count) {
    const int npairs = n * (n + 1) / 2;
    int wgs = count >= 250 ? 1 : 250 / count;
    const int cap = y2_slab_capacity(n);
    if (wgs > cap) wgs = cap;
    if (wgs > npairs) wgs = npairs;
    const int ppw = (npairs + wgs - 1) / wgs;
    return (npairs + ppw - 1) / ppw;
}
static int y2_fused_ppt(int count) { return count < 4 ? 4 : 8; }
static int y2_fused_tiles(int n, int count) {
    const int ppt = y2_fused_ppt(count);
    const int ntiles = (n * (n + 1) / 2 + ppt - 1) / ppt;
    int t = count < 4 ? 1 : 4;
    while ((ntiles + t - 1) / t > y2_slab_capacity(n)) ++t;
    return t;
}
static int y2_fused_slabs(int n, int count) {
    if (y2_64_applicable(n)) return y2_64_slabs(n, count);
    const int ppt = y2_fused_ppt(count);
    const int ntiles = (n * (n + 1) / 2 + ppt - 1) / ppt, t = y2_fused_tiles(n, count);
    return (ntiles + t - 1) / t;
}
static int p64_rowlen(int npairs) {
    int r = npairs + 4;
    r += (8 - (r & 31) + 32) & 31;
    return r;
}
// LDS bytes of the pair_dma.hip kernels: ptd_kernel<0>, <1>, <0, 1>, y2d_kernel<1>, y2d_kernel<0>
constexpr unsigned kPdRB = 4 * 1024 + 64, kPdTab = 4 * kPdRB + 16 * 3872;
constexpr unsigned kPdLds = kPdTab, kPdLds1 = kPdTab + 512 * 4, kPdLdsDot = kPdTab + 2 * 48 * 8;
constexpr unsigned kPdLdsY = 8 * kPdRB + 16 * 3872 + 4 * 32 * 34 * 8;
constexpr unsigned kY2dLds = 8 * kPdRB > 4 * 32 * 33 * 8 ? 8 * kPdRB : 4 * 32 * 33 * 8;

// launch_pair_transform as it stood: the record, tiles per workgroup, grid.x and LDS of what it launched ("": the error)
struct Launch {
    std::string name;
    int tiles_per_wg;
    unsigned grid_x;
    size_t lds;
};
static Launch fmt(const char *f, int a, int b, int tpw, size_t gx, size_t lds) {
    char buf[64];
    snprintf(buf, sizeof buf, f, a, b);
    return Launch{buf, tpw, (unsigned)gx, lds};
}
static Launch launch_pair_transform(PairTransformArgs a, int count, const PairKnobs &k) {
    if (a.n > 32) {
        if (!pair64_applicable(a)) return Launch{"", 0, 0, 0};
        const int npairs = a.n * (a.n + 1) / 2, ntiles = (npairs + 3) / 4;
        int tpw = (int)ceil_div((int64_t)ntiles * count, (int64_t)250);
        if (tpw < 1) tpw = 1;
        return fmt("pt64_kernel<%d>", a.packed ? 1 : 0, 0, tpw, ceil_div(ntiles, tpw),
                   sizeof(double) * (4096 + 2048 + (size_t)4 * p64_rowlen(npairs)));
    }
    const int n = a.n;
    const int npad = (n + 15) / 16 * 16;
    const int ntq = (n + 7) / 8;
    constexpr int tpw_env = 4;
    a.tiles_per_wg = (count < 4 || tpw_env < 1) ? 1 : (tpw_env > ntq ? ntq : tpw_env);
    const int ntiles = a.lead_sym ? (n * (n + 1) / 2 + 7) / 8 : n * ntq;
    const unsigned grid = (unsigned)((ntiles + a.tiles_per_wg - 1) / a.tiles_per_wg);
    const size_t stage_rows = a.rs_lower ? (size_t)n * (n + 1) / 2 : (size_t)n * n;
    if (pair_transform_dma_applicable(a, count, k.pt_dma)) {
        const int nt8 = (n * (n + 1) / 2 + 7) / 8;
        return fmt(a.packed ? "ptd_kernel<1>" : "ptd_kernel<0>", 0, 0, a.tiles_per_wg,
                   (nt8 + a.tiles_per_wg - 1) / a.tiles_per_wg, a.packed ? kPdLds1 : kPdLds);
    }
    if (k.pt_pipe && a.lead_sym && a.in_lower && a.rs_lower && a.in_pairs && (npad == 16 || npad == 32)) {
        const int mode = a.k3 ? -1 : (a.out && a.out_pairs && !a.packed) ? 0 : (a.packed && a.sym8 && !a.out) ? 1 : -1;
        const size_t npairs = (size_t)n * (n + 1) / 2;
        const size_t lds = sizeof(double) * ((size_t)4 * kPtRowLen + npairs * 16 + 16);
        if (mode >= 0 && count < 4 && npairs >= 8)
            return fmt("pt_pipe4_kernel<%d,%d>", npad, mode, 1, (npairs + 3) / 4,
                       sizeof(double) * ((size_t)4 * kPtRowLen + npairs * 8 + 8));
        if (mode >= 0 && lds <= 80 * 1024)
            return fmt("pt_pipe_kernel<%d,%d>", npad, mode, a.tiles_per_wg,
                       ((npairs + 7) / 8 + a.tiles_per_wg - 1) / a.tiles_per_wg, lds);
    }
    const bool rowbuf = a.in_pairs;
    const size_t rowbuf_doubles = rowbuf ? (size_t)4 * kPtRowLen + 2 : 0;
    if (npad != 16 && npad != 32) return Launch{"", 0, 0, 0};
    return fmt("pt_kernel<%d,%d>", npad, rowbuf ? 1 : 0, a.tiles_per_wg, grid,
               sizeof(double) * ((npad == 16 ? (size_t)16 * 16 : (size_t)32 * 48) + stage_rows * 9 + rowbuf_doubles));
}
}  // namespace old

static const int kCounts[] = {1, 2, 3, 4, 7, 8, 9, 31, 32, 33, 64, 250, 251, 512};
static double *fakep(uintptr_t k) { return (double *)(0x10000000ull * k); }   // (never dereferenced)

static void check_pair_launch(const char *what, const PairTransformArgs &a, int count, int kn, const PairKnobs &k) {
    const PairPlan p = plan_pair_step(a, count, k);
    const old::Launch o = old::launch_pair_transform(a, count, k);
    CHECK(o.name == pair_plan_name(p) && (p.kernel == kPairUnsupported) == o.name.empty(), "%s n=%d count=%d knobs=%d: %s, was %s",
          what, a.n, count, kn, pair_plan_name(p), o.name.c_str());
    CHECK(p.tiles_per_wg == o.tiles_per_wg && p.grid_x == o.grid_x && p.lds == o.lds,
          "%s n=%d count=%d knobs=%d %s: tiles %d grid %u lds %zu, were %d %u %zu", what, a.n, count, kn, pair_plan_name(p),
          p.tiles_per_wg, p.grid_x, p.lds, o.tiles_per_wg, o.grid_x, o.lds);
    if (p.kernel == kPairUnsupported) return;
    CHECK(p.lds <= 160 * 1024, "%s n=%d count=%d: %zu bytes of LDS", what, a.n, count, p.lds);
    CHECK((p.kernel != kPtPipe && p.kernel != kPtd) || p.lds <= 80 * 1024, "%s n=%d count=%d: %zu bytes, two workgroups per CU",
          what, a.n, count, p.lds);
    const int n = a.n, npairs = n * (n + 1) / 2;
    const int ntiles = p.kernel == kPt64 || p.kernel == kPtPipe4 ? (npairs + 3) / 4
                       : p.kernel != kPt || a.lead_sym          ? (npairs + 7) / 8
                                                                : n * ((n + 7) / 8);
    CHECK((int64_t)p.grid_x * p.tiles_per_wg >= ntiles && p.tiles_per_wg >= 1, "%s n=%d count=%d: %u x %d workgroup tiles of %d",
          what, n, count, p.grid_x, p.tiles_per_wg, ntiles);
}

// (the kernel and its template arguments, not the names: pair_plan_name returns one buffer)
static bool same_plan(const PairPlan &a, const PairPlan &b) {
    return a.kernel == b.kernel && a.t[0] == b.t[0] && a.t[1] == b.t[1] && a.tiles_per_wg == b.tiles_per_wg &&
           a.grid_x == b.grid_x && a.lds == b.lds;
}
static bool same_args(const PairTransformArgs &a, const PairTransformArgs &b) { return !memcmp(&a, &b, sizeof a); }

static void check_y2_plan(const Y2Plan &p, int n, int count) {
    CHECK(p.slabs >= 1 && p.slabs <= y2_slab_capacity(n), "%s n=%d count=%d: %d slabs of %d", y2_plan_name(p), n, count, p.slabs,
          y2_slab_capacity(n));
    CHECK(p.lds <= 160 * 1024 && (p.kernel != kY2d || p.lds <= 80 * 1024), "%s n=%d: %zu bytes of LDS", y2_plan_name(p), n, p.lds);
    if (p.kernel != kY2GsT && p.kernel != kY2Sb)
        CHECK((int64_t)p.slabs * p.tiles_per_wg * p.ppt >= n * (n + 1) / 2, "%s n=%d count=%d: %d x %d x %d pairs", y2_plan_name(p),
              n, count, p.slabs, p.tiles_per_wg, p.ppt);
}

static void check_pair_plans() {
    CHECK(y2_slab_capacity(32) == old::y2_slab_capacity(32) && y2_slab_capacity(33) == old::y2_slab_capacity(33) &&
              y2_slabs(7) == 64 && y2_slabs(7) <= y2_slab_capacity(7),
          "y2 slab capacity");
    for (int kn = 0; kn < 16; ++kn) {
        const PairKnobs k{(kn & 1) != 0, (kn & 2) != 0, (kn & 4) != 0, (kn & 8) != 0};
        for (int n = 1; n <= 64; ++n)
            for (int count : kCounts) {
                const int npr = n * (n + 1) / 2, ld = pair_ld(n);
                double *const B1 = fakep(1), *const B2 = fakep(2), *const K3 = fakep(3), *const vec2 = fakep(4);
                PairTransformArgs z;
                memset(&z, 0, sizeof z);
                z.C = fakep(5);
                z.n = n;
                z.sC = z.sin = z.sout = 1 << 24;
                // ---- the energy phase (phase_hamiltonian): sym = the symmetric pipeline, s4 = int2e handed over packed
                for (int sym = 0; sym < 2; ++sym)
                    for (int s4 = 0; s4 <= sym; ++s4) {
                        PairTransformArgs a = z;
                        a.in = fakep(6);
                        a.out = sym ? K3 : B1;
                        a.lead_sym = a.in_lower = a.rs_lower = a.out_pairs = sym;
                        a.in_pairs = s4;
                        a.out_ld = ld;
                        check_pair_launch("energy first", a, count, kn, k);
                        a.in_pairs = a.out_pairs;
                        a.in_ld = a.out_ld;
                        a.out_pairs = a.out_ld = 0;
                        a.in = a.out;
                        a.k3 = sym ? nullptr : K3;
                        a.sk3 = a.sin;
                        PairTransformArgs full = a;
                        full.out = B2;
                        check_pair_launch("energy second, full", full, count, kn, k);
                        a.out = nullptr;
                        a.packed = vec2;
                        a.spacked = a.sin;
                        a.packed_len = (int64_t)npr * (npr + 1) / 2 + 3;
                        a.diag_mult = 0.5;
                        a.sym8 = sym;
                        check_pair_launch(sym ? "energy second, packed sym8" : "energy second, packed reference", a, count, kn, k);
                    }
                // ---- rotate_four_index
                PairTransformArgs r = z;
                r.in = fakep(6);
                r.out = B1;
                for (int ct = 0; ct < 2; ++ct) {
                    r.ct = ct;
                    check_pair_launch("rotate_four_index", r, count, kn, k);
                }
                // ---- the gradient side: the reference layouts' two steps, then the symmetric pipeline's
                PairTransformArgs f = z;
                f.ct = 1;
                f.in = B1;
                f.out = B2;
                f.in_ld = f.out_ld = ld;
                check_pair_launch("gradient first, reference", f, count, kn, k);
                check_pair_launch("gradient second, reference", grad_second_args(f, B1, 0), count, kn, k);
                f.lead_sym = f.in_lower = f.rs_lower = f.out_pairs = f.in_pairs = 1;
                for (int form = 0; form < 4; ++form) {   // dense; N^4-addressed first step; a misaligned operand; an odd stride
                    PairTransformArgs a = f;
                    const double *M1 = K3;
                    int64_t sM1 = a.sin;
                    if (form == 2) a.in = reinterpret_cast<const double *>(reinterpret_cast<uintptr_t>(B1) + 8);
                    if (form == 2 && (count & 1)) M1 = reinterpret_cast<const double *>(reinterpret_cast<uintptr_t>(K3) + 8), a.in = B1;
                    if (form == 3) ((count & 1) ? sM1 : a.sin) += 1;
                    const bool want_G = form == 1, wide = n > 32;
                    for (int s2kl = 0; s2kl < 2; ++s2kl)
                        for (int one_slot = 0; one_slot < 2; ++one_slot) {
                            const GradPairPlan g = plan_grad_pairs(a, B1, M1, sM1, count, want_G, wide, s2kl, one_slot != 0, k);
                            PairTransformArgs a1 = a;
                            a1.in_pairs = (!want_G || wide) ? 1 : 0;
                            check_pair_launch("gradient first", a1, count, kn, k);
                            PairTransformArgs a2 = a1;   // grad_second_args as it stood: the buffers by name
                            a2.in = B2;
                            a2.out = B1;
                            a2.in_pairs = a1.out_pairs;
                            a2.out_pairs = s2kl;
                            check_pair_launch("gradient second", a2, count, kn, k);
                            // gradient_sym8_pairs as it stood
                            const bool pairstep = old::y2_pairstep_applicable(a, M1, sM1, count, k);
                            const bool dot = s2kl && !want_G && !wide && one_slot &&
                                             old::pair_transform_dot_applicable(grad_second_args(a1, B1, 1), count, k);
                            const int nslab = pairstep ? old::y2_pairstep_slabs(n, count) : old::y2_fused_slabs(n, count);
                            CHECK(g.y2_in_first == pairstep && g.dot_in_second == dot && g.nslab() == nslab && g.y2.slabs == nslab,
                                  "gradient plan n=%d count=%d knobs=%d form=%d s2kl=%d one_slot=%d: %d %d %d, were %d %d %d", n,
                                  count, kn, form, s2kl, one_slot, g.y2_in_first, g.dot_in_second, g.nslab(), pairstep, dot, nslab);
                            check_y2_plan(g.y2, n, count);
                            const PairPlan p1 = plan_pair_step(a1, count, k), p2 = plan_pair_step(a2, count, k);
                            CHECK(same_plan(g.first, p1) && same_args(g.first_args, a1) && same_args(g.second_args, a2),
                                  "gradient plan n=%d count=%d knobs=%d form=%d: first step or the steps' arguments", n, count, kn,
                                  form);
                            if (pairstep) {   // launch_y2_pairstep
                                CHECK(g.y2.kernel == kY2dPairstep && g.y2.t == 1 && g.y2.tiles_per_wg == old::y2_pairstep_tiles(count) &&
                                          g.y2.ppt == 8 && g.y2.lds == old::kPdLdsY && g.y2.grid_z == 1 &&
                                          !strcmp(y2_plan_name(g.y2), "y2d_kernel<1> pairstep"),
                                      "y2 pairstep plan n=%d count=%d", n, count);
                            } else {   // launch_y2_fused
                                const bool w64 = old::y2_64_applicable(n), dma = !w64 && old::y2_dma_applicable(n, k.pt_dma);
                                const int npad = (n + 15) / 16 * 16, slabs = old::y2_fused_slabs(n, count);
                                const size_t rows = sizeof(double) * (size_t)8 * kPtRowLen, redb = sizeof(double) * 4 * npad * (npad + 1);
                                char name[32];
                                snprintf(name, sizeof name, w64 ? "y2_64_kernel" : dma ? "y2d_kernel" : "y2_fused_kernel<%d>", npad);
                                CHECK(!strcmp(y2_plan_name(g.y2), name) && g.y2.grid_z == 1, "y2 plan n=%d count=%d: %s, was %s", n,
                                      count, y2_plan_name(g.y2), name);
                                if (w64)
                                    CHECK(g.y2.ppt == (npr + slabs - 1) / slabs &&
                                              g.y2.lds == sizeof(double) * (4096 + 2048 + (size_t)4 * old::p64_rowlen(npr)),
                                          "y2_64 plan n=%d count=%d", n, count);
                                else
                                    CHECK(g.y2.tiles_per_wg == old::y2_fused_tiles(n, count) && g.y2.ppt == old::y2_fused_ppt(count) &&
                                              g.y2.lds == (dma ? old::kY2dLds : rows > redb ? rows : redb),
                                          "y2 fused plan n=%d count=%d", n, count);
                            }
                            if (dot) {   // launch_pair_transform_dot
                                const int t = old::y2_pairstep_tiles(count), nt8 = (npr + 7) / 8;
                                CHECK(g.second.kernel == kPtdDot && !strcmp(pair_plan_name(g.second), "ptd_kernel<0> +ip1") &&
                                          g.second.tiles_per_wg == t && g.second.grid_x == (unsigned)((nt8 + t - 1) / t) &&
                                          g.second.lds == old::kPdLdsDot && g.second.lds <= 160 * 1024,
                                      "dot plan n=%d count=%d", n, count);
                            } else {
                                CHECK(same_plan(g.second, p2), "gradient plan n=%d count=%d knobs=%d form=%d: second step", n, count,
                                      kn, form);
                            }
                        }
                }
                // ---- Y2 with the dense operands (launch_y2, launch_y2_sb)
                for (Y2Operands from : {kY2FromGsT, kY2FromSb}) {
                    const Y2Plan p = plan_y2(from, n, count, k);
                    const int nt = (n + 15) / 16;
                    char name[32];
                    snprintf(name, sizeof name, from == kY2FromSb ? "y2_sb_kernel<%d>" : "y2_kernel<%d>", nt > 4 ? 4 : nt);
                    CHECK(!strcmp(y2_plan_name(p), name) && p.slabs == 64 && p.grid_z == (nt > 4 ? 4u : 1u) && p.lds == 0,
                          "y2 dense plan n=%d: %s, was %s", n, y2_plan_name(p), name);
                    check_y2_plan(p, n, count);
                }
            }
    }
    // beyond the kernels' range: the plan says so
    for (int n : {0, 65, 96}) {
        PairTransformArgs a;
        memset(&a, 0, sizeof a);
        a.n = n;
        CHECK(plan_pair_step(a, 4, PairKnobs{true, true, true, true}).kernel == kPairUnsupported, "pair plan n=%d", n);
        CHECK(plan_y2(kY2FromPairs, n, 4, PairKnobs{true, true, true, true}).kernel == kY2Unsupported, "y2 plan n=%d", n);
    }
    CHECK(plan_y2(kY2FromGsT, 128, 1, PairKnobs{}).t == 4 && plan_y2(kY2FromGsT, 129, 1, PairKnobs{}).kernel == kY2Unsupported,
          "y2 dense plan beyond 128");
}
#endif

int main(int argc, char **argv) {
    std::string out;
    char line[256];
    auto emit = [&](const char *what, int n, int T, int layout, int a, int b, size_t v) {
        snprintf(line, sizeof line, "%s n=%d T=%d layout=%d %d %d : %zu\n", what, n, T, layout, a, b, v);
        out += line;
    };
    for (int n : kN) {
        for (int T : kT)
            for (int layout : kLayouts) {
                const evc_trdm_set t = make_set(n, T, layout);
                for (int natm : {0, 1, 7}) {
                    emit("workspace_bytes", n, T, layout, natm, 0, evc_workspace_bytes(&t, natm));
                    emit("workspace_bytes_batch", n, T, layout, natm, 5, evc_workspace_bytes_batch(&t, natm, 5));
                    emit("workspace_bytes_roots", n, T, layout, natm, 3, evc_workspace_bytes_roots(&t, natm, 3));
                    emit("workspace_bytes_roots_batch", n, T, layout, natm, 6, evc_workspace_bytes_roots_batch(&t, natm, 2, 3));
#ifndef BYTE_COUNTS_ONLY
                    check_carve(t, natm);
#endif
                }
            }
        emit("grad_elec_ws_bytes", n, 0, 0, 0, 0, evc_grad_elec_ws_bytes(n, 0));
        emit("grad_elec_ws_bytes", n, 0, 0, 7, 0, evc_grad_elec_ws_bytes(n, 7));
        emit("integrals_oao_ws_bytes", n, 0, 0, 4, 0, evc_integrals_oao_ws_bytes(n, 4));
    }
    for (int T : kT) emit("subspace_solve_ws_bytes", 0, T, 0, 3, 0, evc_subspace_solve_ws_bytes(T, 3));
    // the rejected inputs: 0 bytes
    {
        evc_trdm_set bad = make_set(3, 2, 8);
        bad.ld2 += 1;
        emit("workspace_bytes bad_set", 3, 2, 8, 1, 0, evc_workspace_bytes(&bad, 1));
        const evc_trdm_set t = make_set(3, 2, 8);
        emit("workspace_bytes_batch count0", 3, 2, 8, 1, 0, evc_workspace_bytes_batch(&t, 1, 0));
        emit("workspace_bytes_roots npairs0", 3, 2, 8, 1, 0, evc_workspace_bytes_roots(&t, 1, 0));
        emit("workspace_bytes_roots_batch slots>4096", 3, 2, 8, 1, 0, evc_workspace_bytes_roots_batch(&t, 1, 64, 65));
        emit("grad_elec_ws_bytes n97", 97, 0, 0, 1, 0, evc_grad_elec_ws_bytes(97, 1));
    }
#ifndef BYTE_COUNTS_ONLY
    check_routes();
    check_pair_plans();
#endif
    fputs(out.c_str(), stdout);
    if (argc > 1) {
        FILE *f = fopen(argv[1], "r");
        if (!f) {
            printf("FAILED cannot open %s\n", argv[1]);
            return 2;
        }
        std::string other;
        while (fgets(line, sizeof line, f))
            if (strncmp(line, "OK", 2) && strncmp(line, "FAILED", 6)) other += line;
        fclose(f);
        CHECK(other == out, "byte counts differ from %s", argv[1]);
    }
    if (g_failed) return 1;
    printf("OK\n");
    return 0;
}
