// Host-only check of the pure parts of the orchestration, meant for a sanitizer build: the route functions (route.hpp),
// carve and every workspace byte count, over n = 1, 2, 3, 32, 33, 64, 65, T = 1, 32, 33, 129 and the five layouts.
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
                if (r.symmetric) CHECK(n <= kPairTransformMaxN || y2_64_applicable(n), "fused Y2 at n=%d", n);
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
