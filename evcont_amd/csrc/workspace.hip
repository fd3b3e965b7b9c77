// The views of a call and its workspace: set and geometry checks, the constructors of Geo / Out, the carving of a geometry
// slot, the set-up of a call, the workspace byte counts.
#include "pipeline.hpp"

namespace evc {

int check_set(const evc_trdm_set *t) {
    EVC_REQUIRE(t != nullptr, "trdm_set is NULL");
    EVC_REQUIRE(t->n >= 1 && t->n <= kMaxOrbitals, "trdm_set: n=%d out of range 1..%d", t->n, kMaxOrbitals);
    EVC_REQUIRE(t->ntrain >= 1 && t->ntrain <= kSubspaceMaxT, "trdm_set: ntrain=%d out of range 1..%d", t->ntrain,
                kSubspaceMaxT);
    EVC_REQUIRE(t->layout == 6 || t->layout == 5 || t->layout == 3 || t->layout == 2 || t->layout == EVC_LAYOUT_SYM8,
                "trdm_set: layout=%d (must be the ndim of two_RDM: 6, 5, 3 or 2, or EVC_LAYOUT_SYM8)", t->layout);
    const int64_t n2 = (int64_t)t->n * t->n, ns = (int64_t)t->n * (t->n + 1) / 2;
    const int64_t cols = is_sym8(t->layout) ? ns * (ns + 1) / 2 : is_packed(t->layout) ? n2 * (n2 + 1) / 2 : n2 * n2;
    const int64_t rows = layout_pairs(t->layout) ? (int64_t)t->ntrain * (t->ntrain + 1) / 2
                                              : (int64_t)t->ntrain * t->ntrain;
    EVC_REQUIRE(t->cols2 == cols, "trdm_set: cols2=%lld, expected %lld", (long long)t->cols2, (long long)cols);
    EVC_REQUIRE(t->rows2_total == rows, "trdm_set: rows2_total=%lld, expected %lld", (long long)t->rows2_total,
                (long long)rows);
    EVC_REQUIRE(t->rows2 >= 0 && t->row_offset >= 0 && t->row_offset + t->rows2 <= rows,
                "trdm_set: local rows [%lld,+%lld) outside 0..%lld", (long long)t->row_offset,
                (long long)t->rows2, (long long)rows);
    EVC_REQUIRE(t->ld2 >= cols && t->ld2 % 2 == 0, "trdm_set: ld2=%lld must be even and >= cols2",
                (long long)t->ld2);
    EVC_REQUIRE(t->ld1 >= n2 && t->ld1 % 2 == 0, "trdm_set: ld1=%lld must be even and >= N*N", (long long)t->ld1);
    EVC_REQUIRE(t->rows2 == 0 || (t->two_rdm && aligned16(t->two_rdm)), "trdm_set: two_rdm NULL or misaligned");
    EVC_REQUIRE(t->one_rdm && aligned16(t->one_rdm) && t->s_train, "trdm_set: one_rdm/s_train NULL or misaligned");
    return 0;
}

Ws carve(const evc_trdm_set *t, int natm, char *base) {
    Ws w;
    const size_t n = t->n, n2 = n * n, n4 = n2 * n2, T = t->ntrain;
    size_t off = 0;
    auto take = [&](size_t doubles) {
        double *p = base ? reinterpret_cast<double *>(base + off) : nullptr;
        off += align_up(doubles * sizeof(double), 256);
        return p;
    };
    w.X = take(n2);
    w.U = take(n2);
    w.s = take(n);
    w.lflag = take(1);
    w.h1 = take(n2);
    w.Dpred = take(n2);
    w.Pao = take(n2);
    w.Y1 = take(n2);
    // (the symmetric pipeline keeps dense (pair, pair) matrices in these: pair_ld(n) rows -- whole 16-row groups are
    //  written -- at the pitch pair_ld(n), which exceeds n^4 doubles for n <= 3)
    const size_t ldp = (size_t)pair_ld((int)n), nbig = n4 > ldp * ldp ? n4 : ldp * ldp;
    w.B1 = take(nbig);
    w.B2 = take(nbig);
    w.K3 = take(nbig);
    w.G = take(n4);
    w.vec2 = take((size_t)t->ld2 + 2);
    const GemvShape s2{t->rows2, t->cols2, t->ld2}, s1{(int64_t)(T * T), (int64_t)n2, t->ld1};
    // (carved for the span plan with the most spans, gemv_dispatch.hip; setup picks the plan of the actual call)
    w.h2part = take((size_t)t->rows2 * (t->rows2 > 0 ? rows_max_spans(s2, false) : 1) + 1);
    w.h1part = take((size_t)T * T * rows_max_spans(s1, true));
    w.h2rows = take((size_t)t->rows2_total);
    w.w2 = take((size_t)t->rows2 + 1);
    w.w2t = take((size_t)t->rows2 * kMaxBatchG + 1);
    w.w1 = take(T * T);
    w.w1t = take((size_t)T * T * kMaxBatchG);
    w.d1part = take(T * T >= 1024 ? (size_t)kColSlabs * t->ld1 : 0);
    w.y2part = take((size_t)y2_slab_capacity((int)n) * n2);
    w.y2 = take(n2);
    w.t2part = take((size_t)n * 3 * ip1_chunks((int)n));
    w.term3 = take((size_t)(natm > 0 ? natm : 1) * 3);
    w.evals = take(T);
    w.evecs = take(T * T);
    const size_t Tp = (T + 15) & ~(size_t)15;   // T > kSubspaceSmallT: matrices at pitch Tp (subspace_big.hip)
    const bool bigT = T > (size_t)kSubspaceSmallT;
    w.vstd = take(bigT ? Tp * Tp : ((T + 1) & ~(size_t)1) * ((T + 1) & ~(size_t)1));
    w.bcache = take(bigT ? 2 * Tp * Tp : 2 * T * T);
    w.sbig = take(bigT ? subspace_big_scratch_doubles((int)T) : 0);
    w.base = base;
    w.bytes = off;
    w.stride = (int64_t)(off / sizeof(double));
    return w;
}

LoewdinArgs loewdin_args(int n, const Geo &g, const Call &c) {
    const Ws &w = c.w;
    LoewdinArgs la{};
    la.S = g.S;
    la.h = g.hcore;
    la.X = w.X;
    la.U = w.U;
    la.s = w.s;
    la.h1 = w.h1;
    la.sS = g.sS;
    la.sh = g.sh;
    la.sws = w.stride;
    la.n = n;
    la.warm = c.warm ? 1 : 0;
    la.scratch = w.B1;   // (free until the integral rotation; n > 64 only)
    la.sscratch = w.stride;
    la.flag = w.lflag;   // (read by the two halves of a split step only)
    return la;
}

Geo geo_single(const evc_geometry *g) {
    Geo o;
    memset(&o, 0, sizeof(o));
    if (!g) return o;
    o.natm = g->natm;
    o.count = 1;
    o.S = g->S;
    o.hcore = g->hcore;
    o.eri = g->eri;
    o.ipovlp = g->ipovlp;
    o.dhcore = g->dhcore;
    o.eri_ip1 = g->eri_ip1;
    o.gnuc = g->gnuc;
    o.aoslices = g->aoslices;
    o.enuc = g->enuc;
    return o;
}

Geo geo_batch(const evc_trdm_set *t, const evc_geometry_batch *gb) {
    Geo g;
    memset(&g, 0, sizeof(g));
    if (!t || !gb) return g;
    const int64_t n2 = (int64_t)t->n * t->n, n4 = n2 * n2, A3 = (int64_t)gb->natm * 3;
    g.natm = gb->natm;
    g.count = gb->count;
    g.batch = 1;
    g.S = gb->S;
    g.sS = n2;
    g.hcore = gb->hcore;
    g.sh = n2;
    g.eri = gb->eri;
    g.seri = n4;
    g.ipovlp = gb->ipovlp;
    g.sip = 3 * n2;
    g.dhcore = gb->dhcore;
    g.sdh = A3 * n2;
    g.eri_ip1 = gb->eri_ip1;
    g.sip1 = 3 * n4;   // (phase_gradient: the packed size with EVC_FLAG_IP1_S2KL)
    g.gnuc = gb->gnuc;
    g.sgn = A3;
    g.aoslices = gb->aoslices;
    g.enuc_dev = gb->enuc;
    return g;
}

int check_geometry(const char *who, const Geo &g, bool need_grad) {
    EVC_REQUIRE(g.count >= 1 && g.count <= 4096,
                "%s: geometry is NULL / null batch descriptor, or count=%d out of range 1..4096", who, g.count);
    EVC_REQUIRE(g.S && g.hcore && g.eri && (!g.batch || g.enuc_dev), "%s: geometry: S/hcore/eri%s must be given", who,
                g.batch ? "/enuc" : "");
    // (the pair kernels fetch the rows of the two large arrays through 16-byte windows)
    EVC_REQUIRE(aligned16(g.eri) && (!g.eri_ip1 || aligned16(g.eri_ip1)),
                "%s: geometry: eri / eri_ip1 must be 16-byte aligned", who);
    if (need_grad)
        EVC_REQUIRE(g.natm >= 1 && g.ipovlp && g.dhcore && g.eri_ip1 && g.aoslices && (!g.batch || g.gnuc),
                    "%s: geometry: natm=%d, ipovlp/dhcore/eri_ip1/aoslices%s are required for the gradient", who, g.natm,
                    g.batch ? "/gnuc" : "");
    return 0;
}

Out out_single(const evc_outputs *o) {
    Out r;
    memset(&r, 0, sizeof(r));
    if (o) {
        r.energy = o->energy;
        r.coeffs = o->coeffs;
        r.grad = o->grad;
        r.d_pred = o->d_pred;
        r.g_pred = o->g_pred;
        r.hmat = o->hmat;
    }
    return r;
}

Out out_batch(const evc_trdm_set *t, const evc_geometry_batch *gb, const evc_outputs_batch *ob) {
    Out r;
    memset(&r, 0, sizeof(r));
    if (t && gb && ob) {
        const int64_t n2 = (int64_t)t->n * t->n, T = t->ntrain;
        r.energy = ob->energy;
        r.se = T;
        r.coeffs = ob->coeffs;
        r.sc = T * T;
        r.grad = ob->grad;
        r.sg = (int64_t)gb->natm * 3;
        r.d_pred = ob->d_pred;
        r.sd = n2;
        r.g_pred = ob->g_pred;
        r.sG = n2 * n2;
        r.hmat = ob->hmat;
        r.sH = T * T;
    }
    return r;
}

int setup(const char *who, const evc_trdm_set *t, Geo &g, int flags, void *ws, size_t ws_bytes, int slots, Call &c) {
    EVC_REQUIRE(ws && aligned16(ws), "%s: workspace NULL or misaligned", who);
    c.w = carve(t, g.natm, static_cast<char *>(ws));
    EVC_REQUIRE(ws_bytes >= c.w.bytes * (size_t)slots, "%s: workspace too small: %zu < %zu", who, ws_bytes,
                c.w.bytes * (size_t)slots);
    memset(&c.rp2, 0, sizeof(c.rp2));
    memset(&c.rp1, 0, sizeof(c.rp1));
    c.rp2.rows = t->rows2;
    c.rp2.cols = t->cols2;
    c.rp2.ld = t->ld2;
    c.rp1.rows = (int64_t)t->ntrain * t->ntrain;
    c.rp1.cols = (int64_t)t->n * t->n;
    c.rp1.ld = t->ld1;
    // span plan of this call (never more spans than the buffers were carved for)
    plan_gemv_rows(gemv_shape(c.rp2), gemv_shape(c.rp1), slots, lds_device_cus(), gemv_knobs()).apply(c.rp2, c.rp1);
    c.warm = (flags & EVC_FLAG_WARM_START) != 0;
    c.loewdin_done = (flags & EVC_FLAG_LOEWDIN_DONE) != 0;
    c.split = 0;
    g.eri_s4 = (flags & EVC_FLAG_ERI_S4) ? 1 : 0;
    c.eri = transform_route(t->layout, t->n, g.eri_s4 != 0);
    c.ip1 = transform_route(t->layout, t->n, (flags & EVC_FLAG_IP1_S2KL) != 0);
    return 0;
}


}  // namespace evc

using namespace evc;

extern "C" size_t evc_workspace_bytes(const evc_trdm_set *t, int natm) {
    return evc_workspace_bytes_batch(t, natm, 1);
}

extern "C" size_t evc_workspace_bytes_batch(const evc_trdm_set *t, int natm, int count) {
    if (check_set(t) || count < 1) return 0;
    return carve(t, natm, nullptr).bytes * (size_t)count;
}
