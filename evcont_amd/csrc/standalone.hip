// Stand-alone entry points beside the pipeline: the subspace solve, the OAO integrals of a batch, the electronic gradient
// of given RDMs.
#include "pipeline.hpp"

using namespace evc;

extern "C" size_t evc_subspace_solve_ws_bytes(int T, int count) {
    if (T <= kSubspaceSmallT || T > kSubspaceMaxT || count < 1) return 0;
    return sizeof(double) * subspace_big_scratch_doubles(T) * (size_t)count;
}

extern "C" int evc_subspace_solve(const double *h1rows, const double *h2rows, const double *S_train, int T,
                                  int layout, int nroots, double e_shift, double *evals, double *evecs,
                                  double *w2, double *w1, double *Hout, void *ws, size_t ws_bytes, void *stream) {
    EVC_REQUIRE(h1rows && h2rows && S_train && evals && evecs, "evc_subspace_solve: null pointer");
    EVC_REQUIRE(T >= 1 && T <= kSubspaceMaxT, "evc_subspace_solve: T=%d out of range 1..%d", T, kSubspaceMaxT);
    EVC_REQUIRE(T <= kSubspaceSmallT || (ws && aligned16(ws) && ws_bytes >= evc_subspace_solve_ws_bytes(T, 1)),
                "evc_subspace_solve: T=%d needs a workspace of evc_subspace_solve_ws_bytes(T, 1) bytes", T);
    EVC_REQUIRE(layout == 6 || layout == 5 || layout == 3 || layout == 2 || layout == EVC_LAYOUT_SYM8,
                "evc_subspace_solve: layout=%d", layout);
    EVC_REQUIRE(nroots >= 1 && nroots <= T, "evc_subspace_solve: nroots=%d out of range", nroots);
    SolveArgs a;
    memset(&a, 0, sizeof(a));
    a.h1part = h1rows;
    a.nsp1 = 1;
    a.alpha1 = 1.0;
    a.h2part = h2rows;
    a.nsp2 = 1;
    a.alpha2 = 1.0;
    a.S = S_train;
    a.T = T;
    a.layout = layout;
    a.nroots = nroots;
    a.e_shift = e_shift;
    a.evals = evals;
    a.evecs = evecs;
    a.w2 = w2;
    a.w1 = w1;
    a.Hout = Hout;
    a.w2_offset = 0;
    a.w2_count = layout_pairs(layout) ? (int64_t)T * (T + 1) / 2 : (int64_t)T * T;
    a.scratch = static_cast<double *>(ws);
    return launch_subspace_solve(a, 1, as_stream(stream));
}

extern "C" int evc_subspace_solve_batch(const double *H, const double *S, int64_t s_stride, int T, int count,
                                        int nroots, const double *e_shift, double *evals, double *evecs,
                                        void *ws, size_t ws_bytes, void *stream) {
    EVC_REQUIRE(H && S && evals && evecs, "evc_subspace_solve_batch: null pointer");
    EVC_REQUIRE(T >= 1 && T <= kSubspaceMaxT, "evc_subspace_solve_batch: T=%d out of range 1..%d", T, kSubspaceMaxT);
    EVC_REQUIRE(T <= kSubspaceSmallT || (ws && aligned16(ws) && ws_bytes >= evc_subspace_solve_ws_bytes(T, count)),
                "evc_subspace_solve_batch: T=%d needs a workspace of evc_subspace_solve_ws_bytes(T, count) bytes", T);
    EVC_REQUIRE(count >= 1 && count <= (1 << 24), "evc_subspace_solve_batch: count=%d out of range", count);
    EVC_REQUIRE(nroots >= 1 && nroots <= T, "evc_subspace_solve_batch: nroots=%d out of range", nroots);
    EVC_REQUIRE(s_stride == 0 || s_stride >= (int64_t)T * T, "evc_subspace_solve_batch: s_stride=%lld",
                (long long)s_stride);
    SolveArgs a;
    memset(&a, 0, sizeof(a));
    a.h1part = H;  // the assembled matrix plays the role of the (single) one-body partial
    a.nsp1 = 1;
    a.alpha1 = 1.0;
    a.sh1 = (int64_t)T * T;
    a.h2part = nullptr;
    a.nsp2 = 0;
    a.S = S;
    a.sS = s_stride;
    a.T = T;
    a.layout = EVC_LAYOUT_FULL6;
    a.nroots = nroots;
    a.e_shift_dev = e_shift;
    a.evals = evals;
    a.sev = T;
    a.evecs = evecs;
    a.svec = (int64_t)T * T;
    a.scratch = static_cast<double *>(ws);
    a.sscratch = T > kSubspaceSmallT ? (int64_t)subspace_big_scratch_doubles(T) : 0;
    return launch_subspace_solve(a, count, as_stream(stream));
}

// Workspace of evc_integrals_oao_batch per geometry: X, U, s, h1 (Loewdin outputs) + one N^4 buffer.
// Layout inside one stride (every piece starts on a 16-byte boundary): [X | U | s | h1 | B1 (n^4)].
static int64_t even_up(int64_t x) { return (x + 1) & ~(int64_t)1; }
static int64_t integrals_ws_stride(int n) {
    const int64_t n2 = (int64_t)n * n;
    return 3 * even_up(n2) + even_up(n) + even_up(n2 * n2);
}

extern "C" size_t evc_integrals_oao_ws_bytes(int n, int count) {
    if (n < 1 || n > kMaxOrbitals || count < 1) return 0;
    return sizeof(double) * (size_t)integrals_ws_stride(n) * (size_t)count;
}

extern "C" int evc_integrals_oao_batch(int n, int count, const double *S, const double *hcore, const double *eri,
                                       double *h1, double *h2, double *trafo, void *ws, size_t ws_bytes,
                                       void *stream) {
    EVC_REQUIRE(S && hcore && eri && h1 && h2 && ws, "evc_integrals_oao_batch: null pointer");
    EVC_REQUIRE(n >= 1 && n <= kMaxOrbitals, "evc_integrals_oao_batch: n=%d out of range 1..%d", n, kMaxOrbitals);
    EVC_REQUIRE(count >= 1 && count <= 65535, "evc_integrals_oao_batch: count=%d out of range", count);
    EVC_REQUIRE(aligned16(ws) && ws_bytes >= evc_integrals_oao_ws_bytes(n, count),
                "evc_integrals_oao_batch: workspace misaligned or too small");
    hipStream_t st = as_stream(stream);
    const int64_t n2 = (int64_t)n * n, n4 = n2 * n2, sw = integrals_ws_stride(n);
    double *base = static_cast<double *>(ws);
    double *X = base, *U = X + even_up(n2), *s = U + even_up(n2), *h1w = s + even_up(n), *B1 = h1w + even_up(n2);
    LoewdinArgs la{};
    la.S = S;
    la.h = hcore;
    la.X = X;
    la.U = U;
    la.s = s;
    la.h1 = h1w;
    la.sS = n2;
    la.sh = n2;
    la.sws = sw;
    la.n = n;
    la.scratch = B1;   // (the N^4 buffer is free until the rotation)
    la.sscratch = sw;
    EVC_TRY(launch_loewdin(la, count, st));
    EVC_TRY(rotate_four_index(transform_route(EVC_LAYOUT_FULL6, n, false).steps, eri, n4, X, sw, 0, n, B1, sw, h2, n4, count,
                                st));
    hipError_t e = hipMemcpy2DAsync(h1, sizeof(double) * n2, h1w, sizeof(double) * sw, sizeof(double) * n2, count,
                                    hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && trafo)
        e = hipMemcpy2DAsync(trafo, sizeof(double) * n2, X, sizeof(double) * sw, sizeof(double) * n2, count,
                             hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
        set_error("evc_integrals_oao_batch: copy failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

// The set of evc_grad_elec_oao: one training state of the full layout (workspace size and carving of that call).
static void fake_set(evc_trdm_set &t, int n) {
    memset(&t, 0, sizeof(t));
    t.n = n;
    t.ntrain = 1;
    t.layout = EVC_LAYOUT_FULL6;
    t.rows2_total = 1;
    t.cols2 = (int64_t)n * n * n * n;
    t.ld2 = t.cols2 + (t.cols2 & 1);
    t.ld1 = (int64_t)n * n + ((n * n) & 1);
}

extern "C" size_t evc_grad_elec_ws_bytes(int n, int natm) {
    if (n < 1 || n > kMaxOrbitals) return 0;
    evc_trdm_set t;
    fake_set(t, n);
    return carve(&t, natm, nullptr).bytes;
}

extern "C" int evc_grad_elec_oao(int n, const evc_geometry *g, const double *trafo, const double *one_rdm,
                                 const double *two_rdm, double *grad, void *ws, size_t ws_bytes, void *stream) {
    EVC_REQUIRE(n >= 1 && n <= kMaxOrbitals, "evc_grad_elec_oao: n=%d out of range 1..%d", n, kMaxOrbitals);
    Geo geo = geo_single(g);
    if (check_geometry("evc_grad_elec_oao", geo, true)) return -1;
    EVC_REQUIRE(one_rdm && two_rdm && grad, "evc_grad_elec_oao: null pointer");
    evc_trdm_set t;
    fake_set(t, n);
    Call c;
    if (setup("evc_grad_elec_oao", &t, geo, 0, ws, ws_bytes, 1, c)) return -1;
    const Ws &w = c.w;
    hipStream_t st = as_stream(stream);
    EVC_TRY(launch_loewdin(loewdin_args(n, geo, c), 1, st));
    if (trafo) {
        // caller-supplied ao_mo_trafo (gradients_loewdin.py:271-272); its derivative is still the
        // Loewdin response of g->S, exactly as the reference computes it when none is passed (:274-277)
        hipError_t e = hipMemcpyAsync(w.X, trafo, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) {
            set_error("evc_grad_elec_oao: copy failed: %s", hipGetErrorString(e));
            return (int)e;
        }
    }
    EVC_TRY(launch_quarter_transform(g->eri, 0, w.X, 0, 0, n, w.B1, 0, 1, st));
    EVC_TRY(launch_quarter_transform(w.B1, 0, w.X, 0, 0, n, w.B2, 0, 1, st));
    EVC_TRY(launch_quarter_transform(w.B2, 0, w.X, 0, 0, n, w.K3, 0, 1, st));
    return gradient_unpacked(GradCall{n, geo, c, st, one_rdm, 0, 1.0, false, grad, 0}, two_rdm, 0);
}
