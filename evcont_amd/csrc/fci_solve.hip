// The vector work of a block Davidson eigensolver around evc_fci_sigma (fci_davidson.py), on CI vectors that stay on the
// device: sets of `dim`-long vectors stored as the rows of (count, ld) arrays, ld >= dim.
//   hdiag        <I|H|I> of the operator evc_fci_sigma applies, from three norb^2 tables and one energy per string
//   dots         out[i][j] = X_i . Y_j: up to 8 rows of X per pass of a row of Y, one partial per block of determinants,
//                the blocks added in order by a second launch
//   combine      Out_r = beta Out_r + sum_j coef[j][r] V_j, V read once for up to 8 outputs
//   correction   r_r = sum_j y_jr (W_j - theta_r V_j), |r_r|^2 and t_r = r_r / (hdiag - theta_r) in one pass over V and W
// Memory-bound streaming kernels without LDS tiles; the only LDS is the 8 x 4 doubles of a workgroup's reduction.  Every
// sum over the determinants uses the blocks of fci_rows_per_block(dim) and a fixed order inside a thread, a wave and a
// workgroup: the same bits for every grouping of the vectors and from run to run, and no atomics.
#include "common.hpp"
#include "kernels.hpp"

namespace evc {

constexpr int kSolveGroup = 8;       // vectors a thread accumulates for in one pass
constexpr int kSolveMaxVecs = 256;   // vectors per set in one call
constexpr int kHdiagTab = kFciMaxOrb * kFciMaxOrb;
constexpr int kHdiagFixed = kFciMaxOrb + 3 * kHdiagTab;   // doubles: hp | J | K | Jc, then one energy per string

// Launch through the runtime call (not the chevrons): tests/test_fci_solve_closure.py keeps the list of the kernels this
// file launches, kernel by kernel, against the records of EVC_PROF_FCI_SOLVE.
template <typename T>
struct same_type {
    using type = T;
};
template <typename... P>
static void solve_launch(void (*kernel)(P...), dim3 grid, hipStream_t st, typename same_type<P>::type... a) {
    void *args[] = {(void *)&a...};
    (void)hipLaunchKernel(reinterpret_cast<const void *>(kernel), grid, dim3(256), args, 0, st);
}

// ---- hdiag -----------------------------------------------------------------------
// hp[p] = h1[pp] - 1/2 sum_r (pr|rp), J[pr] = (pp|rr), K[pq] = (pq|qp), Jc[pr] = (J[pr] + J[rp]) / 2
__global__ __launch_bounds__(256) void fci_hdiag_prep_kernel(const double *__restrict__ h1,
                                                             const double *__restrict__ h2, int norb,
                                                             double *__restrict__ tabs) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= norb * norb) return;
    const int64_t n = norb, p = idx / norb, q = idx % norb;
    const double jpq = h2[((p * n + p) * n + q) * n + q], jqp = h2[((q * n + q) * n + p) * n + p];
    tabs[kFciMaxOrb + idx] = jpq;
    tabs[kFciMaxOrb + kHdiagTab + idx] = h2[((p * n + q) * n + q) * n + p];
    tabs[kFciMaxOrb + 2 * kHdiagTab + idx] = 0.5 * (jpq + jqp);
    if (q == 0) {
        double s = 0.0;
        for (int64_t r = 0; r < n; ++r) s += h2[((p * n + r) * n + r) * n + p];
        tabs[p] = h1[p * n + p] - 0.5 * s;
    }
}

// One thread per string of either spin: its occupation mask (orbital p is occupied iff E_pp keeps the string) and
//   e = sum_p hp[p] n_p + 1/2 sum_pr J[pr] n_p n_r + 1/2 sum_pq K[pq] n_p (1 - n_q)
__global__ __launch_bounds__(256) void fci_hdiag_string_kernel(const int32_t *__restrict__ tab_a,
                                                               const int32_t *__restrict__ tab_b, int norb, int npad,
                                                               int64_t na, int64_t nb, const double *__restrict__ tabs,
                                                               double *__restrict__ es, uint32_t *__restrict__ occ) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= na + nb) return;
    const int32_t *__restrict__ row = s < na ? tab_a + s * npad : tab_b + (s - na) * npad;
    uint32_t mask = 0;
    for (int p = 0; p < norb; ++p)
        if (row[p * norb + p] != 0) mask |= 1u << p;
    const double *__restrict__ J = tabs + kFciMaxOrb, *__restrict__ K = J + kHdiagTab;
    double e1 = 0.0, ej = 0.0, ek = 0.0;
    for (int p = 0; p < norb; ++p) {
        if (!(mask >> p & 1u)) continue;
        e1 += tabs[p];
        for (int q = 0; q < norb; ++q) {
            if (mask >> q & 1u) ej += J[p * norb + q];
            else ek += K[p * norb + q];
        }
    }
    es[s] = e1 + 0.5 * ej + 0.5 * ek;
    occ[s] = mask;
}

// hdiag(Ia, Ib) = e(Ia) + e(Ib) + sum_{p in Ia, r in Ib} Jc[pr]
__global__ __launch_bounds__(256) void fci_hdiag_det_kernel(int norb, int64_t na, int64_t nb,
                                                            const double *__restrict__ tabs,
                                                            const double *__restrict__ es,
                                                            const uint32_t *__restrict__ occ,
                                                            double *__restrict__ hdiag) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= na * nb) return;
    const int64_t ia = k / nb, ib = k % nb;
    const uint32_t ma = occ[ia], mb = occ[na + ib];
    const double *__restrict__ Jc = tabs + kFciMaxOrb + 2 * kHdiagTab;
    double s = 0.0;
    for (int p = 0; p < norb; ++p) {
        if (!(ma >> p & 1u)) continue;
        for (int r = 0; r < norb; ++r)
            if (mb >> r & 1u) s += Jc[p * norb + r];
    }
    hdiag[k] = (es[ia] + es[na + ib]) + s;
}

// ---- reductions over a block of determinants ---------------------------------------
// The workgroup's 256 threads hold up to 8 running sums each over the determinants k0 + t, k0 + t + 256, ...; wave_sum
// adds the lanes, thread r < count adds the four waves of value r and stores P[r * pitch].
__device__ __forceinline__ void solve_block_partials(const double (&acc)[kSolveGroup], int count, double *__restrict__ P,
                                                     int64_t pitch) {
    __shared__ double red[kSolveGroup][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < kSolveGroup; ++r) {
        const double v = wave_sum(acc[r]);
        if (lane == 0) red[r][wave] = v;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < count) P[t * pitch] = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
}

// P[(blk * nx + i) * ny + j] = sum over block blk of X_i Y_j; blockIdx = (blk, j, group of 8 rows of X)
__global__ __launch_bounds__(256) void fci_dots_kernel(const double *__restrict__ X, int64_t ldx, int nx,
                                                       const double *__restrict__ Y, int64_t ldy, int ny, int64_t dim,
                                                       int64_t rows, double *__restrict__ P) {
    const int64_t blk = blockIdx.x;
    const int j = blockIdx.y, i0 = blockIdx.z * kSolveGroup;
    const int ng = nx - i0 < kSolveGroup ? nx - i0 : kSolveGroup;
    const int64_t k0 = blk * rows, k1 = k0 + rows < dim ? k0 + rows : dim;
    const double *__restrict__ x = X + (int64_t)i0 * ldx, *__restrict__ y = Y + (int64_t)j * ldy;
    double acc[kSolveGroup];
#pragma unroll
    for (int i = 0; i < kSolveGroup; ++i) acc[i] = 0.0;
    for (int64_t k = k0 + threadIdx.x; k < k1; k += 256) {
        const double yv = y[k];
#pragma unroll
        for (int i = 0; i < kSolveGroup; ++i)
            if (i < ng) acc[i] = fma(x[(int64_t)i * ldx + k], yv, acc[i]);
    }
    solve_block_partials(acc, ng, P + (blk * nx + i0) * ny + j, ny);
}

// out[e] = sum over the blocks, in order, of P[blk * n + e]
__global__ __launch_bounds__(256) void fci_solve_reduce_kernel(const double *__restrict__ P, int64_t nblk, int n,
                                                               double *__restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
    for (int64_t b = 0; b < nblk; ++b) s += P[b * n + e];
    out[e] = s;
}

// ---- combine ---------------------------------------------------------------------
// Out_r[e] = beta Out_r[e] + sum_j coef[j * ldc + r] V_j[e], r < k <= 8; beta == 0 does not read Out
__global__ __launch_bounds__(256) void fci_combine_kernel(const double *__restrict__ V, int64_t ldv, int m,
                                                          const double *__restrict__ coef, int ldc, int k, double beta,
                                                          double *__restrict__ Out, int64_t ldo, int64_t dim) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= dim) return;
    double acc[kSolveGroup];
#pragma unroll
    for (int r = 0; r < kSolveGroup; ++r) acc[r] = (r < k && beta != 0.0) ? beta * Out[(int64_t)r * ldo + e] : 0.0;
    for (int j = 0; j < m; ++j) {
        const double v = V[(int64_t)j * ldv + e];
#pragma unroll
        for (int r = 0; r < kSolveGroup; ++r)
            if (r < k) acc[r] = fma(coef[(int64_t)j * ldc + r], v, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < kSolveGroup; ++r)
        if (r < k) Out[(int64_t)r * ldo + e] = acc[r];
}

// ---- Davidson correction -----------------------------------------------------------
// One workgroup per block of determinants, k <= 8 roots: x_r = sum_j y_jr V_j, s_r = sum_j y_jr W_j, r_r = s_r - theta_r
// x_r, T_r = r_r / d with d = hdiag - theta_r, |d| floored at 1e-8 keeping its sign (0 counts as positive);
// P[blk * kt + r] = the block's share of |r_r|^2.
__global__ __launch_bounds__(256) void fci_correction_kernel(const double *__restrict__ V, int64_t ldv,
                                                             const double *__restrict__ W, int64_t ldw, int m,
                                                             const double *__restrict__ coef, int ldc,
                                                             const double *__restrict__ theta, int k, int kt,
                                                             const double *__restrict__ hdiag, double *__restrict__ T,
                                                             int64_t ldt, int64_t dim, int64_t rows,
                                                             double *__restrict__ P) {
    const int64_t blk = blockIdx.x;
    const int64_t k0 = blk * rows, k1 = k0 + rows < dim ? k0 + rows : dim;
    double th[kSolveGroup], rsq[kSolveGroup];
#pragma unroll
    for (int r = 0; r < kSolveGroup; ++r) {
        th[r] = r < k ? theta[r] : 0.0;
        rsq[r] = 0.0;
    }
    for (int64_t e = k0 + threadIdx.x; e < k1; e += 256) {
        double ax[kSolveGroup], as[kSolveGroup];
#pragma unroll
        for (int r = 0; r < kSolveGroup; ++r) ax[r] = as[r] = 0.0;
        for (int j = 0; j < m; ++j) {
            const double v = V[(int64_t)j * ldv + e], w = W[(int64_t)j * ldw + e];
#pragma unroll
            for (int r = 0; r < kSolveGroup; ++r)
                if (r < k) {
                    const double c = coef[(int64_t)j * ldc + r];
                    ax[r] = fma(c, v, ax[r]);
                    as[r] = fma(c, w, as[r]);
                }
        }
        const double hd = hdiag[e];
#pragma unroll
        for (int r = 0; r < kSolveGroup; ++r)
            if (r < k) {
                const double res = fma(-th[r], ax[r], as[r]);
                rsq[r] = fma(res, res, rsq[r]);
                double d = hd - th[r];
                if (fabs(d) < 1e-8) d = d < 0.0 ? -1e-8 : 1e-8;
                T[(int64_t)r * ldt + e] = res / d;
            }
    }
    solve_block_partials(rsq, k, P + blk * kt, 1);
}

static void clear_solve_record() { note_kernel(EVC_PROF_FCI_SOLVE, "%s", ""); }

// [a, a + (n - 1) * ld + dim) and [b, ...) share a double
static bool sets_overlap(const double *a, int64_t na, int64_t lda, const double *b, int64_t nb, int64_t ldb, int64_t dim) {
    if (na < 1 || nb < 1) return false;
    const double *ae = a + (na - 1) * lda + dim, *be = b + (nb - 1) * ldb + dim;
    return a < be && b < ae;
}

static size_t hdiag_bytes(int64_t na, int64_t nb) {
    return align_up((size_t)(kHdiagFixed + na + nb) * 8 + (size_t)(na + nb) * 4, 256);
}

static int solve_dim(const char *who, int64_t dim) {
    EVC_REQUIRE(dim >= 1 && dim <= (int64_t)12870 * 12870, "%s: dim=%lld", who, (long long)dim);
    return 0;
}

}  // namespace evc

using namespace evc;

extern "C" size_t evc_fci_solve_workspace_bytes(int norb, int64_t na, int64_t nb, int nvec) {
    if (!(norb >= 1 && norb <= kFciMaxOrb && na >= 1 && nb >= 1 && na <= 12870 && nb <= 12870 && nvec >= 1 &&
          nvec <= kSolveMaxVecs)) {
        set_error("evc_fci_solve_workspace_bytes: norb=%d na=%lld nb=%lld nvec=%d (norb 1 ... %d, strings 1 ... 12870, "
                  "vectors 1 ... %d)", norb, (long long)na, (long long)nb, nvec, kFciMaxOrb, kSolveMaxVecs);
        return 0;
    }
    const int64_t dim = na * nb, nblk = ceil_div(dim, fci_rows_per_block(dim));
    const size_t d = align_up((size_t)nblk * nvec * nvec * 8, 256), h = hdiag_bytes(na, nb);
    return d > h ? d : h;
}

extern "C" int evc_fci_hdiag(int norb, int64_t na, int64_t nb, const int32_t *tab_a, const int32_t *tab_b,
                             const double *h1, const double *h2, double *hdiag, void *ws, size_t ws_bytes, void *stream) {
    EVC_REQUIRE(norb >= 1 && norb <= kFciMaxOrb, "evc_fci_hdiag: norb=%d, supported 1 ... %d", norb, kFciMaxOrb);
    EVC_REQUIRE(na >= 1 && nb >= 1 && na <= 12870 && nb <= 12870, "evc_fci_hdiag: na=%lld nb=%lld strings (1 ... 12870 each)",
                (long long)na, (long long)nb);
    EVC_REQUIRE(tab_a && tab_b && h1 && h2 && hdiag && ws, "evc_fci_hdiag: null pointer");
    EVC_REQUIRE(aligned16(ws), "evc_fci_hdiag: workspace not 16-byte aligned");
    EVC_REQUIRE(ws_bytes >= hdiag_bytes(na, nb), "evc_fci_hdiag: workspace of %zu bytes, %zu needed", ws_bytes,
                hdiag_bytes(na, nb));
    hipStream_t st = as_stream(stream);
    clear_solve_record();
    const int npad = (norb * norb + 15) / 16 * 16;
    double *tabs = static_cast<double *>(ws), *es = tabs + kHdiagFixed;
    uint32_t *occ = reinterpret_cast<uint32_t *>(es + na + nb);
    solve_launch(fci_hdiag_prep_kernel, dim3((unsigned)ceil_div(norb * norb, 256)), st, h1, h2, norb, tabs);
    EVC_LAUNCH_CHECK("fci_hdiag_prep_kernel");
    solve_launch(fci_hdiag_string_kernel, dim3((unsigned)ceil_div(na + nb, 256)), st, tab_a, tab_b, norb, npad, na, nb,
                 tabs, es, occ);
    EVC_LAUNCH_CHECK("fci_hdiag_string_kernel");
    solve_launch(fci_hdiag_det_kernel, dim3((unsigned)ceil_div(na * nb, 256)), st, norb, na, nb, tabs, es, occ, hdiag);
    EVC_LAUNCH_CHECK("fci_hdiag_det_kernel");
    note_kernel(EVC_PROF_FCI_SOLVE, "fci_hdiag_prep_kernel + fci_hdiag_string_kernel strings=%lld + fci_hdiag_det_kernel",
                (long long)(na + nb));
    return 0;
}

extern "C" int evc_fci_dots(int64_t dim, const double *X, int64_t ldx, int nx, const double *Y, int64_t ldy, int ny,
                            double *out, void *ws, size_t ws_bytes, void *stream) {
    if (int rc = solve_dim("evc_fci_dots", dim)) return rc;
    EVC_REQUIRE(X && Y && out && ws, "evc_fci_dots: null pointer");
    EVC_REQUIRE(nx >= 1 && nx <= kSolveMaxVecs && ny >= 1 && ny <= kSolveMaxVecs, "evc_fci_dots: nx=%d ny=%d (1 ... %d each)",
                nx, ny, kSolveMaxVecs);
    EVC_REQUIRE(ldx >= dim && ldy >= dim, "evc_fci_dots: ldx=%lld ldy=%lld for %lld determinants", (long long)ldx,
                (long long)ldy, (long long)dim);
    EVC_REQUIRE(aligned16(ws), "evc_fci_dots: workspace not 16-byte aligned");
    const int64_t rows = fci_rows_per_block(dim), nblk = ceil_div(dim, rows);
    const size_t need = (size_t)nblk * nx * ny * 8;
    EVC_REQUIRE(ws_bytes >= need, "evc_fci_dots: workspace of %zu bytes, %zu needed for %d x %d products in %lld blocks",
                ws_bytes, need, nx, ny, (long long)nblk);
    hipStream_t st = as_stream(stream);
    clear_solve_record();
    double *P = static_cast<double *>(ws);
    const int groups = (int)ceil_div(nx, kSolveGroup);
    solve_launch(fci_dots_kernel, dim3((unsigned)nblk, (unsigned)ny, (unsigned)groups), st, X, ldx, nx, Y, ldy, ny, dim,
                 rows, P);
    EVC_LAUNCH_CHECK("fci_dots_kernel");
    solve_launch(fci_solve_reduce_kernel, dim3((unsigned)ceil_div(nx * ny, 256)), st, P, nblk, nx * ny, out);
    EVC_LAUNCH_CHECK("fci_solve_reduce_kernel");
    note_kernel(EVC_PROF_FCI_SOLVE, "fci_dots_kernel nx=%d ny=%d groups=%d blocks=%lld + fci_solve_reduce_kernel", nx, ny,
                groups, (long long)nblk);
    return 0;
}

extern "C" int evc_fci_combine(int64_t dim, const double *V, int64_t ldv, int m, const double *coef, int ldc, int k,
                               double beta, double *Out, int64_t ldo, void *stream) {
    if (int rc = solve_dim("evc_fci_combine", dim)) return rc;
    EVC_REQUIRE(m >= 0 && m <= kSolveMaxVecs && k >= 1 && k <= kSolveMaxVecs, "evc_fci_combine: m=%d (0 ... %d) k=%d (1 ... %d)",
                m, kSolveMaxVecs, k, kSolveMaxVecs);
    EVC_REQUIRE(Out && (m == 0 || (V && coef)), "evc_fci_combine: null pointer");
    EVC_REQUIRE(ldo >= dim && (m == 0 || (ldv >= dim && ldc >= k)), "evc_fci_combine: ldv=%lld ldo=%lld ldc=%d for %lld "
                "determinants and %d outputs", (long long)ldv, (long long)ldo, ldc, (long long)dim, k);
    EVC_REQUIRE(!sets_overlap(Out, k, ldo, V, m, ldv, dim), "evc_fci_combine: Out must not alias V");
    hipStream_t st = as_stream(stream);
    clear_solve_record();
    for (int r0 = 0; r0 < k; r0 += kSolveGroup) {
        const int kk = k - r0 < kSolveGroup ? k - r0 : kSolveGroup;
        solve_launch(fci_combine_kernel, dim3((unsigned)ceil_div(dim, 256)), st, V, ldv, m, coef ? coef + r0 : coef, ldc, kk, beta,
                     Out + (int64_t)r0 * ldo, ldo, dim);
        EVC_LAUNCH_CHECK("fci_combine_kernel");
    }
    note_kernel(EVC_PROF_FCI_SOLVE, "fci_combine_kernel m=%d k=%d groups=%d", m, k, (int)ceil_div(k, kSolveGroup));
    return 0;
}

extern "C" int evc_fci_davidson_correction(int64_t dim, const double *V, int64_t ldv, const double *W, int64_t ldw, int m,
                                           const double *coef, int ldc, const double *theta, int k, const double *hdiag,
                                           double *T, int64_t ldt, double *rnorm2, void *ws, size_t ws_bytes,
                                           void *stream) {
    if (int rc = solve_dim("evc_fci_davidson_correction", dim)) return rc;
    EVC_REQUIRE(V && W && coef && theta && hdiag && T && rnorm2 && ws, "evc_fci_davidson_correction: null pointer");
    EVC_REQUIRE(m >= 1 && m <= kSolveMaxVecs && k >= 1 && k <= kSolveMaxVecs,
                "evc_fci_davidson_correction: m=%d k=%d (1 ... %d each)", m, k, kSolveMaxVecs);
    EVC_REQUIRE(ldv >= dim && ldw >= dim && ldt >= dim && ldc >= k, "evc_fci_davidson_correction: ldv=%lld ldw=%lld ldt=%lld "
                "ldc=%d for %lld determinants and %d roots", (long long)ldv, (long long)ldw, (long long)ldt, ldc,
                (long long)dim, k);
    EVC_REQUIRE(!sets_overlap(T, k, ldt, V, m, ldv, dim) && !sets_overlap(T, k, ldt, W, m, ldw, dim) &&
                    !sets_overlap(T, k, ldt, hdiag, 1, dim, dim),
                "evc_fci_davidson_correction: T must not alias V, W or hdiag");
    EVC_REQUIRE(aligned16(ws), "evc_fci_davidson_correction: workspace not 16-byte aligned");
    const int64_t rows = fci_rows_per_block(dim), nblk = ceil_div(dim, rows);
    const size_t need = (size_t)nblk * k * 8;
    EVC_REQUIRE(ws_bytes >= need, "evc_fci_davidson_correction: workspace of %zu bytes, %zu needed", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    clear_solve_record();
    double *P = static_cast<double *>(ws);
    for (int r0 = 0; r0 < k; r0 += kSolveGroup) {
        const int kk = k - r0 < kSolveGroup ? k - r0 : kSolveGroup;
        solve_launch(fci_correction_kernel, dim3((unsigned)nblk), st, V, ldv, W, ldw, m, coef + r0, ldc, theta + r0, kk, k,
                     hdiag, T + (int64_t)r0 * ldt, ldt, dim, rows, P + r0);
        EVC_LAUNCH_CHECK("fci_correction_kernel");
    }
    solve_launch(fci_solve_reduce_kernel, dim3((unsigned)ceil_div(k, 256)), st, P, nblk, k, rnorm2);
    EVC_LAUNCH_CHECK("fci_solve_reduce_kernel");
    note_kernel(EVC_PROF_FCI_SOLVE, "fci_correction_kernel m=%d k=%d groups=%d blocks=%lld + fci_solve_reduce_kernel", m, k,
                (int)ceil_div(k, kSolveGroup), (long long)nblk);
    return 0;
}
