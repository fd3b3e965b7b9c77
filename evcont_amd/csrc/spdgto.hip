// AO integrals and their first nuclear derivatives of a molecule built from contracted s, p and REAL SPHERICAL d Gaussian
// shells (evc_spdgto_integrals_batch, evc_spdgto_dipole_batch): the device statement of evcont_amd/gto_spd.py
// spd_gaussian_mol, written straight into the arrays of an evc_geometry_batch.  spgto.hip stays the route for molecules of
// s and p shells alone, sgto.hip for one s function per centre.
//
// Scheme: that of spgto.hip (McMurchie-Davidson with the Hermite Coulomb integrals kept factored per dimension), with
// general powers 0 ... 2 per dimension and function.  A contracted function is a sum over (primitive x monomial) with
// constant weights (spd_mono): s and p have one monomial, d_xy, d_yz, d_xz one, d_{x^2-y^2} two and d_{2z^2-x^2-y^2} three;
// the thread that owns a contracted element loops over the monomials of its functions, so there is no transformation pass
// over int2e and the Cartesian combination x^2 + y^2 + z^2 never appears.  Per dimension the Hermite coefficients come from
// power-raising steps run up to the HIGHEST powers with the wanted row picked by selects (spd_bra_dim, spd_ket_dim): every
// loop has fixed bounds and no register array is indexed at run time.  Orders: the bra reaches t <= 5 (2 + 2 and the
// centre derivative), the ket tau <= 4, their fold n <= 9 (8 without the gradient); Boys functions F0 ... F9 (F0 ... F8
// under EVC_FLAG_ENERGY_ONLY, F0 ... F5 / F0 ... F4 for the attraction).  The three components of int2e_ip1 are computed
// in turn from the kept arrays of the other two dimensions.
// Boys functions (gto_boys, shared with spgto.hip): below t = 12 the convergent series of the highest order, then downward
// recursion; above it F0 from erf and upward recursion.
//
// Kernels, each a launch of its own (FP64 VALU; DESIGN.md: FP64 MFMA blocks its SIMD's vector issue), the cut of spgto.hip:
//   spdgto_pair_kernel    the primitive-pair table (one row of kGtoRow doubles per ordered pair of primitive entries).
//   spdgto_one_kernel     one thread per contracted pair mu >= nu: S, hcore (mirrored), ipovlp, dhcore.
//   spdgto_nuc_kernel     nuclear repulsion and its gradient, one thread per centre.
//   spdgto_two_kernel     one thread per (mu nu | kappa >= lambda); primitive quartets in one fixed order (ket pair outer,
//                         bra pair inner), inside a quartet the monomials in one fixed order (ket outer, bra inner).
//                         No screening: every quartet is evaluated.
//   spdgto_dipole_kernel  <mu| r - origin |nu>, one thread per contracted pair mu >= nu, mirrored.
// No sum is split across threads and there are no read-modify-write operations between threads: the same bits from run to
// run and for every batch size, and the full forms are the unpacked packed forms.
// The basis is a HOST argument and reaches the kernels by value.
// What lives where: as in spgto.hip.  gto_shells.hpp holds what the two routes share (limits, GtoPrims, gto_boys, gto_raise,
// gto_conv, gto_dot, gto_overlap_kinetic, the pair-table body, the whole host side), told about this route by SpdRoute at
// the end of the file, and the monomials of the d functions (spd_mono, also read by field.hip).  Here: the maths of the powers 0 ... 2 (spd_bra_dim, spd_ket_dim, spd_fold, spd_poly,
// spd_os_table, spd_st_dim, the one / two / dipole bodies) and the kernels.
#include "gto_shells.hpp"

namespace evc {

struct SpdPrims : GtoPrims {};
struct SpdAos {
    uint8_t off[kGtoMaxAo];      // first primitive of the function's shell
    uint8_t np[kGtoMaxAo];       // primitives of the shell
    uint8_t kind[kGtoMaxAo];     // 0: s; 1, 2, 3: p_x, p_y, p_z; 4 ... 8: d_xy, d_yz, d_z2, d_xz, d_x2-y2
    uint8_t atom[kGtoMaxAo];
};

// (the monomials of a function, spd_nmono / spd_mono, and the select spd_sel3: gto_shells.hpp, shared with field.hip)

// ---- Hermite coefficients of one dimension ---------------------------------------------------
// Hermite coefficients (t <= 5) of one dimension of a primitive pair with the powers i, j (0 ... 2), without the
// exponential: `base` = E^{ij}, `der` = those of d/dA, 2a E^{i+1,j} - i E^{i-1,j}.  XA = P - A, XB = P - B, ip = 1 / 2p.
// All raising steps run; the rows are picked by selects.
GTO_HD void spd_bra_dim(int i, int j, double a, double XA, double XB, double ip, double (&base)[6], double (&der)[6]) {
    const double e0[6] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double b1[6], b2[6], ej[6], a1[6], a2[6], a3[6];
    gto_raise(e0, XB, ip, b1);
    gto_raise(b1, XB, ip, b2);
#pragma unroll
    for (int t = 0; t < 6; ++t) ej[t] = spd_sel3(j, e0[t], b1[t], b2[t]);
    gto_raise(ej, XA, ip, a1);
    gto_raise(a1, XA, ip, a2);
    gto_raise(a2, XA, ip, a3);
    const double ax2 = 2.0 * a, di = (double)i;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        base[t] = spd_sel3(i, ej[t], a1[t], a2[t]);
        der[t] = ax2 * spd_sel3(i, a1[t], a2[t], a3[t]) - di * spd_sel3(i, 0.0, ej[t], a1[t]);
    }
}

// (-1)^tau E^{kl}_tau (tau <= 4) of one dimension of the ket pair, powers k, l (0 ... 2).
GTO_HD void spd_ket_dim(int k, int l, double XC, double XD, double ip, double (&o)[5]) {
    const double e0[5] = {1.0, 0.0, 0.0, 0.0, 0.0};
    double d1[5], d2[5], el[5], c1[5], c2[5];
    gto_raise(e0, XD, ip, d1);
    gto_raise(d1, XD, ip, d2);
#pragma unroll
    for (int t = 0; t < 5; ++t) el[t] = spd_sel3(l, e0[t], d1[t], d2[t]);
    gto_raise(el, XC, ip, c1);
    gto_raise(c1, XC, ip, c2);
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const double v = spd_sel3(k, el[t], c1[t], c2[t]);
        o[t] = (t & 1) ? -v : v;
    }
}

// c[n] = sum_{t + tau = n} b[t] k[tau], n <= M.
template <int M>
GTO_HD void spd_fold(const double (&b)[6], const double (&k)[5], double (&c)[M + 1]) {
#pragma unroll
    for (int n = 0; n <= M; ++n) {
        double s = 0.0;
#pragma unroll
        for (int tau = 0; tau < 5; ++tau)
            if (n - tau >= 0 && n - tau < 6) s = fma(b[n - tau], k[tau], s);
        c[n] = s;
    }
}

// the first M + 1 entries of a bra array
template <int M>
GTO_HD void spd_take(const double (&b)[6], double (&c)[M + 1]) {
#pragma unroll
    for (int n = 0; n <= M; ++n) c[n] = b[n];
}

// a_{n,j} = n! / ((n - j)! (2j - n)! 2^{n - j}), j <= n <= 2j
constexpr double spd_factorial(int n) { return n <= 1 ? 1.0 : n * spd_factorial(n - 1); }
constexpr double spd_poly_coef(int n, int j) {
    return spd_factorial(n) / (spd_factorial(n - j) * spd_factorial(2 * j - n) * (double)(1 << (n - j)));
}

// A[j] = sum_n c[n] a_{n,j} X^{2j - n}: the derivatives d^n/dX^n of a function of alpha |R|^2 as raises of its order.
template <int M>
GTO_HD void spd_poly(const double (&c)[M + 1], double X, double (&A)[M + 1]) {
    double Xp[M + 1];
    Xp[0] = 1.0;
#pragma unroll
    for (int k = 1; k <= M; ++k) Xp[k] = Xp[k - 1] * X;
#pragma unroll
    for (int j = 0; j <= M; ++j) {
        double s = 0.0;
#pragma unroll
        for (int n = j; n <= M; ++n)
            if (n <= 2 * j) s = fma(c[n] * spd_poly_coef(n, j), Xp[2 * j - n], s);
        A[j] = s;
    }
}

// ---- pair table ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spdgto_pair_kernel(SpdPrims bs, const double *__restrict__ coords, int natm, int nprim,
                                                           double *__restrict__ tab) {
    gto_pair_body(blockIdx.x * 256 + threadIdx.x, blockIdx.y, bs, coords, natm, nprim, tab);
}

// ---- two-electron integrals ----------------------------------------------------------------
// M: the highest Hermite order, 9 with the gradient and 8 without.
template <bool GRAD>
GTO_HD void spd_two_body(int mu, int nu, int v, int g, const SpdAos &ao, const double *tab, int N, int nprim, int s4,
                         int s2kl, double *eri, double *ip1) {
    constexpr int M = GRAD ? 9 : 8;
    const int Ms = N * (N + 1) / 2;
    if (v >= Ms) return;
    const int kap = gto_tri_row(v), lam = v - kap * (kap + 1) / 2;
    const double *tg = tab + (int64_t)g * nprim * nprim * kGtoRow;
    const int km = ao.kind[mu], kn = ao.kind[nu], kk = ao.kind[kap], kl = ao.kind[lam];
    const int nm = spd_nmono(km), nn = spd_nmono(kn), nk = spd_nmono(kk), nl = spd_nmono(kl);
    double acc = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    for (int pc = ao.off[kap]; pc < ao.off[kap] + ao.np[kap]; ++pc)
        for (int pd = ao.off[lam]; pd < ao.off[lam] + ao.np[lam]; ++pd) {
            const double *kr = tg + ((int64_t)pc * nprim + pd) * kGtoRow;
            const double q = kr[0], qx = kr[1], qy = kr[2], qz = kr[3], ck = kr[4];
            for (int pa = ao.off[mu]; pa < ao.off[mu] + ao.np[mu]; ++pa)
                for (int pb = ao.off[nu]; pb < ao.off[nu] + ao.np[nu]; ++pb) {
                    const double *br = tg + ((int64_t)pa * nprim + pb) * kGtoRow;
                    const double p = br[0], X[3] = {br[1] - qx, br[2] - qy, br[3] - qz};
                    const double s = p + q, pq = p * q;
                    const double alpha = pq / s;
                    double H[M + 1];
                    gto_boys<M>(alpha * (X[0] * X[0] + X[1] * X[1] + X[2] * X[2]), H);
                    double w = 34.986836655249725 / (pq * sqrt(s)) * br[4] * ck;   // 2 pi^2.5
#pragma unroll
                    for (int m = 0; m <= M; ++m) {
                        H[m] = H[m] * w;
                        w = w * (-2.0 * alpha);
                    }
                    for (int ik = 0; ik < nk; ++ik)
                        for (int il = 0; il < nl; ++il) {
                            int pk[3], pl[3];
                            double wk, wl;
                            spd_mono(kk, ik, pk[0], pk[1], pk[2], wk);
                            spd_mono(kl, il, pl[0], pl[1], pl[2], wl);
                            double ek[3][5];
#pragma unroll
                            for (int x = 0; x < 3; ++x) spd_ket_dim(pk[x], pl[x], kr[8 + x], kr[11 + x], kr[7], ek[x]);
                            for (int im = 0; im < nm; ++im)
                                for (int in = 0; in < nn; ++in) {
                                    int pm[3], pn[3];
                                    double wm, wn;
                                    spd_mono(km, im, pm[0], pm[1], pm[2], wm);
                                    spd_mono(kn, in, pn[0], pn[1], pn[2], wn);
                                    const double wt = (wk * wl) * (wm * wn);
                                    double A[3][M + 1], der[3][6];
#pragma unroll
                                    for (int x = 0; x < 3; ++x) {
                                        double base[6], c[M + 1];
                                        spd_bra_dim(pm[x], pn[x], br[5], br[8 + x], br[11 + x], br[7], base, der[x]);
                                        spd_fold<M>(base, ek[x], c);
                                        spd_poly<M>(c, X[x], A[x]);
                                    }
                                    double yz[M + 1];
                                    gto_conv<M>(A[1], A[2], yz);
                                    acc = acc + wt * gto_dot<M>(H, A[0], yz);
                                    if (GRAD) {
                                        // electron gradient = - centre gradient; one direction at a time
                                        double c[M + 1], D[M + 1], oth[M + 1];
                                        spd_fold<M>(der[0], ek[0], c);
                                        spd_poly<M>(c, X[0], D);
                                        gx = gx - wt * gto_dot<M>(H, D, yz);
                                        spd_fold<M>(der[1], ek[1], c);
                                        spd_poly<M>(c, X[1], D);
                                        gto_conv<M>(A[0], A[2], oth);
                                        gy = gy - wt * gto_dot<M>(H, D, oth);
                                        spd_fold<M>(der[2], ek[2], c);
                                        spd_poly<M>(c, X[2], D);
                                        gto_conv<M>(A[0], A[1], oth);
                                        gz = gz - wt * gto_dot<M>(H, D, oth);
                                    }
                                }
                        }
                }
        }
    const int64_t n2 = (int64_t)N * N, kl2 = (int64_t)kap * N + lam, lk2 = (int64_t)lam * N + kap;
    if (GRAD) {
        const double gv[3] = {gx, gy, gz};
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const int64_t row = ((int64_t)g * 3 + x) * n2 + (int64_t)mu * N + nu;
            if (s2kl) {
                ip1[row * Ms + v] = gv[x];
            } else {
                ip1[row * n2 + kl2] = gv[x];
                ip1[row * n2 + lk2] = gv[x];
            }
        }
    }
    if (mu < nu) return;
    if (s4) {
        eri[((int64_t)g * Ms + mu * (mu + 1) / 2 + nu) * Ms + v] = acc;
    } else {
        double *eg = eri + (int64_t)g * n2 * n2;
        const int64_t mn = ((int64_t)mu * N + nu) * n2, nm2 = ((int64_t)nu * N + mu) * n2;
        eg[mn + kl2] = acc;
        eg[mn + lk2] = acc;
        eg[nm2 + kl2] = acc;
        eg[nm2 + lk2] = acc;
    }
}

// GRAD: gridDim.y = N^2, blockIdx.y = mu N + nu; otherwise gridDim.y = Ms, blockIdx.y = mu (mu + 1) / 2 + nu.
// s4 / s2kl: the forms of eri / eri_ip1 (EVC_FLAG_ERI_S4 / EVC_FLAG_IP1_S2KL).
template <bool GRAD>
__global__ __launch_bounds__(64) void spdgto_two_kernel(SpdAos ao, const double *__restrict__ tab, int N, int nprim, int s4,
                                                         int s2kl, double *__restrict__ eri, double *__restrict__ ip1) {
    const int by = blockIdx.y;
    int mu, nu;
    if (GRAD) {
        mu = by / N;
        nu = by - mu * N;
    } else {
        mu = gto_tri_row(by);
        nu = by - mu * (mu + 1) / 2;
    }
    spd_two_body<GRAD>(mu, nu, blockIdx.x * 64 + threadIdx.x, blockIdx.z, ao, tab, N, nprim, s4, s2kl, eri, ip1);
}

// ---- one-electron integrals ------------------------------------------------------------------
// One dimension of overlap and kinetic energy of a primitive pair with the powers i, j (0 ... 2), without the factor
// sqrt(pi / p) and the exponential: s(i', j') by the Obara-Saika recursion for i' <= 3, j' <= 4, then
//   out[0], out[1]   the overlap and -1/2 d^2/dx^2 on the second function,
//                    4 b^2 s(i, j+2) - 2 b (2j + 1) s(i, j) + j (j - 1) s(i, j-2)
//   out[2], out[3]   their derivatives for the centre of the first function, 2a (i + 1) - i (i - 1)
GTO_HD void spd_os_table(double XA, double XB, double ip, double (&s)[4][5]) {
    s[0][0] = 1.0;
#pragma unroll
    for (int jj = 1; jj < 5; ++jj) s[0][jj] = XB * s[0][jj - 1] + (jj > 1 ? ip * (jj - 1) * s[0][jj - 2] : 0.0);
#pragma unroll
    for (int ii = 1; ii < 4; ++ii)
#pragma unroll
        for (int jj = 0; jj < 5; ++jj)
            s[ii][jj] = XA * s[ii - 1][jj] + (ii > 1 ? ip * (ii - 1) * s[ii - 2][jj] : 0.0) +
                        (jj > 0 ? ip * jj * s[ii - 1][jj - 1] : 0.0);
}

GTO_HD void spd_st_dim(int i, int j, double a, double b, double XA, double XB, double ip, double (&out)[4]) {
    double s[4][5];
    spd_os_table(XA, XB, ip, s);
    const double b4 = 4.0 * b * b, b2 = 2.0 * b * (2 * j + 1), jj1 = (double)(j * (j - 1)), a2 = 2.0 * a, di = (double)i;
    // per row i' the overlap and the kinetic term at the columns of j
    double so[4], tk[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double c0 = spd_sel3(j, s[r][0], s[r][1], s[r][2]), cp = spd_sel3(j, s[r][2], s[r][3], s[r][4]);
        const double cm = j == 2 ? s[r][0] : 0.0;
        so[r] = c0;
        tk[r] = -0.5 * (b4 * cp - b2 * c0 + jj1 * cm);
    }
    out[0] = spd_sel3(i, so[0], so[1], so[2]);
    out[1] = spd_sel3(i, tk[0], tk[1], tk[2]);
    out[2] = a2 * spd_sel3(i, so[1], so[2], so[3]) - di * spd_sel3(i, 0.0, so[0], so[1]);
    out[3] = a2 * spd_sel3(i, tk[1], tk[2], tk[3]) - di * spd_sel3(i, 0.0, tk[0], tk[1]);
}

// e = the contracted pair mu >= nu of geometry g.
template <bool GRAD>
GTO_HD void spd_one_body(int e, int g, const SpdAos &ao, const double *tab, const double *coords, const double *charges,
                         int N, int natm, int nprim, double *S, double *hcore, double *ipovlp, double *dhcore) {
    constexpr int M = GRAD ? 5 : 4;
    if (e >= N * (N + 1) / 2) return;
    const int mu = gto_tri_row(e), nu = e - mu * (mu + 1) / 2;
    const int km = ao.kind[mu], kn = ao.kind[nu], am = ao.atom[mu], an = ao.atom[nu];
    const int nm = spd_nmono(km), nn = spd_nmono(kn);
    const double *Rg = coords + (int64_t)g * natm * 3;
    const double *tg = tab + (int64_t)g * nprim * nprim * kGtoRow;
    const int64_t n2 = (int64_t)N * N, ij = (int64_t)mu * N + nu, ji = (int64_t)nu * N + mu;
    // overlap and kinetic energy; dsa, dta: derivatives for the centre of mu; dsb, dtb: for the centre of nu
    double s = 0.0, tk = 0.0, dsa[3] = {0.0, 0.0, 0.0}, dta[3] = {0.0, 0.0, 0.0}, dsb[3] = {0.0, 0.0, 0.0},
           dtb[3] = {0.0, 0.0, 0.0};
    for (int pa = ao.off[mu]; pa < ao.off[mu] + ao.np[mu]; ++pa)
        for (int pb = ao.off[nu]; pb < ao.off[nu] + ao.np[nu]; ++pb) {
            const double *r = tg + ((int64_t)pa * nprim + pb) * kGtoRow;
            const double pip = kGtoPi / r[0], w0 = pip * sqrt(pip) * r[4];
            for (int im = 0; im < nm; ++im)
                for (int in = 0; in < nn; ++in) {
                    int pm[3], pn[3];
                    double wm, wn;
                    spd_mono(km, im, pm[0], pm[1], pm[2], wm);
                    spd_mono(kn, in, pn[0], pn[1], pn[2], wn);
                    const double w = w0 * (wm * wn);
                    double d[3][4], sp, tp, ds[3], dt[3];
#pragma unroll
                    for (int x = 0; x < 3; ++x) spd_st_dim(pm[x], pn[x], r[5], r[6], r[8 + x], r[11 + x], r[7], d[x]);
                    gto_overlap_kinetic(d, sp, tp, ds, dt);
                    s = fma(w, sp, s);
                    tk = fma(w, tp, tk);
                    if (GRAD) {
#pragma unroll
                        for (int x = 0; x < 3; ++x) {
                            dsa[x] = fma(w, ds[x], dsa[x]);
                            dta[x] = fma(w, dt[x], dta[x]);
                        }
                        // the same pair with the roles of its functions exchanged (both operators are symmetric)
#pragma unroll
                        for (int x = 0; x < 3; ++x)
                            spd_st_dim(pn[x], pm[x], r[6], r[5], r[11 + x], r[8 + x], r[7], d[x]);
                        gto_overlap_kinetic(d, sp, tp, ds, dt);
#pragma unroll
                        for (int x = 0; x < 3; ++x) {
                            dsb[x] = fma(w, ds[x], dsb[x]);
                            dtb[x] = fma(w, dt[x], dtb[x]);
                        }
                    }
                }
        }
    // nuclear attraction, the nuclei in ascending order; the operator term of nucleus c goes straight to dhcore[c]
    double vn = 0.0, dva[3] = {0.0, 0.0, 0.0}, dvb[3] = {0.0, 0.0, 0.0}, others[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < natm; ++c) {
        const double z = charges[c], C[3] = {Rg[c * 3], Rg[c * 3 + 1], Rg[c * 3 + 2]};
        double op[3] = {0.0, 0.0, 0.0};
        for (int pa = ao.off[mu]; pa < ao.off[mu] + ao.np[mu]; ++pa)
            for (int pb = ao.off[nu]; pb < ao.off[nu] + ao.np[nu]; ++pb) {
                const double *r = tg + ((int64_t)pa * nprim + pb) * kGtoRow;
                const double p = r[0], X[3] = {r[1] - C[0], r[2] - C[1], r[3] - C[2]};
                double H[M + 1];
                gto_boys<M>(p * (X[0] * X[0] + X[1] * X[1] + X[2] * X[2]), H);
                double w = -z * (2.0 * kGtoPi / p) * r[4];
#pragma unroll
                for (int m = 0; m <= M; ++m) {
                    H[m] = H[m] * w;
                    w = w * (-2.0 * p);
                }
                for (int im = 0; im < nm; ++im)
                    for (int in = 0; in < nn; ++in) {
                        int pm[3], pn[3];
                        double wm, wn;
                        spd_mono(km, im, pm[0], pm[1], pm[2], wm);
                        spd_mono(kn, in, pn[0], pn[1], pn[2], wn);
                        const double wt = wm * wn;
                        double A[3][M + 1], Da[3][M + 1], Db[3][M + 1], Op[3][M + 1];
#pragma unroll
                        for (int x = 0; x < 3; ++x) {
                            double base[6], der[6], same[6], c0[M + 1];
                            spd_bra_dim(pm[x], pn[x], r[5], r[8 + x], r[11 + x], r[7], base, der);
                            spd_take<M>(base, c0);
                            spd_poly<M>(c0, X[x], A[x]);
                            if (GRAD) {
                                spd_take<M>(der, c0);
                                spd_poly<M>(c0, X[x], Da[x]);
                                // d/dC of R_n(P - C) = -R_{n+1}
                                c0[0] = 0.0;
#pragma unroll
                                for (int n = 1; n <= M; ++n) c0[n] = -base[n - 1];
                                spd_poly<M>(c0, X[x], Op[x]);
                                spd_bra_dim(pn[x], pm[x], r[6], r[11 + x], r[8 + x], r[7], same, der);
                                spd_take<M>(der, c0);
                                spd_poly<M>(c0, X[x], Db[x]);
                            }
                        }
                        double yz[M + 1];
                        gto_conv<M>(A[1], A[2], yz);
                        vn = vn + wt * gto_dot<M>(H, A[0], yz);
                        if (GRAD) {
                            double xz[M + 1], xy[M + 1];
                            gto_conv<M>(A[0], A[2], xz);
                            gto_conv<M>(A[0], A[1], xy);
                            dva[0] = dva[0] + wt * gto_dot<M>(H, Da[0], yz);
                            dva[1] = dva[1] + wt * gto_dot<M>(H, Da[1], xz);
                            dva[2] = dva[2] + wt * gto_dot<M>(H, Da[2], xy);
                            dvb[0] = dvb[0] + wt * gto_dot<M>(H, Db[0], yz);
                            dvb[1] = dvb[1] + wt * gto_dot<M>(H, Db[1], xz);
                            dvb[2] = dvb[2] + wt * gto_dot<M>(H, Db[2], xy);
                            op[0] = op[0] + wt * gto_dot<M>(H, Op[0], yz);
                            op[1] = op[1] + wt * gto_dot<M>(H, Op[1], xz);
                            op[2] = op[2] + wt * gto_dot<M>(H, Op[2], xy);
                        }
                    }
            }
        if (GRAD) {
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                double *d = dhcore + (((int64_t)g * natm + c) * 3 + x) * n2;
                d[ij] = op[x];
                d[ji] = op[x];
                if (c != am) others[x] = others[x] + op[x];
            }
        }
    }
    const double h = tk + vn;
    S[g * n2 + ij] = s;
    S[g * n2 + ji] = s;
    hcore[g * n2 + ij] = h;
    hcore[g * n2 + ji] = h;
    if (!GRAD) return;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        ipovlp[((int64_t)g * 3 + x) * n2 + ij] = -dsa[x];
        if (mu != nu) ipovlp[((int64_t)g * 3 + x) * n2 + ji] = -dsb[x];
        // the functions of an atom move with it: the row term of mu on the atom of mu, the column term of nu on the atom
        // of nu (this thread wrote the operator terms above and is the only one to touch these two elements)
        const double dha = dta[x] + dva[x], dhb = dtb[x] + dvb[x];
        double *da = dhcore + (((int64_t)g * natm + am) * 3 + x) * n2;
        double *db = dhcore + (((int64_t)g * natm + an) * 3 + x) * n2;
        if (am == an) {
            // both functions on one atom: row, column and the atom's own operator term cancel but for the other nuclei
            // (translational invariance); summing the large cancelling terms instead costs digits with tight functions
            da[ij] = -others[x];
            da[ji] = -others[x];
        } else {
            const double va = da[ij] + dha;
            da[ij] = va;
            da[ji] = va;
            const double vb = db[ij] + dhb;
            db[ij] = vb;
            db[ji] = vb;
        }
    }
}

template <bool GRAD>
__global__ __launch_bounds__(64) void spdgto_one_kernel(SpdAos ao, const double *__restrict__ tab,
                                                         const double *__restrict__ coords,
                                                         const double *__restrict__ charges, int N, int natm, int nprim,
                                                         double *S, double *hcore, double *ipovlp, double *dhcore) {
    spd_one_body<GRAD>(blockIdx.x * 64 + threadIdx.x, blockIdx.y, ao, tab, coords, charges, N, natm, nprim, S, hcore, ipovlp,
                       dhcore);
}

// ---- nuclear repulsion -------------------------------------------------------------------------
// blockIdx.x = geometry; thread i < natm sums over the other centres in ascending order.
template <bool GRAD>
__global__ __launch_bounds__(64) void spdgto_nuc_kernel(const double *__restrict__ coords, const double *__restrict__ charges,
                                                         int natm, double *__restrict__ enuc, double *__restrict__ gnuc) {
    const int g = blockIdx.x, i = threadIdx.x;
    const bool on = i < natm;
    const double *Rg = coords + (int64_t)g * natm * 3;
    const int ii = on ? i : 0;
    const double zi = charges[ii], ax = Rg[ii * 3], ay = Rg[ii * 3 + 1], az = Rg[ii * 3 + 2];
    double en = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    for (int j = 0; j < natm; ++j) {
        if (j == ii) continue;
        const double dx = ax - Rg[j * 3], dy = ay - Rg[j * 3 + 1], dz = az - Rg[j * 3 + 2];
        const double r = sqrt(dx * dx + dy * dy + dz * dz), zz = zi * charges[j];
        if (j > ii) en = en + zz / r;
        if (GRAD) {
            const double r3 = r * r * r;
            gx = gx - zz * dx / r3;
            gy = gy - zz * dy / r3;
            gz = gz - zz * dz / r3;
        }
    }
    if (GRAD && on) {
        double *o = gnuc + ((int64_t)g * natm + i) * 3;
        o[0] = gx;
        o[1] = gy;
        o[2] = gz;
    }
    const double total = wave_sum(on ? en : 0.0);
    if (i == 0) enuc[g] = total;
}

// ---- dipole integrals --------------------------------------------------------------------------
// e = the contracted pair mu >= nu of geometry g; x (r - O) = (x - A) + (A - O): one more power on the first function.
GTO_HD void spd_dipole_body(int e, int g, const SpdPrims &bs, const SpdAos &ao, const double *coords, int N, int natm,
                            double ox, double oy, double oz, double *dip) {
    if (e >= N * (N + 1) / 2) return;
    const int mu = gto_tri_row(e), nu = e - mu * (mu + 1) / 2;
    const int km = ao.kind[mu], kn = ao.kind[nu];
    const int nm = spd_nmono(km), nn = spd_nmono(kn);
    const double *Ra = coords + ((int64_t)g * natm + ao.atom[mu]) * 3, *Rb = coords + ((int64_t)g * natm + ao.atom[nu]) * 3;
    const double O[3] = {ox, oy, oz};
    double acc[3] = {0.0, 0.0, 0.0};
    for (int pa = ao.off[mu]; pa < ao.off[mu] + ao.np[mu]; ++pa)
        for (int pb = ao.off[nu]; pb < ao.off[nu] + ao.np[nu]; ++pb) {
            const double a = bs.ex[pa], b = bs.ex[pb], p = a + b, mup = a * b / p, ip = 0.5 / p;
            double r2 = 0.0, tb[3][4][5];
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const double d = Ra[x] - Rb[x];
                r2 = r2 + d * d;
                spd_os_table(-(b / p) * d, (a / p) * d, ip, tb[x]);
            }
            const double pip = kGtoPi / p, w0 = pip * sqrt(pip) * exp(-mup * r2) * bs.cn[pa] * bs.cn[pb];
            for (int im = 0; im < nm; ++im)
                for (int in = 0; in < nn; ++in) {
                    int pm[3], pn[3];
                    double wm, wn, s0[3], s1[3];
                    spd_mono(km, im, pm[0], pm[1], pm[2], wm);
                    spd_mono(kn, in, pn[0], pn[1], pn[2], wn);
#pragma unroll
                    for (int x = 0; x < 3; ++x) {
                        // s(i', j) for i' <= 3 at the column j
                        double col[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) col[r] = spd_sel3(pn[x], tb[x][r][0], tb[x][r][1], tb[x][r][2]);
                        s0[x] = spd_sel3(pm[x], col[0], col[1], col[2]);
                        s1[x] = spd_sel3(pm[x], col[1], col[2], col[3]) + (Ra[x] - O[x]) * s0[x];
                    }
                    const double w = w0 * (wm * wn);
                    acc[0] = fma(w, s1[0] * s0[1] * s0[2], acc[0]);
                    acc[1] = fma(w, s0[0] * s1[1] * s0[2], acc[1]);
                    acc[2] = fma(w, s0[0] * s0[1] * s1[2], acc[2]);
                }
        }
    const int64_t n2 = (int64_t)N * N;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        dip[((int64_t)g * 3 + x) * n2 + (int64_t)mu * N + nu] = acc[x];
        dip[((int64_t)g * 3 + x) * n2 + (int64_t)nu * N + mu] = acc[x];
    }
}

__global__ __launch_bounds__(64) void spdgto_dipole_kernel(SpdPrims bs, SpdAos ao, const double *__restrict__ coords, int N,
                                                            int natm, double ox, double oy, double oz,
                                                            double *__restrict__ dip) {
    spd_dipole_body(blockIdx.x * 64 + threadIdx.x, blockIdx.y, bs, ao, coords, N, natm, ox, oy, oz, dip);
}

// ---- host side: the route for gto_shells.hpp -----------------------------------------------------
struct SpdRoute {
    using Prims = SpdPrims;
    using Aos = SpdAos;
    static constexpr int kMaxL = 2;
    static constexpr const char *kLs = "0, 1 and 2", *kName = "spdgto";
    static void tag(SpdAos &ao, int f, int l, int c) { ao.kind[f] = (uint8_t)(l == 0 ? 0 : (l == 1 ? 1 + c : 4 + c)); }
    static constexpr auto kPair = spdgto_pair_kernel;
    static constexpr auto kOne = spdgto_one_kernel<true>, kOneE = spdgto_one_kernel<false>;
    static constexpr auto kNuc = spdgto_nuc_kernel<true>, kNucE = spdgto_nuc_kernel<false>;
    static constexpr auto kTwo = spdgto_two_kernel<true>, kTwoE = spdgto_two_kernel<false>;
    static constexpr auto kDipole = spdgto_dipole_kernel;
};

}  // namespace evc

using namespace evc;

extern "C" size_t evc_spdgto_workspace_bytes(int natm, int nshell, int nprim_total, int nao, int count) {
    return gto_workspace_bytes<SpdRoute>("evc_spdgto_workspace_bytes", natm, nshell, nprim_total, nao, count);
}

extern "C" int evc_spdgto_integrals_batch(int natm, int nshell, int count, const double *coords, const double *charges,
                                          const int *shell_atom, const int *shell_l, const int *shell_prim_offset,
                                          const double *exponents, const double *coefficients, const evc_sgto_outputs *out,
                                          int flags, void *ws, size_t ws_bytes, void *stream) {
    return gto_integrals_batch<SpdRoute>("evc_spdgto_integrals_batch", natm, nshell, count, coords, charges, shell_atom,
                                         shell_l, shell_prim_offset, exponents, coefficients, out, flags, ws, ws_bytes,
                                         stream);
}

extern "C" int evc_spdgto_dipole_batch(int natm, int nshell, int count, const double *coords, const int *shell_atom,
                                       const int *shell_l, const int *shell_prim_offset, const double *exponents,
                                       const double *coefficients, const double origin[3], double *dip, void *stream) {
    return gto_dipole_batch<SpdRoute>("evc_spdgto_dipole_batch", natm, nshell, count, coords, shell_atom, shell_l,
                                      shell_prim_offset, exponents, coefficients, origin, dip, stream);
}
