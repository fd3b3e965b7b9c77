// AO integrals and their first nuclear derivatives of a molecule built from contracted Cartesian s and p Gaussian shells
// (evc_spgto_integrals_batch, evc_spgto_dipole_batch): the device statement of evcont_amd/gto_small.py sp_gaussian_mol,
// written straight into the arrays of an evc_geometry_batch.  sgto.hip stays the route for one s function per centre.
//
// Scheme: McMurchie-Davidson, with the Hermite Coulomb integrals kept factored.  Per dimension the product of two
// primitives x_A^i x_B^j is sum_t E_t^{ij} Lambda_t (gto_raise: E^{i+1,j}_t = E_{t-1} / 2p + X_PA E_t + (t + 1) E_{t+1}; the
// exponential factor is kept apart, in the pair table).  The bra and ket expansions of one dimension fold into one
// coefficient array c[n] = sum_{t + tau = n} E_t (-1)^tau E'_tau, and, since the recursion of R_tuv acts on each dimension
// alone (R^m_{n+1} = n R^{m+1}_{n-1} + X R^{m+1}_n), the derivative d^n/dX^n is sum_j a_{n,j}(X) (raise the order m by j)
// with a_{n,j} = n! / ((n - j)! (2j - n)! 2^{n - j}) X^{2j - n}.  So each dimension gives a short array
// A[j] = sum_n c[n] a_{n,j}(X) (sp_poly) and an integral is
//     sum_m H[m] sum_{j + k + l = m} Ax[j] Ay[k] Az[l],    H[m] = w (-2 alpha)^m F_m(alpha |PQ|^2),  m <= 5,
// all loops with fixed bounds, everything in registers.  A derivative with respect to the centre of the first function
// is 2a (i + 1) - i (i - 1) in the power of that dimension: it replaces the E array of ONE dimension, so the three
// components of int2e_ip1 reuse the other two dimensions' arrays of int2e.
// Boys functions (gto_boys): below t = 12 the convergent series of the highest order, then downward recursion
// F_{n-1} = (2t F_n + e^-t) / (2n - 1); above it F0 from erf and upward recursion.
//
// Kernels, each a launch of its own (FP64 VALU; DESIGN.md: FP64 MFMA blocks its SIMD's vector issue):
//   spgto_pair_kernel    the primitive-pair table: per geometry one row of kGtoRow doubles per ORDERED pair of primitive
//                        shells entries (pa, pb): p, P, Kab cn_a cn_b, a, b, 1/2p, P - A, P - B.
//   spgto_one_kernel     one thread per contracted pair mu >= nu: S, hcore (mirrored: exactly symmetric), ipovlp, dhcore
//                        (operator term of every nucleus, plus the rows and columns of the functions that move).
//   spgto_nuc_kernel     nuclear repulsion and its gradient, one thread per centre (the cut of sgto_nuc_kernel).
//   spgto_two_kernel     one thread per (mu nu | kappa >= lambda): blockIdx.y names the bra pair, the threads run over the
//                        packed ket index, blockIdx.z is the geometry.  Every thread walks its primitive quartets in one
//                        fixed order (ket pair outer, bra pair inner) and keeps int2e and the three components of
//                        int2e_ip1 in registers.  int2e is stored by the blocks mu >= nu alone, to every image they own.
//                        No screening: every quartet is evaluated.
//   spgto_dipole_kernel  <mu| r - origin |nu>, one thread per contracted pair mu >= nu, mirrored.
// No sum is split across threads and there are no read-modify-write operations between threads: the same bits from run to
// run and for every batch size, and the full forms are the unpacked packed forms.  The two instantiations of
// spgto_two_kernel (with and without the gradient) use Boys orders 5 and 4 and need not round int2e alike.
// The basis is a HOST argument and reaches the kernels by value.
// What lives where: gto_shells.hpp holds what this file shares with spdgto.hip -- the limits, GtoPrims, gto_tri_row, gto_boys,
// gto_raise, gto_conv, gto_dot, gto_overlap_kinetic, the pair-table body and the whole host side (every refusal, the basis as
// the kernels take it, the three calls), which is told about this route by SpRoute at the end of the file.  Here: the maths
// of the powers 0 and 1 (sp_bra_dim, sp_ket_dim, sp_fold, sp_poly, sp_st_dim, the one / two / dipole bodies) and the kernels.
#include "gto_shells.hpp"

namespace evc {

struct SpPrims : GtoPrims {};
struct SpAos {
    uint8_t off[kGtoMaxAo];      // first primitive of the function's shell
    uint8_t np[kGtoMaxAo];       // primitives of the shell
    int8_t dir[kGtoMaxAo];       // -1: s; 0, 1, 2: p_x, p_y, p_z
    uint8_t atom[kGtoMaxAo];
};

// Hermite coefficients (t <= 3) of one dimension of a primitive pair with the powers i, j (0 or 1), without the
// exponential: `base` = E^{ij}, `der` = those of d/dA, 2a E^{i+1,j} - i E^{i-1,j}.  XA = P - A, XB = P - B, ip = 1 / 2p.
GTO_HD void sp_bra_dim(bool i, bool j, double a, double XA, double XB, double ip, double (&base)[4], double (&der)[4]) {
    const double e0[4] = {1.0, 0.0, 0.0, 0.0};
    double r[4], ej[4], e1[4], e2[4];
    gto_raise(e0, XB, ip, r);
#pragma unroll
    for (int t = 0; t < 4; ++t) ej[t] = j ? r[t] : e0[t];
    gto_raise(ej, XA, ip, e1);
    gto_raise(e1, XA, ip, e2);
    const double a2 = 2.0 * a;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        base[t] = i ? e1[t] : ej[t];
        der[t] = i ? a2 * e2[t] - ej[t] : a2 * e1[t];
    }
}

// (-1)^tau E^{kl}_tau (tau <= 2) of one dimension of the ket pair.
GTO_HD void sp_ket_dim(bool k, bool l, double XC, double XD, double ip, double (&o)[3]) {
    const double e0[3] = {1.0, 0.0, 0.0};
    double r[3], el[3], e1[3];
    gto_raise(e0, XD, ip, r);
#pragma unroll
    for (int t = 0; t < 3; ++t) el[t] = l ? r[t] : e0[t];
    gto_raise(el, XC, ip, e1);
    o[0] = k ? e1[0] : el[0];
    o[1] = -(k ? e1[1] : el[1]);
    o[2] = k ? e1[2] : el[2];
}

// c[n] = sum_{t + tau = n} b[t] k[tau], n <= M.
template <int M>
GTO_HD void sp_fold(const double (&b)[4], const double (&k)[3], double (&c)[M + 1]) {
#pragma unroll
    for (int n = 0; n <= M; ++n) {
        double s = 0.0;
#pragma unroll
        for (int tau = 0; tau < 3; ++tau)
            if (n - tau >= 0 && n - tau < 4) s = fma(b[n - tau], k[tau], s);
        c[n] = s;
    }
}

template <int M, int N>
GTO_HD double sp_at(const double (&c)[M + 1]) {
    if constexpr (N <= M) return c[N];
    return 0.0;
}

// A[j] = sum_n c[n] a_{n,j}(X): the derivatives d^n/dX^n of a function of alpha |R|^2 as raises of its order.
template <int M>
GTO_HD void sp_poly(const double (&c)[M + 1], double X, double (&A)[M + 1]) {
    const double X2 = X * X, X3 = X2 * X;
    const double c1 = sp_at<M, 1>(c), c2 = sp_at<M, 2>(c), c3 = sp_at<M, 3>(c), c4 = sp_at<M, 4>(c), c5 = sp_at<M, 5>(c);
    const double v[6] = {c[0], c1 * X + c2, c2 * X2 + 3.0 * (c3 * X + c4), c3 * X3 + 6.0 * c4 * X2 + 15.0 * c5 * X,
                         c4 * X2 * X2 + 10.0 * c5 * X3, c5 * X3 * X2};
#pragma unroll
    for (int j = 0; j <= M; ++j) A[j] = v[j];
}

// ---- pair table ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spgto_pair_kernel(SpPrims bs, const double *__restrict__ coords, int natm, int nprim,
                                                          double *__restrict__ tab) {
    gto_pair_body(blockIdx.x * 256 + threadIdx.x, blockIdx.y, bs, coords, natm, nprim, tab);
}

// ---- two-electron integrals ----------------------------------------------------------------
// M: the highest Hermite order, 5 with the gradient and 4 without.
template <bool GRAD>
GTO_HD void sp_two_body(int mu, int nu, int v, int g, const SpAos &ao, const double *tab, int N, int nprim, int s4, int s2kl,
                        double *eri, double *ip1) {
    constexpr int M = GRAD ? 5 : 4;
    const int Ms = N * (N + 1) / 2;
    if (v >= Ms) return;
    const int kap = gto_tri_row(v), lam = v - kap * (kap + 1) / 2;
    const double *tg = tab + (int64_t)g * nprim * nprim * kGtoRow;
    const int dm = ao.dir[mu], dn = ao.dir[nu], dk = ao.dir[kap], dl = ao.dir[lam];
    double acc = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    for (int pc = ao.off[kap]; pc < ao.off[kap] + ao.np[kap]; ++pc)
        for (int pd = ao.off[lam]; pd < ao.off[lam] + ao.np[lam]; ++pd) {
            const double *kr = tg + ((int64_t)pc * nprim + pd) * kGtoRow;
            const double q = kr[0], qx = kr[1], qy = kr[2], qz = kr[3], ck = kr[4];
            double ek[3][3];
#pragma unroll
            for (int x = 0; x < 3; ++x) sp_ket_dim(dk == x, dl == x, kr[8 + x], kr[11 + x], kr[7], ek[x]);
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
                    double A[3][M + 1], D[3][M + 1];
#pragma unroll
                    for (int x = 0; x < 3; ++x) {
                        double base[4], der[4], c[M + 1];
                        sp_bra_dim(dm == x, dn == x, br[5], br[8 + x], br[11 + x], br[7], base, der);
                        sp_fold<M>(base, ek[x], c);
                        sp_poly<M>(c, X[x], A[x]);
                        if (GRAD) {
                            sp_fold<M>(der, ek[x], c);
                            sp_poly<M>(c, X[x], D[x]);
                        }
                    }
                    double yz[M + 1];
                    gto_conv<M>(A[1], A[2], yz);
                    acc = acc + gto_dot<M>(H, A[0], yz);
                    if (GRAD) {
                        double xz[M + 1], xy[M + 1];
                        gto_conv<M>(A[0], A[2], xz);
                        gto_conv<M>(A[0], A[1], xy);
                        // electron gradient = - centre gradient
                        gx = gx - gto_dot<M>(H, D[0], yz);
                        gy = gy - gto_dot<M>(H, D[1], xz);
                        gz = gz - gto_dot<M>(H, D[2], xy);
                    }
                }
        }
    const int64_t n2 = (int64_t)N * N, kl = (int64_t)kap * N + lam, lk = (int64_t)lam * N + kap;
    if (GRAD) {
        const double gv[3] = {gx, gy, gz};
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const int64_t row = ((int64_t)g * 3 + x) * n2 + (int64_t)mu * N + nu;
            if (s2kl) {
                ip1[row * Ms + v] = gv[x];
            } else {
                ip1[row * n2 + kl] = gv[x];
                ip1[row * n2 + lk] = gv[x];
            }
        }
    }
    if (mu < nu) return;
    if (s4) {
        eri[((int64_t)g * Ms + mu * (mu + 1) / 2 + nu) * Ms + v] = acc;
    } else {
        double *eg = eri + (int64_t)g * n2 * n2;
        const int64_t mn = ((int64_t)mu * N + nu) * n2, nm = ((int64_t)nu * N + mu) * n2;
        eg[mn + kl] = acc;
        eg[mn + lk] = acc;
        eg[nm + kl] = acc;
        eg[nm + lk] = acc;
    }
}

// GRAD: gridDim.y = N^2, blockIdx.y = mu N + nu; otherwise gridDim.y = Ms, blockIdx.y = mu (mu + 1) / 2 + nu.
// s4 / s2kl: the forms of eri / eri_ip1 (EVC_FLAG_ERI_S4 / EVC_FLAG_IP1_S2KL).
template <bool GRAD>
__global__ __launch_bounds__(64) void spgto_two_kernel(SpAos ao, const double *__restrict__ tab, int N, int nprim, int s4,
                                                        int s2kl, double *__restrict__ eri, double *__restrict__ ip1) {
    const int by = blockIdx.y;
    int mu, nu;
    if (GRAD) {
        mu = by / N;
        nu = by - mu * N;
    } else {
        mu = tri_row_small(by);
        nu = by - mu * (mu + 1) / 2;
    }
    sp_two_body<GRAD>(mu, nu, blockIdx.x * 64 + threadIdx.x, blockIdx.z, ao, tab, N, nprim, s4, s2kl, eri, ip1);
}

// ---- one-electron integrals ------------------------------------------------------------------
// One dimension of overlap and kinetic energy of a primitive pair with the powers i, j (0 or 1), without the factor
// sqrt(pi / p) and the exponential: s(i', j') by the Obara-Saika recursion for i' <= 2, j' <= 3, then
//   out[0], out[1]   the overlap and -1/2 d^2/dx^2 on the second function, 4 b^2 s(i, j+2) - 2 b (2j + 1) s(i, j)
//   out[2], out[3]   their derivatives for the centre of the first function, 2a (i + 1) - i (i - 1)
GTO_HD void sp_st_dim(bool i, bool j, double a, double b, double XA, double XB, double ip, double (&out)[4]) {
    double s[3][4];
    s[0][0] = 1.0;
#pragma unroll
    for (int jj = 1; jj < 4; ++jj) s[0][jj] = XB * s[0][jj - 1] + (jj > 1 ? ip * (jj - 1) * s[0][jj - 2] : 0.0);
#pragma unroll
    for (int ii = 1; ii < 3; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            s[ii][jj] = XA * s[ii - 1][jj] + (ii > 1 ? ip * (ii - 1) * s[ii - 2][jj] : 0.0) +
                        (jj > 0 ? ip * jj * s[ii - 1][jj - 1] : 0.0);
    // the rows i - 1, i, i + 1 at the columns j and j + 2
    double lo[2], mid[2], up[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int j0 = 2 * c;
        lo[c] = i ? (j ? s[0][j0 + 1] : s[0][j0]) : 0.0;
        mid[c] = i ? (j ? s[1][j0 + 1] : s[1][j0]) : (j ? s[0][j0 + 1] : s[0][j0]);
        up[c] = i ? (j ? s[2][j0 + 1] : s[2][j0]) : (j ? s[1][j0 + 1] : s[1][j0]);
    }
    const double b4 = 4.0 * b * b, b2 = 2.0 * b * (j ? 3.0 : 1.0), a2 = 2.0 * a;
    const double tlo = -0.5 * (b4 * lo[1] - b2 * lo[0]), tmid = -0.5 * (b4 * mid[1] - b2 * mid[0]);
    const double tup = -0.5 * (b4 * up[1] - b2 * up[0]);
    out[0] = mid[0];
    out[1] = tmid;
    out[2] = a2 * up[0] - lo[0];
    out[3] = a2 * tup - tlo;
}

// e = the contracted pair mu >= nu of geometry g.
template <bool GRAD>
GTO_HD void sp_one_body(int e, int g, const SpAos &ao, const double *tab, const double *coords, const double *charges, int N,
                        int natm, int nprim, double *S, double *hcore, double *ipovlp, double *dhcore) {
    constexpr int M = 3;
    if (e >= N * (N + 1) / 2) return;
    const int mu = gto_tri_row(e), nu = e - mu * (mu + 1) / 2;
    const int dm = ao.dir[mu], dn = ao.dir[nu], am = ao.atom[mu], an = ao.atom[nu];
    const double *Rg = coords + (int64_t)g * natm * 3;
    const double *tg = tab + (int64_t)g * nprim * nprim * kGtoRow;
    const int64_t n2 = (int64_t)N * N, ij = (int64_t)mu * N + nu, ji = (int64_t)nu * N + mu;
    // overlap and kinetic energy; dsa, dta: derivatives for the centre of mu; dsb, dtb: for the centre of nu
    double s = 0.0, tk = 0.0, dsa[3] = {0.0, 0.0, 0.0}, dta[3] = {0.0, 0.0, 0.0}, dsb[3] = {0.0, 0.0, 0.0},
           dtb[3] = {0.0, 0.0, 0.0};
    for (int pa = ao.off[mu]; pa < ao.off[mu] + ao.np[mu]; ++pa)
        for (int pb = ao.off[nu]; pb < ao.off[nu] + ao.np[nu]; ++pb) {
            const double *r = tg + ((int64_t)pa * nprim + pb) * kGtoRow;
            const double pip = kGtoPi / r[0], w = pip * sqrt(pip) * r[4];
            double d[3][4], sp, tp, ds[3], dt[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) sp_st_dim(dm == x, dn == x, r[5], r[6], r[8 + x], r[11 + x], r[7], d[x]);
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
                for (int x = 0; x < 3; ++x) sp_st_dim(dn == x, dm == x, r[6], r[5], r[11 + x], r[8 + x], r[7], d[x]);
                gto_overlap_kinetic(d, sp, tp, ds, dt);
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    dsb[x] = fma(w, ds[x], dsb[x]);
                    dtb[x] = fma(w, dt[x], dtb[x]);
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
                double A[3][M + 1], Da[3][M + 1], Db[3][M + 1], Op[3][M + 1];
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    double base[4], der[4], same[4];
                    sp_bra_dim(dm == x, dn == x, r[5], r[8 + x], r[11 + x], r[7], base, der);
                    sp_poly<M>(base, X[x], A[x]);
                    if (GRAD) {
                        sp_poly<M>(der, X[x], Da[x]);
                        // d/dC of R_n(P - C) = -R_{n+1}
                        const double shifted[4] = {0.0, -base[0], -base[1], -base[2]};
                        sp_poly<M>(shifted, X[x], Op[x]);
                        sp_bra_dim(dn == x, dm == x, r[6], r[11 + x], r[8 + x], r[7], same, der);
                        sp_poly<M>(der, X[x], Db[x]);
                    }
                }
                double yz[M + 1];
                gto_conv<M>(A[1], A[2], yz);
                vn = vn + gto_dot<M>(H, A[0], yz);
                if (GRAD) {
                    double xz[M + 1], xy[M + 1];
                    gto_conv<M>(A[0], A[2], xz);
                    gto_conv<M>(A[0], A[1], xy);
                    dva[0] = dva[0] + gto_dot<M>(H, Da[0], yz);
                    dva[1] = dva[1] + gto_dot<M>(H, Da[1], xz);
                    dva[2] = dva[2] + gto_dot<M>(H, Da[2], xy);
                    dvb[0] = dvb[0] + gto_dot<M>(H, Db[0], yz);
                    dvb[1] = dvb[1] + gto_dot<M>(H, Db[1], xz);
                    dvb[2] = dvb[2] + gto_dot<M>(H, Db[2], xy);
                    op[0] = op[0] + gto_dot<M>(H, Op[0], yz);
                    op[1] = op[1] + gto_dot<M>(H, Op[1], xz);
                    op[2] = op[2] + gto_dot<M>(H, Op[2], xy);
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
__global__ __launch_bounds__(64) void spgto_one_kernel(SpAos ao, const double *__restrict__ tab,
                                                        const double *__restrict__ coords,
                                                        const double *__restrict__ charges, int N, int natm, int nprim,
                                                        double *S, double *hcore, double *ipovlp, double *dhcore) {
    sp_one_body<GRAD>(blockIdx.x * 64 + threadIdx.x, blockIdx.y, ao, tab, coords, charges, N, natm, nprim, S, hcore, ipovlp,
                      dhcore);
}

// ---- nuclear repulsion -------------------------------------------------------------------------
// blockIdx.x = geometry; thread i < natm sums over the other centres in ascending order.
template <bool GRAD>
__global__ __launch_bounds__(64) void spgto_nuc_kernel(const double *__restrict__ coords, const double *__restrict__ charges,
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
GTO_HD void sp_dipole_body(int e, int g, const SpPrims &bs, const SpAos &ao, const double *coords, int N, int natm,
                           double ox, double oy, double oz, double *dip) {
    if (e >= N * (N + 1) / 2) return;
    const int mu = gto_tri_row(e), nu = e - mu * (mu + 1) / 2;
    const int dm = ao.dir[mu], dn = ao.dir[nu];
    const double *Ra = coords + ((int64_t)g * natm + ao.atom[mu]) * 3, *Rb = coords + ((int64_t)g * natm + ao.atom[nu]) * 3;
    const double O[3] = {ox, oy, oz};
    double acc[3] = {0.0, 0.0, 0.0};
    for (int pa = ao.off[mu]; pa < ao.off[mu] + ao.np[mu]; ++pa)
        for (int pb = ao.off[nu]; pb < ao.off[nu] + ao.np[nu]; ++pb) {
            const double a = bs.ex[pa], b = bs.ex[pb], p = a + b, mup = a * b / p, ip = 0.5 / p;
            double r2 = 0.0, s0[3], s1[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const double d = Ra[x] - Rb[x], XA = -(b / p) * d, XB = (a / p) * d;
                const bool i = dm == x, j = dn == x;
                r2 = r2 + d * d;
                // s(i', j) for i' <= 2 at the column j
                const double c0 = j ? XB : 1.0;
                const double c1 = XA * c0 + (j ? ip : 0.0);
                const double c2 = XA * c1 + ip * c0 + (j ? ip * XA : 0.0);
                s0[x] = i ? c1 : c0;
                s1[x] = (i ? c2 : c1) + (Ra[x] - O[x]) * s0[x];
            }
            const double pip = kGtoPi / p, w = pip * sqrt(pip) * exp(-mup * r2) * bs.cn[pa] * bs.cn[pb];
            acc[0] = fma(w, s1[0] * s0[1] * s0[2], acc[0]);
            acc[1] = fma(w, s0[0] * s1[1] * s0[2], acc[1]);
            acc[2] = fma(w, s0[0] * s0[1] * s1[2], acc[2]);
        }
    const int64_t n2 = (int64_t)N * N;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        dip[((int64_t)g * 3 + x) * n2 + (int64_t)mu * N + nu] = acc[x];
        dip[((int64_t)g * 3 + x) * n2 + (int64_t)nu * N + mu] = acc[x];
    }
}

__global__ __launch_bounds__(64) void spgto_dipole_kernel(SpPrims bs, SpAos ao, const double *__restrict__ coords, int N,
                                                           int natm, double ox, double oy, double oz,
                                                           double *__restrict__ dip) {
    sp_dipole_body(blockIdx.x * 64 + threadIdx.x, blockIdx.y, bs, ao, coords, N, natm, ox, oy, oz, dip);
}

// ---- host side: the route for gto_shells.hpp -----------------------------------------------------
struct SpRoute {
    using Prims = SpPrims;
    using Aos = SpAos;
    static constexpr int kMaxL = 1;
    static constexpr const char *kLs = "0 and 1", *kName = "spgto";
    static void tag(SpAos &ao, int f, int l, int c) { ao.dir[f] = (int8_t)(l == 1 ? c : -1); }
    static constexpr auto kPair = spgto_pair_kernel;
    static constexpr auto kOne = spgto_one_kernel<true>, kOneE = spgto_one_kernel<false>;
    static constexpr auto kNuc = spgto_nuc_kernel<true>, kNucE = spgto_nuc_kernel<false>;
    static constexpr auto kTwo = spgto_two_kernel<true>, kTwoE = spgto_two_kernel<false>;
    static constexpr auto kDipole = spgto_dipole_kernel;
};

}  // namespace evc

using namespace evc;

extern "C" size_t evc_spgto_workspace_bytes(int natm, int nshell, int nprim_total, int nao, int count) {
    return gto_workspace_bytes<SpRoute>("evc_spgto_workspace_bytes", natm, nshell, nprim_total, nao, count);
}

extern "C" int evc_spgto_integrals_batch(int natm, int nshell, int count, const double *coords, const double *charges,
                                         const int *shell_atom, const int *shell_l, const int *shell_prim_offset,
                                         const double *exponents, const double *coefficients, const evc_sgto_outputs *out,
                                         int flags, void *ws, size_t ws_bytes, void *stream) {
    return gto_integrals_batch<SpRoute>("evc_spgto_integrals_batch", natm, nshell, count, coords, charges, shell_atom,
                                        shell_l, shell_prim_offset, exponents, coefficients, out, flags, ws, ws_bytes,
                                        stream);
}

extern "C" int evc_spgto_dipole_batch(int natm, int nshell, int count, const double *coords, const int *shell_atom,
                                      const int *shell_l, const int *shell_prim_offset, const double *exponents,
                                      const double *coefficients, const double origin[3], double *dip, void *stream) {
    return gto_dipole_batch<SpRoute>("evc_spgto_dipole_batch", natm, nshell, count, coords, shell_atom, shell_l,
                                     shell_prim_offset, exponents, coefficients, origin, dip, stream);
}
