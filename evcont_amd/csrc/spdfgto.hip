// AO integrals and their first nuclear derivatives of a molecule built from contracted s, p, REAL SPHERICAL d and REAL
// SPHERICAL f Gaussian shells (evc_spdfgto_integrals_batch, evc_spdfgto_dipole_batch, evc_spdfgto_dipole_grad_batch): the
// device statement of evcont_amd/gto_spdf.py spdf_gaussian_mol, written straight into the arrays of an evc_geometry_batch.
// spdgto.hip stays the route for molecules with l <= 2, spgto.hip for s and p shells alone, sgto.hip for one s function
// per centre.
//
// Scheme: that of spdgto.hip (McMurchie-Davidson with the Hermite Coulomb integrals kept factored per dimension; a
// contracted function is a sum over (primitive x monomial) with constant weights, the thread that owns a contracted element
// loops over the monomials of its functions; the Hermite coefficients of a dimension come from power-raising steps with the
// wanted row picked by selects, so every loop has fixed bounds and no register array is indexed at run time).  The seven f
// functions (m = -3 ... 3, PySCF's order) have at most three monomials each (spdf_mono); Cartesian combinations with r^2
// never appear.
//
// The cut: the two-electron body is specialised on CLASSES of angular momentum.  spdf_two_body<GRAD, LB, LK> is written for
// a bra pair whose higher l is LB and a ket pair whose higher l is LK: the raising steps run to the powers LB and LK, the
// bra arrays hold t <= 2 LB + 1 (2 LB without the gradient), the ket arrays tau <= 2 LK and their fold n <= M =
// 2 LB + 2 LK + 1, with M + 1 Boys functions: (ss|ss) pays for F0, F1 and no raising step, only (f.|f.) quartets for F0 ...
// F13.  One kernel holds the sixteen classes of a GRAD value behind a switch:
//   the bra pair (mu, nu) is the block's (blockIdx.y), so the bra class is uniform in a block;
//   the kets are taken in the order of the functions SORTED BY l (SpdfAos::perm, made on the host): thread v' owns the
//   pair (a' >= b') of sorted positions, that is the functions perm[a'], perm[b'], whose class is the l of perm[a'].  The
//   packed index v' ascends with a', so the ket classes follow each other and a wave of 64 kets is of one class except
//   where it straddles one of the three boundaries; there its lanes run the classes present one after the other.
//   The map v' -> (kappa >= lambda) is a bijection of the packed pairs: every element has one owner, as before.
//   Cost of the single kernel: a wave that straddles a boundary runs two bodies one after the other (at most three such
//   waves per bra pair), and the kernel has the registers and scratch of its worst class, (ff|ff), so every class runs at
//   one wave per SIMD.
// The one-electron, dipole and dipole-gradient kernels are O(N^2) threads and keep ONE body at the orders of l = 3.
// Orders with f: the bra reaches t <= 7 (3 + 3 and the centre derivative), the ket tau <= 6, their fold n <= 13; Boys
// functions F0 ... F13 (F0 ... F12 under EVC_FLAG_ENERGY_ONLY, F0 ... F7 / F0 ... F6 for the attraction); gto_boys as in
// the other routes: below t = 12 the series of the highest order and downward recursion, above it erf and upward recursion.
//
// Kernels, each a launch of its own (FP64 VALU, no MFMA):
//   spdfgto_pair_kernel         the primitive-pair table (gto_pair_body).
//   spdfgto_one_kernel          one thread per contracted pair mu >= nu: S, hcore (mirrored), ipovlp, dhcore.
//   spdfgto_nuc_kernel          nuclear repulsion and its gradient, one thread per centre.
//   spdfgto_two_kernel          one thread per (mu nu | kappa >= lambda); primitive quartets in one fixed order (ket pair
//                               outer, bra pair inner), inside a quartet the monomials in one fixed order (ket outer, bra
//                               inner).  No screening: every quartet is evaluated.
//   spdfgto_dipole_kernel       <mu| r - origin |nu>, one thread per contracted pair mu >= nu, mirrored.
//   spdfgto_dipole_grad_kernel  <d_x mu| r_c - origin_c |nu>, one thread per ORDERED contracted pair (the scheme of
//                               field_grad_kernel, first index up to l + 2 = 5); launched from this file.
// No sum is split across threads and there are no read-modify-write operations between threads: the same bits from run to
// run and for every batch size, and the full forms are the unpacked packed forms.  The class of an element depends on the
// basis alone, so an element is always computed by the same instructions.
// The basis is a HOST argument and reaches the kernels by value.  gto_shells.hpp holds the shared parts and the whole host
// side, told about this route by SpdfRoute at the end of the file.
#include "gto_shells.hpp"

namespace evc {

struct SpdfPrims : GtoPrims {};
struct SpdfAos {
    uint8_t off[kGtoMaxAo];      // first primitive of the function's shell
    uint8_t np[kGtoMaxAo];       // primitives of the shell
    uint8_t kind[kGtoMaxAo];     // 0: s; 1 ... 3: p; 4 ... 8: d (spd_mono); 9 ... 15: f, m = -3 ... 3
    uint8_t atom[kGtoMaxAo];
    uint8_t perm[kGtoMaxAo];     // the functions in ascending l (stable); padding stays behind them
};

constexpr int kSpdfP = 3;        // the highest power of one dimension

GTO_HD int spdf_l(int kind) { return kind == 0 ? 0 : (kind < 4 ? 1 : (kind < 9 ? 2 : 3)); }

// ---- monomials of a function ---------------------------------------------------------------------
// f functions, for primitives normalised as x y z exp(-a r^2):
//   m = -3  y (3 x^2 - y^2) / sqrt(24)        m = 1  x (4 z^2 - x^2 - y^2) / sqrt(40)
//   m = -2  x y z                             m = 2  z (x^2 - y^2) / 2
//   m = -1  y (4 z^2 - x^2 - y^2) / sqrt(40)  m = 3  x (x^2 - 3 y^2) / sqrt(24)
//   m =  0  z (2 z^2 - 3 x^2 - 3 y^2) / sqrt(60)
GTO_HD int spdf_nmono(int kind) {
    if (kind < 9) return spd_nmono(kind);
    const int m = kind - 9;
    return m == 1 ? 1 : ((m >= 2 && m <= 4) ? 3 : 2);
}

// Powers (i0, i1, i2) of x, y, z and weight of monomial k of a function of `kind`.
GTO_HD void spdf_mono(int kind, int k, int &i0, int &i1, int &i2, double &w) {
    if (kind < 9) {
        spd_mono(kind, k, i0, i1, i2, w);
        return;
    }
    constexpr double r24 = 0.20412414523193151, r40 = 0.15811388300841897, r60 = 0.12909944487358056;
    // power of x | power of y << 2 | power of z << 4
    int code;
    switch ((kind - 9) * 3 + k) {
        case 0: code = 2 | (1 << 2); w = 3.0 * r24; break;
        case 1: code = 3 << 2; w = -r24; break;
        case 3: code = 1 | (1 << 2) | (1 << 4); w = 1.0; break;
        case 6: code = (1 << 2) | (2 << 4); w = 4.0 * r40; break;
        case 7: code = 2 | (1 << 2); w = -r40; break;
        case 8: code = 3 << 2; w = -r40; break;
        case 9: code = 3 << 4; w = 2.0 * r60; break;
        case 10: code = 2 | (1 << 4); w = -3.0 * r60; break;
        case 11: code = (2 << 2) | (1 << 4); w = -3.0 * r60; break;
        case 12: code = 1 | (2 << 4); w = 4.0 * r40; break;
        case 13: code = 3; w = -r40; break;
        case 14: code = 1 | (2 << 2); w = -r40; break;
        case 15: code = 2 | (1 << 4); w = 0.5; break;
        case 16: code = (2 << 2) | (1 << 4); w = -0.5; break;
        case 18: code = 3; w = r24; break;
        case 19: code = 1 | (2 << 2); w = -3.0 * r24; break;
        default: code = 0; w = 0.0; break;
    }
    i0 = code & 3;
    i1 = (code >> 2) & 3;
    i2 = (code >> 4) & 3;
}

// v[i] for 0 <= i <= P, by selects
template <int P>
GTO_HD double spdf_sel(int i, const double (&v)[P + 1]) {
    double r = v[P];
#pragma unroll
    for (int k = P - 1; k >= 0; --k) r = i == k ? v[k] : r;
    return r;
}

// ---- Hermite coefficients of one dimension ---------------------------------------------------
// Hermite coefficients (t < T) of one dimension of a primitive pair with the powers i, j (0 ... P), without the
// exponential: `base` = E^{ij}, `der` = those of d/dA, 2a E^{i+1,j} - i E^{i-1,j} (complete for T >= 2 P + 2).
// XA = P - A, XB = P - B, ip = 1 / 2p.  All raising steps run; the rows are picked by selects.
template <int P, int T>
GTO_HD void spdf_bra_dim(int i, int j, double a, double XA, double XB, double ip, double (&base)[T], double (&der)[T]) {
    double b[P + 1][T], r[P + 2][T];
#pragma unroll
    for (int t = 0; t < T; ++t) b[0][t] = t == 0 ? 1.0 : 0.0;
#pragma unroll
    for (int k = 1; k <= P; ++k) gto_raise(b[k - 1], XB, ip, b[k]);
#pragma unroll
    for (int t = 0; t < T; ++t) {
        double v[P + 1];
#pragma unroll
        for (int k = 0; k <= P; ++k) v[k] = b[k][t];
        r[0][t] = spdf_sel<P>(j, v);
    }
#pragma unroll
    for (int k = 1; k <= P + 1; ++k) gto_raise(r[k - 1], XA, ip, r[k]);
    const double ax2 = 2.0 * a, di = (double)i;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        double mid[P + 1], up[P + 1], dn[P + 1];
#pragma unroll
        for (int k = 0; k <= P; ++k) {
            mid[k] = r[k][t];
            up[k] = r[k + 1][t];
            dn[k] = k > 0 ? r[k - 1][t] : 0.0;
        }
        base[t] = spdf_sel<P>(i, mid);
        der[t] = ax2 * spdf_sel<P>(i, up) - di * spdf_sel<P>(i, dn);
    }
}

// (-1)^tau E^{kl}_tau (tau <= 2 P) of one dimension of the ket pair, powers k, l (0 ... P).
template <int P>
GTO_HD void spdf_ket_dim(int k, int l, double XC, double XD, double ip, double (&o)[2 * P + 1]) {
    constexpr int T = 2 * P + 1;
    double d[P + 1][T], c[P + 1][T];
#pragma unroll
    for (int t = 0; t < T; ++t) d[0][t] = t == 0 ? 1.0 : 0.0;
#pragma unroll
    for (int q = 1; q <= P; ++q) gto_raise(d[q - 1], XD, ip, d[q]);
#pragma unroll
    for (int t = 0; t < T; ++t) {
        double v[P + 1];
#pragma unroll
        for (int q = 0; q <= P; ++q) v[q] = d[q][t];
        c[0][t] = spdf_sel<P>(l, v);
    }
#pragma unroll
    for (int q = 1; q <= P; ++q) gto_raise(c[q - 1], XC, ip, c[q]);
#pragma unroll
    for (int t = 0; t < T; ++t) {
        double v[P + 1];
#pragma unroll
        for (int q = 0; q <= P; ++q) v[q] = c[q][t];
        const double e = spdf_sel<P>(k, v);
        o[t] = (t & 1) ? -e : e;
    }
}

// c[n] = sum_{t + tau = n} b[t] k[tau], n <= M.
template <int TB, int TK, int M>
GTO_HD void spdf_fold(const double (&b)[TB], const double (&k)[TK], double (&c)[M + 1]) {
#pragma unroll
    for (int n = 0; n <= M; ++n) {
        double s = 0.0;
#pragma unroll
        for (int tau = 0; tau < TK; ++tau)
            if (n - tau >= 0 && n - tau < TB) s = fma(b[n - tau], k[tau], s);
        c[n] = s;
    }
}

// the first M + 1 entries of a bra array
template <int TB, int M>
GTO_HD void spdf_take(const double (&b)[TB], double (&c)[M + 1]) {
#pragma unroll
    for (int n = 0; n <= M; ++n) c[n] = n < TB ? b[n] : 0.0;
}

// a_{n,j} = n! / ((n - j)! (2j - n)! 2^{n - j}), j <= n <= 2j
// (a loop, not a recursion: where the compiler does not fold a coefficient it must not leave a recursive call, whose
// stack the launch cannot size, in a kernel)
constexpr double spdf_factorial(int n) {
    double f = 1.0;
    for (int k = 2; k <= n; ++k) f = f * k;
    return f;
}
constexpr double spdf_poly_coef(int n, int j) {
    return spdf_factorial(n) / (spdf_factorial(n - j) * spdf_factorial(2 * j - n) * (double)(1 << (n - j)));
}

// A[j] = sum_n c[n] a_{n,j} X^{2j - n}: the derivatives d^n/dX^n of a function of alpha |R|^2 as raises of its order.
template <int M>
GTO_HD void spdf_poly(const double (&c)[M + 1], double X, double (&A)[M + 1]) {
    double Xp[M + 1];
    Xp[0] = 1.0;
#pragma unroll
    for (int k = 1; k <= M; ++k) Xp[k] = Xp[k - 1] * X;
#pragma unroll
    for (int j = 0; j <= M; ++j) {
        double s = 0.0;
#pragma unroll
        for (int n = j; n <= M; ++n)
            if (n <= 2 * j) s = fma(c[n] * spdf_poly_coef(n, j), Xp[2 * j - n], s);
        A[j] = s;
    }
}

// ---- pair table ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spdfgto_pair_kernel(SpdfPrims bs, const double *__restrict__ coords, int natm,
                                                            int nprim, double *__restrict__ tab) {
    gto_pair_body(blockIdx.x * 256 + threadIdx.x, blockIdx.y, bs, coords, natm, nprim, tab);
}

// ---- two-electron integrals ----------------------------------------------------------------
// The element (mu nu | kap lam), kap >= lam, of a bra pair of class LB and a ket pair of class LK (the higher l of the
// pair); v = kap (kap + 1) / 2 + lam.
template <bool GRAD, int LB, int LK>
GTO_HD void spdf_two_body(int mu, int nu, int kap, int lam, int g, const SpdfAos &ao, const double *tab, int N, int nprim,
                          int s4, int s2kl, double *eri, double *ip1) {
    constexpr int TB = 2 * LB + 1 + (GRAD ? 1 : 0), TK = 2 * LK + 1, M = 2 * LB + 2 * LK + (GRAD ? 1 : 0);
    const int Ms = N * (N + 1) / 2, v = kap * (kap + 1) / 2 + lam;
    const double *tg = tab + (int64_t)g * nprim * nprim * kGtoRow;
    const int km = ao.kind[mu], kn = ao.kind[nu], kk = ao.kind[kap], kl = ao.kind[lam];
    const int nm = spdf_nmono(km), nn = spdf_nmono(kn), nk = spdf_nmono(kk), nl = spdf_nmono(kl);
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
                            spdf_mono(kk, ik, pk[0], pk[1], pk[2], wk);
                            spdf_mono(kl, il, pl[0], pl[1], pl[2], wl);
                            double ek[3][TK];
#pragma unroll
                            for (int x = 0; x < 3; ++x)
                                spdf_ket_dim<LK>(pk[x], pl[x], kr[8 + x], kr[11 + x], kr[7], ek[x]);
                            for (int im = 0; im < nm; ++im)
                                for (int in = 0; in < nn; ++in) {
                                    int pm[3], pn[3];
                                    double wm, wn;
                                    spdf_mono(km, im, pm[0], pm[1], pm[2], wm);
                                    spdf_mono(kn, in, pn[0], pn[1], pn[2], wn);
                                    const double wt = (wk * wl) * (wm * wn);
                                    double A[3][M + 1], der[3][TB];
#pragma unroll
                                    for (int x = 0; x < 3; ++x) {
                                        double base[TB], c[M + 1];
                                        spdf_bra_dim<LB, TB>(pm[x], pn[x], br[5], br[8 + x], br[11 + x], br[7], base,
                                                             der[x]);
                                        spdf_fold<TB, TK, M>(base, ek[x], c);
                                        spdf_poly<M>(c, X[x], A[x]);
                                    }
                                    double yz[M + 1];
                                    gto_conv<M>(A[1], A[2], yz);
                                    acc = acc + wt * gto_dot<M>(H, A[0], yz);
                                    if (GRAD) {
                                        // electron gradient = - centre gradient; one direction at a time
                                        double c[M + 1], D[M + 1], oth[M + 1];
                                        spdf_fold<TB, TK, M>(der[0], ek[0], c);
                                        spdf_poly<M>(c, X[0], D);
                                        gx = gx - wt * gto_dot<M>(H, D, yz);
                                        spdf_fold<TB, TK, M>(der[1], ek[1], c);
                                        spdf_poly<M>(c, X[1], D);
                                        gto_conv<M>(A[0], A[2], oth);
                                        gy = gy - wt * gto_dot<M>(H, D, oth);
                                        spdf_fold<TB, TK, M>(der[2], ek[2], c);
                                        spdf_poly<M>(c, X[2], D);
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

// vs: the ket pair in the order of the functions sorted by l.  The class picks the body.
template <bool GRAD>
GTO_HD void spdf_two(int mu, int nu, int vs, int g, const SpdfAos &ao, const double *tab, int N, int nprim, int s4, int s2kl,
                     double *eri, double *ip1) {
    if (vs >= N * (N + 1) / 2) return;
    const int ra = gto_tri_row(vs), rb = vs - ra * (ra + 1) / 2;
    const int fa = ao.perm[ra], fb = ao.perm[rb];
    const int kap = fa > fb ? fa : fb, lam = fa > fb ? fb : fa;
    const int lm = spdf_l(ao.kind[mu]), ln = spdf_l(ao.kind[nu]);
    const int lb = lm > ln ? lm : ln, lk = spdf_l(ao.kind[fa]);   // (sorted: the l of perm[ra] is the higher one)
#define SPDF_CLASS(B, K)                                                                             \
    case (B) * 4 + (K):                                                                              \
        spdf_two_body<GRAD, B, K>(mu, nu, kap, lam, g, ao, tab, N, nprim, s4, s2kl, eri, ip1);       \
        break;
    switch (lb * 4 + lk) {
        SPDF_CLASS(0, 0) SPDF_CLASS(0, 1) SPDF_CLASS(0, 2) SPDF_CLASS(0, 3)
        SPDF_CLASS(1, 0) SPDF_CLASS(1, 1) SPDF_CLASS(1, 2) SPDF_CLASS(1, 3)
        SPDF_CLASS(2, 0) SPDF_CLASS(2, 1) SPDF_CLASS(2, 2) SPDF_CLASS(2, 3)
        SPDF_CLASS(3, 0) SPDF_CLASS(3, 1) SPDF_CLASS(3, 2) SPDF_CLASS(3, 3)
        default: break;
    }
#undef SPDF_CLASS
}

// GRAD: gridDim.y = N^2, blockIdx.y = mu N + nu; otherwise gridDim.y = Ms, blockIdx.y = mu (mu + 1) / 2 + nu.
// s4 / s2kl: the forms of eri / eri_ip1 (EVC_FLAG_ERI_S4 / EVC_FLAG_IP1_S2KL).
template <bool GRAD>
__global__ __launch_bounds__(64) void spdfgto_two_kernel(SpdfAos ao, const double *__restrict__ tab, int N, int nprim, int s4,
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
    spdf_two<GRAD>(mu, nu, blockIdx.x * 64 + threadIdx.x, blockIdx.z, ao, tab, N, nprim, s4, s2kl, eri, ip1);
}

// ---- one-electron integrals ------------------------------------------------------------------
// One dimension of the overlap of a primitive pair without sqrt(pi / p) and the exponential, s(i', j') for i' < NI,
// j' < NJ, by the Obara-Saika recursion.
template <int NI, int NJ>
GTO_HD void spdf_os_table(double XA, double XB, double ip, double (&s)[NI][NJ]) {
    s[0][0] = 1.0;
#pragma unroll
    for (int jj = 1; jj < NJ; ++jj) s[0][jj] = XB * s[0][jj - 1] + (jj > 1 ? ip * (jj - 1) * s[0][jj - 2] : 0.0);
#pragma unroll
    for (int ii = 1; ii < NI; ++ii)
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj)
            s[ii][jj] = XA * s[ii - 1][jj] + (ii > 1 ? ip * (ii - 1) * s[ii - 2][jj] : 0.0) +
                        (jj > 0 ? ip * jj * s[ii - 1][jj - 1] : 0.0);
}

// One dimension of overlap and kinetic energy of a primitive pair with the powers i, j (0 ... 3): from s(i', j') for
// i' <= 4, j' <= 5
//   out[0], out[1]   the overlap and -1/2 d^2/dx^2 on the second function,
//                    4 b^2 s(i, j+2) - 2 b (2j + 1) s(i, j) + j (j - 1) s(i, j-2)
//   out[2], out[3]   their derivatives for the centre of the first function, 2a (i + 1) - i (i - 1)
GTO_HD void spdf_st_dim(int i, int j, double a, double b, double XA, double XB, double ip, double (&out)[4]) {
    constexpr int P = kSpdfP;
    double s[P + 2][P + 3];
    spdf_os_table<P + 2, P + 3>(XA, XB, ip, s);
    const double b4 = 4.0 * b * b, b2 = 2.0 * b * (2 * j + 1), jj1 = (double)(j * (j - 1)), a2 = 2.0 * a, di = (double)i;
    // per row i' the overlap and the kinetic term at the columns of j
    double so[P + 2], tk[P + 2];
#pragma unroll
    for (int r = 0; r < P + 2; ++r) {
        double v0[P + 1], vp[P + 1], vm[P + 1];
#pragma unroll
        for (int k = 0; k <= P; ++k) {
            v0[k] = s[r][k];
            vp[k] = s[r][k + 2];
            vm[k] = k >= 2 ? s[r][k - 2] : 0.0;
        }
        const double c0 = spdf_sel<P>(j, v0), cp = spdf_sel<P>(j, vp), cm = spdf_sel<P>(j, vm);
        so[r] = c0;
        tk[r] = -0.5 * (b4 * cp - b2 * c0 + jj1 * cm);
    }
    double m0[P + 1], m1[P + 1], u0[P + 1], u1[P + 1], d0[P + 1], d1[P + 1];
#pragma unroll
    for (int k = 0; k <= P; ++k) {
        m0[k] = so[k];
        m1[k] = tk[k];
        u0[k] = so[k + 1];
        u1[k] = tk[k + 1];
        d0[k] = k > 0 ? so[k - 1] : 0.0;
        d1[k] = k > 0 ? tk[k - 1] : 0.0;
    }
    out[0] = spdf_sel<P>(i, m0);
    out[1] = spdf_sel<P>(i, m1);
    out[2] = a2 * spdf_sel<P>(i, u0) - di * spdf_sel<P>(i, d0);
    out[3] = a2 * spdf_sel<P>(i, u1) - di * spdf_sel<P>(i, d1);
}

// e = the contracted pair mu >= nu of geometry g.
template <bool GRAD>
GTO_HD void spdf_one_body(int e, int g, const SpdfAos &ao, const double *tab, const double *coords, const double *charges,
                          int N, int natm, int nprim, double *S, double *hcore, double *ipovlp, double *dhcore) {
    constexpr int P = kSpdfP, T = 2 * P + 2, M = GRAD ? 2 * P + 1 : 2 * P;
    if (e >= N * (N + 1) / 2) return;
    const int mu = gto_tri_row(e), nu = e - mu * (mu + 1) / 2;
    const int km = ao.kind[mu], kn = ao.kind[nu], am = ao.atom[mu], an = ao.atom[nu];
    const int nm = spdf_nmono(km), nn = spdf_nmono(kn);
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
                    spdf_mono(km, im, pm[0], pm[1], pm[2], wm);
                    spdf_mono(kn, in, pn[0], pn[1], pn[2], wn);
                    const double w = w0 * (wm * wn);
                    double d[3][4], sp, tp, ds[3], dt[3];
#pragma unroll
                    for (int x = 0; x < 3; ++x) spdf_st_dim(pm[x], pn[x], r[5], r[6], r[8 + x], r[11 + x], r[7], d[x]);
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
                            spdf_st_dim(pn[x], pm[x], r[6], r[5], r[11 + x], r[8 + x], r[7], d[x]);
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
                        spdf_mono(km, im, pm[0], pm[1], pm[2], wm);
                        spdf_mono(kn, in, pn[0], pn[1], pn[2], wn);
                        const double wt = wm * wn;
                        double A[3][M + 1], Da[3][M + 1], Db[3][M + 1], Op[3][M + 1];
#pragma unroll
                        for (int x = 0; x < 3; ++x) {
                            double base[T], der[T], same[T], c0[M + 1];
                            spdf_bra_dim<P, T>(pm[x], pn[x], r[5], r[8 + x], r[11 + x], r[7], base, der);
                            spdf_take<T, M>(base, c0);
                            spdf_poly<M>(c0, X[x], A[x]);
                            if (GRAD) {
                                spdf_take<T, M>(der, c0);
                                spdf_poly<M>(c0, X[x], Da[x]);
                                // d/dC of R_n(P - C) = -R_{n+1}
                                c0[0] = 0.0;
#pragma unroll
                                for (int n = 1; n <= M; ++n) c0[n] = -base[n - 1];
                                spdf_poly<M>(c0, X[x], Op[x]);
                                spdf_bra_dim<P, T>(pn[x], pm[x], r[6], r[11 + x], r[8 + x], r[7], same, der);
                                spdf_take<T, M>(der, c0);
                                spdf_poly<M>(c0, X[x], Db[x]);
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
__global__ __launch_bounds__(64) void spdfgto_one_kernel(SpdfAos ao, const double *__restrict__ tab,
                                                          const double *__restrict__ coords,
                                                          const double *__restrict__ charges, int N, int natm, int nprim,
                                                          double *S, double *hcore, double *ipovlp, double *dhcore) {
    spdf_one_body<GRAD>(blockIdx.x * 64 + threadIdx.x, blockIdx.y, ao, tab, coords, charges, N, natm, nprim, S, hcore,
                        ipovlp, dhcore);
}

// ---- nuclear repulsion -------------------------------------------------------------------------
// blockIdx.x = geometry; thread i < natm sums over the other centres in ascending order.
template <bool GRAD>
__global__ __launch_bounds__(64) void spdfgto_nuc_kernel(const double *__restrict__ coords, const double *__restrict__ charges,
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
GTO_HD void spdf_dipole_body(int e, int g, const SpdfPrims &bs, const SpdfAos &ao, const double *coords, int N, int natm,
                             double ox, double oy, double oz, double *dip) {
    constexpr int P = kSpdfP;
    if (e >= N * (N + 1) / 2) return;
    const int mu = gto_tri_row(e), nu = e - mu * (mu + 1) / 2;
    const int km = ao.kind[mu], kn = ao.kind[nu];
    const int nm = spdf_nmono(km), nn = spdf_nmono(kn);
    const double *Ra = coords + ((int64_t)g * natm + ao.atom[mu]) * 3, *Rb = coords + ((int64_t)g * natm + ao.atom[nu]) * 3;
    const double O[3] = {ox, oy, oz};
    double acc[3] = {0.0, 0.0, 0.0};
    for (int pa = ao.off[mu]; pa < ao.off[mu] + ao.np[mu]; ++pa)
        for (int pb = ao.off[nu]; pb < ao.off[nu] + ao.np[nu]; ++pb) {
            const double a = bs.ex[pa], b = bs.ex[pb], p = a + b, mup = a * b / p, ip = 0.5 / p;
            double r2 = 0.0, tb[3][P + 2][P + 1];
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const double d = Ra[x] - Rb[x];
                r2 = r2 + d * d;
                spdf_os_table<P + 2, P + 1>(-(b / p) * d, (a / p) * d, ip, tb[x]);
            }
            const double pip = kGtoPi / p, w0 = pip * sqrt(pip) * exp(-mup * r2) * bs.cn[pa] * bs.cn[pb];
            for (int im = 0; im < nm; ++im)
                for (int in = 0; in < nn; ++in) {
                    int pm[3], pn[3];
                    double wm, wn, s0[3], s1[3];
                    spdf_mono(km, im, pm[0], pm[1], pm[2], wm);
                    spdf_mono(kn, in, pn[0], pn[1], pn[2], wn);
#pragma unroll
                    for (int x = 0; x < 3; ++x) {
                        // s(i', j) for i' <= 4 at the column j
                        double col[P + 2], lo[P + 1], hi[P + 1];
#pragma unroll
                        for (int r = 0; r < P + 2; ++r) col[r] = spdf_sel<P>(pn[x], tb[x][r]);
#pragma unroll
                        for (int k = 0; k <= P; ++k) {
                            lo[k] = col[k];
                            hi[k] = col[k + 1];
                        }
                        s0[x] = spdf_sel<P>(pm[x], lo);
                        s1[x] = spdf_sel<P>(pm[x], hi) + (Ra[x] - O[x]) * s0[x];
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

__global__ __launch_bounds__(64) void spdfgto_dipole_kernel(SpdfPrims bs, SpdfAos ao, const double *__restrict__ coords, int N,
                                                             int natm, double ox, double oy, double oz,
                                                             double *__restrict__ dip) {
    spdf_dipole_body(blockIdx.x * 64 + threadIdx.x, blockIdx.y, bs, ao, coords, N, natm, ox, oy, oz, dip);
}

// ---- gradient of the dipole integrals ------------------------------------------------------------
// idx = mu N + nu of geometry g.  Per dimension and monomial pair: the overlap factor s0 and the dipole factor
// r0 = s(i + 1) + (A - O) s(i), and their derivatives for the centre of mu, 2a f(i + 1) - i f(i - 1); s(i', j) for
// i' <= 5 (the centre derivative and the operator each raise the first power by one).
GTO_HD void spdf_dipole_grad_body(int idx, int g, const SpdfPrims &bs, const SpdfAos &ao, const double *coords, int N,
                                  int natm, double ox, double oy, double oz, double *ipdip) {
    constexpr int P = kSpdfP;
    if (idx >= N * N) return;
    const int mu = idx / N, nu = idx - mu * N;
    const int km = ao.kind[mu], kn = ao.kind[nu];
    const int nm = spdf_nmono(km), nn = spdf_nmono(kn);
    const double *Ra = coords + ((int64_t)g * natm + ao.atom[mu]) * 3, *Rb = coords + ((int64_t)g * natm + ao.atom[nu]) * 3;
    const double AO[3] = {Ra[0] - ox, Ra[1] - oy, Ra[2] - oz};
    double acc[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    for (int pa = ao.off[mu]; pa < ao.off[mu] + ao.np[mu]; ++pa)
        for (int pb = ao.off[nu]; pb < ao.off[nu] + ao.np[nu]; ++pb) {
            const double a = bs.ex[pa], b = bs.ex[pb], p = a + b, mup = a * b / p, ip = 0.5 / p, a2 = 2.0 * a;
            double r2 = 0.0, tb[3][P + 3][P + 1];
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const double d = Ra[x] - Rb[x];
                r2 = r2 + d * d;
                spdf_os_table<P + 3, P + 1>(-(b / p) * d, (a / p) * d, ip, tb[x]);
            }
            const double pip = kGtoPi / p, w0 = pip * sqrt(pip) * exp(-mup * r2) * bs.cn[pa] * bs.cn[pb];
            for (int im = 0; im < nm; ++im)
                for (int in = 0; in < nn; ++in) {
                    int pm[3], pn[3];
                    double wm, wn, s0[3], r0[3], ds[3], dr[3];
                    spdf_mono(km, im, pm[0], pm[1], pm[2], wm);
                    spdf_mono(kn, in, pn[0], pn[1], pn[2], wn);
#pragma unroll
                    for (int x = 0; x < 3; ++x) {
                        double col[P + 3], v0[P + 1], vm[P + 1], v1[P + 1], v2[P + 1];
#pragma unroll
                        for (int r = 0; r < P + 3; ++r) col[r] = spdf_sel<P>(pn[x], tb[x][r]);
#pragma unroll
                        for (int k = 0; k <= P; ++k) {
                            v0[k] = col[k];
                            vm[k] = k > 0 ? col[k - 1] : 0.0;
                            v1[k] = col[k + 1];
                            v2[k] = col[k + 2];
                        }
                        const int i = pm[x];
                        const double di = (double)i;
                        const double sm = spdf_sel<P>(i, vm), sp1 = spdf_sel<P>(i, v1), sp2 = spdf_sel<P>(i, v2);
                        s0[x] = spdf_sel<P>(i, v0);
                        r0[x] = sp1 + AO[x] * s0[x];
                        ds[x] = a2 * sp1 - di * sm;
                        dr[x] = a2 * (sp2 + AO[x] * sp1) - di * (s0[x] + AO[x] * sm);
                    }
                    const double w = w0 * (wm * wn);
#pragma unroll
                    for (int x = 0; x < 3; ++x) {
                        const int y = (x + 1) % 3, z = (x + 2) % 3;
                        acc[x][x] = fma(w, dr[x] * s0[y] * s0[z], acc[x][x]);
                        acc[x][y] = fma(w, ds[x] * r0[y] * s0[z], acc[x][y]);
                        acc[x][z] = fma(w, ds[x] * s0[y] * r0[z], acc[x][z]);
                    }
                }
        }
    const int64_t n2 = (int64_t)N * N;
    double *o = ipdip + (int64_t)g * 9 * n2 + idx;
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(int64_t)(x * 3 + c) * n2] = -acc[x][c];   // electron gradient = - centre gradient
}

__global__ __launch_bounds__(64) void spdfgto_dipole_grad_kernel(SpdfPrims bs, SpdfAos ao, const double *__restrict__ coords,
                                                                  int N, int natm, double ox, double oy, double oz,
                                                                  double *__restrict__ ipdip) {
    spdf_dipole_grad_body(blockIdx.x * 64 + threadIdx.x, blockIdx.y, bs, ao, coords, N, natm, ox, oy, oz, ipdip);
}

// ---- host side: the route for gto_shells.hpp -----------------------------------------------------
struct SpdfRoute {
    using Prims = SpdfPrims;
    using Aos = SpdfAos;
    static constexpr int kMaxL = 3;
    static constexpr const char *kLs = "0, 1, 2 and 3", *kName = "spdfgto";
    // gto_describe sets off / np of function f before it calls tag, in ascending f; padding has no primitives and stays
    // where it is, a function is inserted behind those of its own and of lower l
    static void tag(SpdfAos &ao, int f, int l, int c) {
        ao.kind[f] = (uint8_t)(l == 0 ? 0 : (l == 1 ? 1 + c : (l == 2 ? 4 + c : 9 + c)));
        int at = f;
        if (ao.np[f] != 0)
            for (; at > 0 && spdf_l(ao.kind[ao.perm[at - 1]]) > l; --at) ao.perm[at] = ao.perm[at - 1];
        ao.perm[at] = (uint8_t)f;
    }
    static constexpr auto kPair = spdfgto_pair_kernel;
    static constexpr auto kOne = spdfgto_one_kernel<true>, kOneE = spdfgto_one_kernel<false>;
    static constexpr auto kNuc = spdfgto_nuc_kernel<true>, kNucE = spdfgto_nuc_kernel<false>;
    static constexpr auto kTwo = spdfgto_two_kernel<true>, kTwoE = spdfgto_two_kernel<false>;
    static constexpr auto kDipole = spdfgto_dipole_kernel;
};

static bool spdf_aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace evc

using namespace evc;

extern "C" size_t evc_spdfgto_workspace_bytes(int natm, int nshell, int nprim_total, int nao, int count) {
    return gto_workspace_bytes<SpdfRoute>("evc_spdfgto_workspace_bytes", natm, nshell, nprim_total, nao, count);
}

extern "C" int evc_spdfgto_integrals_batch(int natm, int nshell, int count, const double *coords, const double *charges,
                                           const int *shell_atom, const int *shell_l, const int *shell_prim_offset,
                                           const double *exponents, const double *coefficients, const evc_sgto_outputs *out,
                                           int flags, void *ws, size_t ws_bytes, void *stream) {
    return gto_integrals_batch<SpdfRoute>("evc_spdfgto_integrals_batch", natm, nshell, count, coords, charges, shell_atom,
                                          shell_l, shell_prim_offset, exponents, coefficients, out, flags, ws, ws_bytes,
                                          stream);
}

extern "C" int evc_spdfgto_dipole_batch(int natm, int nshell, int count, const double *coords, const int *shell_atom,
                                        const int *shell_l, const int *shell_prim_offset, const double *exponents,
                                        const double *coefficients, const double origin[3], double *dip, void *stream) {
    return gto_dipole_batch<SpdfRoute>("evc_spdfgto_dipole_batch", natm, nshell, count, coords, shell_atom, shell_l,
                                       shell_prim_offset, exponents, coefficients, origin, dip, stream);
}

extern "C" int evc_spdfgto_dipole_grad_batch(int natm, int nshell, int count, const double *coords, const int *shell_atom,
                                             const int *shell_l, const int *shell_prim_offset, const double *exponents,
                                             const double *coefficients, const double origin[3], double *ipdip,
                                             void *stream) {
    const char *who = "evc_spdfgto_dipole_grad_batch";
    SpdfPrims bs;
    SpdfAos ao;
    int nprim = 0, N = 0;
    if (int rc = gto_describe<SpdfRoute>(who, natm, nshell, count, shell_atom, shell_l, shell_prim_offset, exponents,
                                         coefficients, bs, ao, nprim, N))
        return rc;
    EVC_REQUIRE(coords && origin && ipdip, "%s: null pointer", who);
    EVC_REQUIRE(spdf_aligned8(coords) && spdf_aligned8(ipdip), "%s: misaligned pointer (8 bytes)", who);
    gto_launch(spdfgto_dipole_grad_kernel, dim3((unsigned)ceil_div((int64_t)N * N, 64), (unsigned)count), dim3(64),
               as_stream(stream), bs, ao, coords, N, natm, origin[0], origin[1], origin[2], ipdip);
    EVC_LAUNCH_CHECK("spdfgto_dipole_grad_kernel");
    return 0;
}
