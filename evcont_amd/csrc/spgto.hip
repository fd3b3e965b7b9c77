// AO integrals and their first nuclear derivatives of a molecule built from contracted Cartesian s and p Gaussian shells
// (evc_spgto_integrals_batch, evc_spgto_dipole_batch): the device statement of evcont_amd/gto_small.py sp_gaussian_mol,
// written straight into the arrays of an evc_geometry_batch.  sgto.hip stays the route for one s function per centre.
//
// Scheme: McMurchie-Davidson, with the Hermite Coulomb integrals kept factored.  Per dimension the product of two
// primitives x_A^i x_B^j is sum_t E_t^{ij} Lambda_t (sp_raise: E^{i+1,j}_t = E_{t-1} / 2p + X_PA E_t + (t + 1) E_{t+1}; the
// exponential factor is kept apart, in the pair table).  The bra and ket expansions of one dimension fold into one
// coefficient array c[n] = sum_{t + tau = n} E_t (-1)^tau E'_tau, and, since the recursion of R_tuv acts on each dimension
// alone (R^m_{n+1} = n R^{m+1}_{n-1} + X R^{m+1}_n), the derivative d^n/dX^n is sum_j a_{n,j}(X) (raise the order m by j)
// with a_{n,j} = n! / ((n - j)! (2j - n)! 2^{n - j}) X^{2j - n}.  So each dimension gives a short array
// A[j] = sum_n c[n] a_{n,j}(X) (sp_poly) and an integral is
//     sum_m H[m] sum_{j + k + l = m} Ax[j] Ay[k] Az[l],    H[m] = w (-2 alpha)^m F_m(alpha |PQ|^2),  m <= 5,
// all loops with fixed bounds, everything in registers.  A derivative with respect to the centre of the first function
// is 2a (i + 1) - i (i - 1) in the power of that dimension: it replaces the E array of ONE dimension, so the three
// components of int2e_ip1 reuse the other two dimensions' arrays of int2e.
// Boys functions (sp_boys): below t = 12 the convergent series of the highest order, then downward recursion
// F_{n-1} = (2t F_n + e^-t) / (2n - 1); above it F0 from erf and upward recursion.
//
// Kernels, each a launch of its own (FP64 VALU; DESIGN.md: FP64 MFMA blocks its SIMD's vector issue):
//   spgto_pair_kernel    the primitive-pair table: per geometry one row of kSpRow doubles per ORDERED pair of primitive
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
#include <math.h>
#include <stdint.h>

#include "common.hpp"

namespace evc {

constexpr int kSpMaxAtoms = 64;        // centres
constexpr int kSpMaxAo = 64;           // contracted functions
constexpr int kSpMaxShells = 64;
constexpr int kSpMaxShellPrim = 8;     // primitives of one shell
constexpr int kSpMaxPrim = 128;        // primitives of all shells
constexpr int kSpMaxCount = 65535;     // geometries per call (gridDim.z)
constexpr int kSpRow = 14;             // doubles of a row of the pair table
constexpr int kSpFlags = EVC_FLAG_ENERGY_ONLY | EVC_FLAG_ERI_S4 | EVC_FLAG_IP1_S2KL;
constexpr double kSpBoysCrossover = 12.0;
constexpr double kSpPi = 3.141592653589793;

struct SpPrims {
    double ex[kSpMaxPrim];      // exponents
    double cn[kSpMaxPrim];      // coefficient x norm of the primitive
    uint8_t atom[kSpMaxPrim];   // its centre
};
struct SpAos {
    uint8_t off[kSpMaxAo];      // first primitive of the function's shell
    uint8_t np[kSpMaxAo];       // primitives of the shell
    int8_t dir[kSpMaxAo];       // -1: s; 0, 1, 2: p_x, p_y, p_z
    uint8_t atom[kSpMaxAo];
};

// Every launch of this file: the runtime call, not the chevrons (tests/test_spgto_closure.py).
template <typename T>
struct spgto_same_type {
    using type = T;
};
template <typename... P>
static void spgto_launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t st,
                         typename spgto_same_type<P>::type... a) {
    void *args[] = {(void *)&a...};
    // the result is read by the EVC_LAUNCH_CHECK (hipGetLastError) that follows the call
    (void)hipLaunchKernel(reinterpret_cast<const void *>(kernel), grid, block, args, 0, st);
}

#define SP_HD __host__ __device__ __forceinline__

// row of the packed index m = row (row + 1) / 2 + col, col <= row
SP_HD int sp_tri_row(int m) {
    int r = (int)((sqrt(8.0 * m + 1.0) - 1.0) * 0.5);
    if (r * (r + 1) / 2 > m) --r;
    if ((r + 1) * (r + 2) / 2 <= m) ++r;
    return r;
}

// Eight more terms of the series of F_L from term K0 on, and eight more while they still count.
template <int L, int K0>
SP_HD void sp_series(double t2, double &term, double &s) {
#pragma unroll
    for (int k = K0; k < K0 + 8; ++k) {
        term = term * (t2 * (1.0 / (2 * L + 2 * k + 1)));
        s = s + term;
    }
    if constexpr (K0 + 8 < 64) {
        if (!(term < s * 1e-17)) sp_series<L, K0 + 8>(t2, term, s);
    }
}

// F_0 ... F_L of t in f[0 .. L].
template <int L>
SP_HD void sp_boys(double t, double (&f)[L + 1]) {
    if (t < kSpBoysCrossover) {
        // F_L(t) = e^-t sum_k (2t)^k / ((2L + 1)(2L + 3) ... (2L + 2k + 1)): all terms positive, at most 65 of them
        const double t2 = 2.0 * t, et = exp(-t);
        double term = 1.0 / (2 * L + 1), s = term;
        sp_series<L, 1>(t2, term, s);
        f[L] = et * s;
#pragma unroll
        for (int n = L; n > 0; --n) f[n - 1] = (t2 * f[n] + et) * (1.0 / (2 * n - 1));
    } else {
        const double rt = sqrt(t), et = exp(-t), i2t = 0.5 / t;
        f[0] = 0.8862269254527579 / rt * erf(rt);   // sqrt(pi) / 2
#pragma unroll
        for (int n = 0; n < L; ++n) f[n + 1] = ((2 * n + 1) * f[n] - et) * i2t;
    }
}

// One more power on a function whose centre is X away from P: o[t] = e[t-1] / 2p + X e[t] + (t + 1) e[t+1].
template <int T>
SP_HD void sp_raise(const double (&e)[T], double X, double ip, double (&o)[T]) {
#pragma unroll
    for (int t = 0; t < T; ++t)
        o[t] = (t > 0 ? ip * e[t - 1] : 0.0) + X * e[t] + (t + 1 < T ? (t + 1) * e[t + 1] : 0.0);
}

// Hermite coefficients (t <= 3) of one dimension of a primitive pair with the powers i, j (0 or 1), without the
// exponential: `base` = E^{ij}, `der` = those of d/dA, 2a E^{i+1,j} - i E^{i-1,j}.  XA = P - A, XB = P - B, ip = 1 / 2p.
SP_HD void sp_bra_dim(bool i, bool j, double a, double XA, double XB, double ip, double (&base)[4], double (&der)[4]) {
    const double e0[4] = {1.0, 0.0, 0.0, 0.0};
    double r[4], ej[4], e1[4], e2[4];
    sp_raise(e0, XB, ip, r);
#pragma unroll
    for (int t = 0; t < 4; ++t) ej[t] = j ? r[t] : e0[t];
    sp_raise(ej, XA, ip, e1);
    sp_raise(e1, XA, ip, e2);
    const double a2 = 2.0 * a;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        base[t] = i ? e1[t] : ej[t];
        der[t] = i ? a2 * e2[t] - ej[t] : a2 * e1[t];
    }
}

// (-1)^tau E^{kl}_tau (tau <= 2) of one dimension of the ket pair.
SP_HD void sp_ket_dim(bool k, bool l, double XC, double XD, double ip, double (&o)[3]) {
    const double e0[3] = {1.0, 0.0, 0.0};
    double r[3], el[3], e1[3];
    sp_raise(e0, XD, ip, r);
#pragma unroll
    for (int t = 0; t < 3; ++t) el[t] = l ? r[t] : e0[t];
    sp_raise(el, XC, ip, e1);
    o[0] = k ? e1[0] : el[0];
    o[1] = -(k ? e1[1] : el[1]);
    o[2] = k ? e1[2] : el[2];
}

// c[n] = sum_{t + tau = n} b[t] k[tau], n <= M.
template <int M>
SP_HD void sp_fold(const double (&b)[4], const double (&k)[3], double (&c)[M + 1]) {
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
SP_HD double sp_at(const double (&c)[M + 1]) {
    if constexpr (N <= M) return c[N];
    return 0.0;
}

// A[j] = sum_n c[n] a_{n,j}(X): the derivatives d^n/dX^n of a function of alpha |R|^2 as raises of its order.
template <int M>
SP_HD void sp_poly(const double (&c)[M + 1], double X, double (&A)[M + 1]) {
    const double X2 = X * X, X3 = X2 * X;
    const double c1 = sp_at<M, 1>(c), c2 = sp_at<M, 2>(c), c3 = sp_at<M, 3>(c), c4 = sp_at<M, 4>(c), c5 = sp_at<M, 5>(c);
    const double v[6] = {c[0], c1 * X + c2, c2 * X2 + 3.0 * (c3 * X + c4), c3 * X3 + 6.0 * c4 * X2 + 15.0 * c5 * X,
                         c4 * X2 * X2 + 10.0 * c5 * X3, c5 * X3 * X2};
#pragma unroll
    for (int j = 0; j <= M; ++j) A[j] = v[j];
}

// W[m] = sum_{j + k = m} U[j] V[k], m <= M.
template <int M>
SP_HD void sp_conv(const double (&U)[M + 1], const double (&V)[M + 1], double (&W)[M + 1]) {
#pragma unroll
    for (int m = 0; m <= M; ++m) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j <= m; ++j) s = fma(U[j], V[m - j], s);
        W[m] = s;
    }
}

// sum_m H[m] W[m]
template <int M>
SP_HD double sp_dot(const double (&H)[M + 1], const double (&U)[M + 1], const double (&V)[M + 1]) {
    double W[M + 1], s = 0.0;
    sp_conv<M>(U, V, W);
#pragma unroll
    for (int m = 0; m <= M; ++m) s = fma(H[m], W[m], s);
    return s;
}

// ---- pair table ------------------------------------------------------------------------
// idx = pa nprim + pb of geometry g
SP_HD void sp_pair_body(int idx, int g, const SpPrims &bs, const double *coords, int natm, int nprim, double *tab) {
    if (idx >= nprim * nprim) return;
    const int pa = idx / nprim, pb = idx - pa * nprim;
    const double a = bs.ex[pa], b = bs.ex[pb];
    const double *Ra = coords + ((int64_t)g * natm + bs.atom[pa]) * 3, *Rb = coords + ((int64_t)g * natm + bs.atom[pb]) * 3;
    const double p = a + b, mu = a * b / p;
    double *row = tab + ((int64_t)g * nprim * nprim + idx) * kSpRow;
    double r2 = 0.0;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const double A = Ra[x], B = Rb[x], d = A - B;
        r2 = r2 + d * d;
        // where A_x = B_x (a pair on one centre) P_x is A_x exactly: P - Q and P - C vanish exactly where they do
        // mathematically; P - A and P - B come from A - B and vanish with it
        row[1 + x] = A == B ? A : (a * A + b * B) / p;
        row[8 + x] = -(b / p) * d;
        row[11 + x] = (a / p) * d;
    }
    row[0] = p;
    row[4] = exp(-mu * r2) * bs.cn[pa] * bs.cn[pb];
    row[5] = a;
    row[6] = b;
    row[7] = 0.5 / p;
}

__global__ __launch_bounds__(256) void spgto_pair_kernel(SpPrims bs, const double *__restrict__ coords, int natm, int nprim,
                                                          double *__restrict__ tab) {
    sp_pair_body(blockIdx.x * 256 + threadIdx.x, blockIdx.y, bs, coords, natm, nprim, tab);
}

// ---- two-electron integrals ----------------------------------------------------------------
// M: the highest Hermite order, 5 with the gradient and 4 without.
template <bool GRAD>
SP_HD void sp_two_body(int mu, int nu, int v, int g, const SpAos &ao, const double *tab, int N, int nprim, int s4, int s2kl,
                       double *eri, double *ip1) {
    constexpr int M = GRAD ? 5 : 4;
    const int Ms = N * (N + 1) / 2;
    if (v >= Ms) return;
    const int kap = sp_tri_row(v), lam = v - kap * (kap + 1) / 2;
    const double *tg = tab + (int64_t)g * nprim * nprim * kSpRow;
    const int dm = ao.dir[mu], dn = ao.dir[nu], dk = ao.dir[kap], dl = ao.dir[lam];
    double acc = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    for (int pc = ao.off[kap]; pc < ao.off[kap] + ao.np[kap]; ++pc)
        for (int pd = ao.off[lam]; pd < ao.off[lam] + ao.np[lam]; ++pd) {
            const double *kr = tg + ((int64_t)pc * nprim + pd) * kSpRow;
            const double q = kr[0], qx = kr[1], qy = kr[2], qz = kr[3], ck = kr[4];
            double ek[3][3];
#pragma unroll
            for (int x = 0; x < 3; ++x) sp_ket_dim(dk == x, dl == x, kr[8 + x], kr[11 + x], kr[7], ek[x]);
            for (int pa = ao.off[mu]; pa < ao.off[mu] + ao.np[mu]; ++pa)
                for (int pb = ao.off[nu]; pb < ao.off[nu] + ao.np[nu]; ++pb) {
                    const double *br = tg + ((int64_t)pa * nprim + pb) * kSpRow;
                    const double p = br[0], X[3] = {br[1] - qx, br[2] - qy, br[3] - qz};
                    const double s = p + q, pq = p * q;
                    const double alpha = pq / s;
                    double H[M + 1];
                    sp_boys<M>(alpha * (X[0] * X[0] + X[1] * X[1] + X[2] * X[2]), H);
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
                    sp_conv<M>(A[1], A[2], yz);
                    acc = acc + sp_dot<M>(H, A[0], yz);
                    if (GRAD) {
                        double xz[M + 1], xy[M + 1];
                        sp_conv<M>(A[0], A[2], xz);
                        sp_conv<M>(A[0], A[1], xy);
                        // electron gradient = - centre gradient
                        gx = gx - sp_dot<M>(H, D[0], yz);
                        gy = gy - sp_dot<M>(H, D[1], xz);
                        gz = gz - sp_dot<M>(H, D[2], xy);
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
SP_HD void sp_st_dim(bool i, bool j, double a, double b, double XA, double XB, double ip, double (&out)[4]) {
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

// Overlap s, kinetic energy t and their derivatives for the centre of the first function of one primitive pair (without
// the pair's weight): d[x] of three dimensions.
SP_HD void sp_overlap_kinetic(const double (&d)[3][4], double &s, double &t, double (&ds)[3], double (&dt)[3]) {
    s = d[0][0] * d[1][0] * d[2][0];
    t = d[0][1] * d[1][0] * d[2][0] + d[0][0] * d[1][1] * d[2][0] + d[0][0] * d[1][0] * d[2][1];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const int y = (x + 1) % 3, z = (x + 2) % 3;
        ds[x] = d[x][2] * d[y][0] * d[z][0];
        dt[x] = d[x][3] * d[y][0] * d[z][0] + d[x][2] * (d[y][1] * d[z][0] + d[y][0] * d[z][1]);
    }
}

// e = the contracted pair mu >= nu of geometry g.
template <bool GRAD>
SP_HD void sp_one_body(int e, int g, const SpAos &ao, const double *tab, const double *coords, const double *charges, int N,
                       int natm, int nprim, double *S, double *hcore, double *ipovlp, double *dhcore) {
    constexpr int M = 3;
    if (e >= N * (N + 1) / 2) return;
    const int mu = sp_tri_row(e), nu = e - mu * (mu + 1) / 2;
    const int dm = ao.dir[mu], dn = ao.dir[nu], am = ao.atom[mu], an = ao.atom[nu];
    const double *Rg = coords + (int64_t)g * natm * 3;
    const double *tg = tab + (int64_t)g * nprim * nprim * kSpRow;
    const int64_t n2 = (int64_t)N * N, ij = (int64_t)mu * N + nu, ji = (int64_t)nu * N + mu;
    // overlap and kinetic energy; dsa, dta: derivatives for the centre of mu; dsb, dtb: for the centre of nu
    double s = 0.0, tk = 0.0, dsa[3] = {0.0, 0.0, 0.0}, dta[3] = {0.0, 0.0, 0.0}, dsb[3] = {0.0, 0.0, 0.0},
           dtb[3] = {0.0, 0.0, 0.0};
    for (int pa = ao.off[mu]; pa < ao.off[mu] + ao.np[mu]; ++pa)
        for (int pb = ao.off[nu]; pb < ao.off[nu] + ao.np[nu]; ++pb) {
            const double *r = tg + ((int64_t)pa * nprim + pb) * kSpRow;
            const double pip = kSpPi / r[0], w = pip * sqrt(pip) * r[4];
            double d[3][4], sp, tp, ds[3], dt[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) sp_st_dim(dm == x, dn == x, r[5], r[6], r[8 + x], r[11 + x], r[7], d[x]);
            sp_overlap_kinetic(d, sp, tp, ds, dt);
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
                sp_overlap_kinetic(d, sp, tp, ds, dt);
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
                const double *r = tg + ((int64_t)pa * nprim + pb) * kSpRow;
                const double p = r[0], X[3] = {r[1] - C[0], r[2] - C[1], r[3] - C[2]};
                double H[M + 1];
                sp_boys<M>(p * (X[0] * X[0] + X[1] * X[1] + X[2] * X[2]), H);
                double w = -z * (2.0 * kSpPi / p) * r[4];
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
                sp_conv<M>(A[1], A[2], yz);
                vn = vn + sp_dot<M>(H, A[0], yz);
                if (GRAD) {
                    double xz[M + 1], xy[M + 1];
                    sp_conv<M>(A[0], A[2], xz);
                    sp_conv<M>(A[0], A[1], xy);
                    dva[0] = dva[0] + sp_dot<M>(H, Da[0], yz);
                    dva[1] = dva[1] + sp_dot<M>(H, Da[1], xz);
                    dva[2] = dva[2] + sp_dot<M>(H, Da[2], xy);
                    dvb[0] = dvb[0] + sp_dot<M>(H, Db[0], yz);
                    dvb[1] = dvb[1] + sp_dot<M>(H, Db[1], xz);
                    dvb[2] = dvb[2] + sp_dot<M>(H, Db[2], xy);
                    op[0] = op[0] + sp_dot<M>(H, Op[0], yz);
                    op[1] = op[1] + sp_dot<M>(H, Op[1], xz);
                    op[2] = op[2] + sp_dot<M>(H, Op[2], xy);
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
SP_HD void sp_dipole_body(int e, int g, const SpPrims &bs, const SpAos &ao, const double *coords, int N, int natm,
                          double ox, double oy, double oz, double *dip) {
    if (e >= N * (N + 1) / 2) return;
    const int mu = sp_tri_row(e), nu = e - mu * (mu + 1) / 2;
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
            const double pip = kSpPi / p, w = pip * sqrt(pip) * exp(-mup * r2) * bs.cn[pa] * bs.cn[pb];
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

// ---- host side ---------------------------------------------------------------------------------
static int spgto_shape(const char *who, int natm, int nshell, int nprim, int nao, int count) {
    EVC_REQUIRE(natm >= 1 && natm <= kSpMaxAtoms, "%s: natm=%d, supported 1 ... %d", who, natm, kSpMaxAtoms);
    EVC_REQUIRE(nshell >= 1 && nshell <= kSpMaxShells, "%s: nshell=%d, supported 1 ... %d", who, nshell, kSpMaxShells);
    EVC_REQUIRE(nprim >= nshell && nprim <= kSpMaxPrim, "%s: nprim_total=%d, supported nshell ... %d", who, nprim,
                kSpMaxPrim);
    EVC_REQUIRE(nao >= nshell && nao <= kSpMaxAo && nao <= 3 * nshell, "%s: nao=%d, supported nshell ... %d", who, nao,
                kSpMaxAo);
    EVC_REQUIRE(count >= 1 && count <= kSpMaxCount, "%s: count=%d, supported 1 ... %d", who, count, kSpMaxCount);
    return 0;
}

static size_t spgto_table_bytes(int nprim, int count) {
    return align_up((size_t)count * nprim * nprim * kSpRow * sizeof(double), 256);
}

// The basis as the kernels take it; every refusal that concerns it.
static int spgto_describe(const char *who, int natm, int nshell, int count, const int *shell_atom, const int *shell_l,
                          const int *shell_prim_offset, const double *exponents, const double *coefficients, SpPrims &bs,
                          SpAos &ao, int &nprim, int &nao) {
    EVC_REQUIRE(natm >= 1 && natm <= kSpMaxAtoms, "%s: natm=%d, supported 1 ... %d", who, natm, kSpMaxAtoms);
    EVC_REQUIRE(nshell >= 1 && nshell <= kSpMaxShells, "%s: nshell=%d, supported 1 ... %d", who, nshell, kSpMaxShells);
    EVC_REQUIRE(shell_atom && shell_l && shell_prim_offset && exponents && coefficients, "%s: null pointer", who);
    EVC_REQUIRE(shell_prim_offset[0] == 0, "%s: shell_prim_offset[0]=%d, must be 0", who, shell_prim_offset[0]);
    nao = 0;
    for (int s = 0; s < nshell; ++s) {
        const int l = shell_l[s], k = shell_prim_offset[s + 1] - shell_prim_offset[s];
        EVC_REQUIRE(l == 0 || l == 1, "%s: shell %d has l=%d, supported 0 and 1", who, s, l);
        EVC_REQUIRE(k >= 1 && k <= kSpMaxShellPrim, "%s: shell %d has %d primitives, supported 1 ... %d", who, s, k,
                    kSpMaxShellPrim);
        EVC_REQUIRE(shell_prim_offset[s + 1] <= kSpMaxPrim, "%s: more than %d primitives in all", who, kSpMaxPrim);
        EVC_REQUIRE(shell_atom[s] >= 0 && shell_atom[s] < natm, "%s: shell_atom[%d]=%d outside 0 ... natm-1", who, s,
                    shell_atom[s]);
        EVC_REQUIRE(s == 0 || shell_atom[s] >= shell_atom[s - 1], "%s: shell_atom must be ascending (shell %d)", who, s);
        nao += 2 * l + 1;
    }
    nprim = shell_prim_offset[nshell];
    if (int rc = spgto_shape(who, natm, nshell, nprim, nao, count)) return rc;
    int f = 0;
    for (int s = 0; s < nshell; ++s) {
        for (int k = shell_prim_offset[s]; k < shell_prim_offset[s + 1]; ++k) {
            const double a = exponents[k];
            EVC_REQUIRE(a > 0.0 && isfinite(a), "%s: exponent %d is %g, must be positive", who, k, a);
            const double norm = pow(2.0 * a / kSpPi, 0.75) * (shell_l[s] == 1 ? 2.0 * sqrt(a) : 1.0);
            bs.ex[k] = a;
            bs.cn[k] = coefficients[k] * norm;
            bs.atom[k] = (uint8_t)shell_atom[s];
        }
        for (int c = 0; c < 2 * shell_l[s] + 1; ++c, ++f) {
            ao.off[f] = (uint8_t)shell_prim_offset[s];
            ao.np[f] = (uint8_t)(shell_prim_offset[s + 1] - shell_prim_offset[s]);
            ao.dir[f] = (int8_t)(shell_l[s] == 1 ? c : -1);
            ao.atom[f] = (uint8_t)shell_atom[s];
        }
    }
    for (int k = nprim; k < kSpMaxPrim; ++k) {
        bs.ex[k] = 1.0;
        bs.cn[k] = 0.0;
        bs.atom[k] = 0;
    }
    for (; f < kSpMaxAo; ++f) {
        ao.off[f] = 0;
        ao.np[f] = 0;
        ao.dir[f] = -1;
        ao.atom[f] = 0;
    }
    return 0;
}

}  // namespace evc

using namespace evc;

extern "C" size_t evc_spgto_workspace_bytes(int natm, int nshell, int nprim_total, int nao, int count) {
    if (spgto_shape("evc_spgto_workspace_bytes", natm, nshell, nprim_total, nao, count)) return 0;
    return spgto_table_bytes(nprim_total, count);
}

extern "C" int evc_spgto_integrals_batch(int natm, int nshell, int count, const double *coords, const double *charges,
                                         const int *shell_atom, const int *shell_l, const int *shell_prim_offset,
                                         const double *exponents, const double *coefficients, const evc_sgto_outputs *out,
                                         int flags, void *ws, size_t ws_bytes, void *stream) {
    const char *who = "evc_spgto_integrals_batch";
    SpPrims bs;
    SpAos ao;
    int nprim = 0, N = 0;
    if (int rc = spgto_describe(who, natm, nshell, count, shell_atom, shell_l, shell_prim_offset, exponents, coefficients, bs,
                                ao, nprim, N))
        return rc;
    EVC_REQUIRE((flags & ~kSpFlags) == 0, "%s: flags=%d, accepted EVC_FLAG_ENERGY_ONLY, EVC_FLAG_ERI_S4 and "
                "EVC_FLAG_IP1_S2KL", who, flags);
    const bool grad = !(flags & EVC_FLAG_ENERGY_ONLY);
    const int s4 = (flags & EVC_FLAG_ERI_S4) != 0, s2kl = (flags & EVC_FLAG_IP1_S2KL) != 0;
    EVC_REQUIRE(coords && charges && out && ws, "%s: null pointer", who);
    EVC_REQUIRE(out->enuc && out->S && out->hcore && out->eri, "%s: null pointer among enuc, S, hcore, eri", who);
    EVC_REQUIRE(!grad || (out->ipovlp && out->dhcore && out->eri_ip1 && out->gnuc), "%s: null pointer among ipovlp, dhcore, "
                "eri_ip1, gnuc (allowed only with EVC_FLAG_ENERGY_ONLY)", who);
    EVC_REQUIRE(aligned16(ws), "%s: workspace not 16-byte aligned", who);
    const size_t need = spgto_table_bytes(nprim, count);
    EVC_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, %zu needed for %d primitives, %d geometries", who, ws_bytes,
                need, nprim, count);
    hipStream_t st = as_stream(stream);
    const int Ms = N * (N + 1) / 2;
    double *tab = static_cast<double *>(ws);
    spgto_launch(spgto_pair_kernel, dim3((unsigned)ceil_div((int64_t)nprim * nprim, 256), (unsigned)count), dim3(256), st, bs,
                 coords, natm, nprim, tab);
    EVC_LAUNCH_CHECK("spgto_pair_kernel");
    const dim3 grid1((unsigned)ceil_div(Ms, 64), (unsigned)count),
        grid2((unsigned)ceil_div(Ms, 64), (unsigned)(grad ? N * N : Ms), (unsigned)count);
    if (grad) {
        spgto_launch(spgto_one_kernel<true>, grid1, dim3(64), st, ao, (const double *)tab, coords, charges, N, natm, nprim,
                     out->S, out->hcore, out->ipovlp, out->dhcore);
        EVC_LAUNCH_CHECK("spgto_one_kernel");
        spgto_launch(spgto_nuc_kernel<true>, dim3((unsigned)count), dim3(64), st, coords, charges, natm, out->enuc, out->gnuc);
        EVC_LAUNCH_CHECK("spgto_nuc_kernel");
        spgto_launch(spgto_two_kernel<true>, grid2, dim3(64), st, ao, (const double *)tab, N, nprim, s4, s2kl, out->eri,
                     out->eri_ip1);
    } else {
        spgto_launch(spgto_one_kernel<false>, grid1, dim3(64), st, ao, (const double *)tab, coords, charges, N, natm, nprim,
                     out->S, out->hcore, (double *)nullptr, (double *)nullptr);
        EVC_LAUNCH_CHECK("spgto_one_kernel");
        spgto_launch(spgto_nuc_kernel<false>, dim3((unsigned)count), dim3(64), st, coords, charges, natm, out->enuc,
                     (double *)nullptr);
        EVC_LAUNCH_CHECK("spgto_nuc_kernel");
        spgto_launch(spgto_two_kernel<false>, grid2, dim3(64), st, ao, (const double *)tab, N, nprim, s4, 0, out->eri,
                     (double *)nullptr);
    }
    EVC_LAUNCH_CHECK("spgto_two_kernel");
    return 0;
}

extern "C" int evc_spgto_dipole_batch(int natm, int nshell, int count, const double *coords, const int *shell_atom,
                                      const int *shell_l, const int *shell_prim_offset, const double *exponents,
                                      const double *coefficients, const double origin[3], double *dip, void *stream) {
    const char *who = "evc_spgto_dipole_batch";
    SpPrims bs;
    SpAos ao;
    int nprim = 0, N = 0;
    if (int rc = spgto_describe(who, natm, nshell, count, shell_atom, shell_l, shell_prim_offset, exponents, coefficients, bs,
                                ao, nprim, N))
        return rc;
    EVC_REQUIRE(coords && origin && dip, "%s: null pointer", who);
    spgto_launch(spgto_dipole_kernel, dim3((unsigned)ceil_div(N * (N + 1) / 2, 64), (unsigned)count), dim3(64), as_stream(stream),
                 bs, ao, coords, N, natm, origin[0], origin[1], origin[2], dip);
    EVC_LAUNCH_CHECK("spgto_dipole_kernel");
    return 0;
}
