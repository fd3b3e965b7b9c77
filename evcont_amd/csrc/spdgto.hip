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
// Boys functions (spd_boys): the scheme of sp_boys: below t = 12 the convergent series of the highest order, then downward
// recursion; above it F0 from erf and upward recursion.
//
// Kernels, each a launch of its own (FP64 VALU; DESIGN.md: FP64 MFMA blocks its SIMD's vector issue), the cut of spgto.hip:
//   spdgto_pair_kernel    the primitive-pair table (one row of kSpdRow doubles per ordered pair of primitive entries).
//   spdgto_one_kernel     one thread per contracted pair mu >= nu: S, hcore (mirrored), ipovlp, dhcore.
//   spdgto_nuc_kernel     nuclear repulsion and its gradient, one thread per centre.
//   spdgto_two_kernel     one thread per (mu nu | kappa >= lambda); primitive quartets in one fixed order (ket pair outer,
//                         bra pair inner), inside a quartet the monomials in one fixed order (ket outer, bra inner).
//                         No screening: every quartet is evaluated.
//   spdgto_dipole_kernel  <mu| r - origin |nu>, one thread per contracted pair mu >= nu, mirrored.
// No sum is split across threads and there are no read-modify-write operations between threads: the same bits from run to
// run and for every batch size, and the full forms are the unpacked packed forms.
// The basis is a HOST argument and reaches the kernels by value.
#include <math.h>
#include <stdint.h>

#include "common.hpp"

namespace evc {

constexpr int kSpdMaxAtoms = 64;        // centres
constexpr int kSpdMaxAo = 64;           // contracted functions
constexpr int kSpdMaxShells = 64;
constexpr int kSpdMaxShellPrim = 8;     // primitives of one shell
constexpr int kSpdMaxPrim = 128;        // primitives of all shells
constexpr int kSpdMaxCount = 65535;     // geometries per call (gridDim.z)
constexpr int kSpdRow = 14;             // doubles of a row of the pair table
constexpr int kSpdFlags = EVC_FLAG_ENERGY_ONLY | EVC_FLAG_ERI_S4 | EVC_FLAG_IP1_S2KL;
constexpr double kSpdBoysCrossover = 12.0;
constexpr double kSpdPi = 3.141592653589793;

struct SpdPrims {
    double ex[kSpdMaxPrim];      // exponents
    double cn[kSpdMaxPrim];      // coefficient x norm of the primitive
    uint8_t atom[kSpdMaxPrim];   // its centre
};
struct SpdAos {
    uint8_t off[kSpdMaxAo];      // first primitive of the function's shell
    uint8_t np[kSpdMaxAo];       // primitives of the shell
    uint8_t kind[kSpdMaxAo];     // 0: s; 1, 2, 3: p_x, p_y, p_z; 4 ... 8: d_xy, d_yz, d_z2, d_xz, d_x2-y2
    uint8_t atom[kSpdMaxAo];
};

// Every launch of this file: the runtime call, not the chevrons (tests/test_spdgto_closure.py).
template <typename T>
struct spdgto_same_type {
    using type = T;
};
template <typename... P>
static void spdgto_launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t st,
                          typename spdgto_same_type<P>::type... a) {
    void *args[] = {(void *)&a...};
    // the result is read by the EVC_LAUNCH_CHECK (hipGetLastError) that follows the call
    (void)hipLaunchKernel(reinterpret_cast<const void *>(kernel), grid, block, args, 0, st);
}

#define SPD_HD __host__ __device__ __forceinline__

// row of the packed index m = row (row + 1) / 2 + col, col <= row
SPD_HD int spd_tri_row(int m) {
    int r = (int)((sqrt(8.0 * m + 1.0) - 1.0) * 0.5);
    if (r * (r + 1) / 2 > m) --r;
    if ((r + 1) * (r + 2) / 2 <= m) ++r;
    return r;
}

// ---- monomials of a function ---------------------------------------------------------------
SPD_HD int spd_nmono(int kind) { return kind == 6 ? 3 : (kind == 8 ? 2 : 1); }

// Powers (i0, i1, i2) of x, y, z and weight of monomial k of a function of `kind`, for primitives normalised as
// x y exp(-a r^2): 2 z^2 - x^2 - y^2 carries 1 / sqrt(12), x^2 - y^2 carries 1 / 2.
SPD_HD void spd_mono(int kind, int k, int &i0, int &i1, int &i2, double &w) {
    // 6 bits per kind: power of x | power of y << 2 | power of z << 4, of the first monomial
    constexpr uint64_t first = (1ull << 6) | (4ull << 12) | (16ull << 18) | (5ull << 24) | (20ull << 30) | (32ull << 36) |
                               (17ull << 42) | (2ull << 48);
    int code = (int)(first >> (6 * kind)) & 63;
    w = 1.0;
    if (kind == 6) {
        code = k == 0 ? 32 : (k == 1 ? 2 : 8);
        w = k == 0 ? 0.57735026918962576 : -0.28867513459481288;
    }
    if (kind == 8) {
        code = k == 0 ? 2 : 8;
        w = k == 0 ? 0.5 : -0.5;
    }
    i0 = code & 3;
    i1 = (code >> 2) & 3;
    i2 = (code >> 4) & 3;
}

SPD_HD double spd_sel3(int i, double v0, double v1, double v2) { return i == 0 ? v0 : (i == 1 ? v1 : v2); }

// ---- Boys functions ------------------------------------------------------------------------
// Eight more terms of the series of F_L from term K0 on, and eight more while they still count.
template <int L, int K0>
SPD_HD void spd_series(double t2, double &term, double &s) {
#pragma unroll
    for (int k = K0; k < K0 + 8; ++k) {
        term = term * (t2 * (1.0 / (2 * L + 2 * k + 1)));
        s = s + term;
    }
    if constexpr (K0 + 8 < 64) {
        if (!(term < s * 1e-17)) spd_series<L, K0 + 8>(t2, term, s);
    }
}

// F_0 ... F_L of t in f[0 .. L].
template <int L>
SPD_HD void spd_boys(double t, double (&f)[L + 1]) {
    if (t < kSpdBoysCrossover) {
        const double t2 = 2.0 * t, et = exp(-t);
        double term = 1.0 / (2 * L + 1), s = term;
        spd_series<L, 1>(t2, term, s);
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

// ---- Hermite coefficients of one dimension ---------------------------------------------------
// One more power on a function whose centre is X away from P: o[t] = e[t-1] / 2p + X e[t] + (t + 1) e[t+1].
template <int T>
SPD_HD void spd_raise(const double (&e)[T], double X, double ip, double (&o)[T]) {
#pragma unroll
    for (int t = 0; t < T; ++t)
        o[t] = (t > 0 ? ip * e[t - 1] : 0.0) + X * e[t] + (t + 1 < T ? (t + 1) * e[t + 1] : 0.0);
}

// Hermite coefficients (t <= 5) of one dimension of a primitive pair with the powers i, j (0 ... 2), without the
// exponential: `base` = E^{ij}, `der` = those of d/dA, 2a E^{i+1,j} - i E^{i-1,j}.  XA = P - A, XB = P - B, ip = 1 / 2p.
// All raising steps run; the rows are picked by selects.
SPD_HD void spd_bra_dim(int i, int j, double a, double XA, double XB, double ip, double (&base)[6], double (&der)[6]) {
    const double e0[6] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double b1[6], b2[6], ej[6], a1[6], a2[6], a3[6];
    spd_raise(e0, XB, ip, b1);
    spd_raise(b1, XB, ip, b2);
#pragma unroll
    for (int t = 0; t < 6; ++t) ej[t] = spd_sel3(j, e0[t], b1[t], b2[t]);
    spd_raise(ej, XA, ip, a1);
    spd_raise(a1, XA, ip, a2);
    spd_raise(a2, XA, ip, a3);
    const double ax2 = 2.0 * a, di = (double)i;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        base[t] = spd_sel3(i, ej[t], a1[t], a2[t]);
        der[t] = ax2 * spd_sel3(i, a1[t], a2[t], a3[t]) - di * spd_sel3(i, 0.0, ej[t], a1[t]);
    }
}

// (-1)^tau E^{kl}_tau (tau <= 4) of one dimension of the ket pair, powers k, l (0 ... 2).
SPD_HD void spd_ket_dim(int k, int l, double XC, double XD, double ip, double (&o)[5]) {
    const double e0[5] = {1.0, 0.0, 0.0, 0.0, 0.0};
    double d1[5], d2[5], el[5], c1[5], c2[5];
    spd_raise(e0, XD, ip, d1);
    spd_raise(d1, XD, ip, d2);
#pragma unroll
    for (int t = 0; t < 5; ++t) el[t] = spd_sel3(l, e0[t], d1[t], d2[t]);
    spd_raise(el, XC, ip, c1);
    spd_raise(c1, XC, ip, c2);
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const double v = spd_sel3(k, el[t], c1[t], c2[t]);
        o[t] = (t & 1) ? -v : v;
    }
}

// c[n] = sum_{t + tau = n} b[t] k[tau], n <= M.
template <int M>
SPD_HD void spd_fold(const double (&b)[6], const double (&k)[5], double (&c)[M + 1]) {
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
SPD_HD void spd_take(const double (&b)[6], double (&c)[M + 1]) {
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
SPD_HD void spd_poly(const double (&c)[M + 1], double X, double (&A)[M + 1]) {
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

// W[m] = sum_{j + k = m} U[j] V[k], m <= M.
template <int M>
SPD_HD void spd_conv(const double (&U)[M + 1], const double (&V)[M + 1], double (&W)[M + 1]) {
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
SPD_HD double spd_dot(const double (&H)[M + 1], const double (&U)[M + 1], const double (&V)[M + 1]) {
    double W[M + 1], s = 0.0;
    spd_conv<M>(U, V, W);
#pragma unroll
    for (int m = 0; m <= M; ++m) s = fma(H[m], W[m], s);
    return s;
}

// ---- pair table ------------------------------------------------------------------------
// idx = pa nprim + pb of geometry g: p, P, Kab cn_a cn_b, a, b, 1/2p, P - A, P - B
SPD_HD void spd_pair_body(int idx, int g, const SpdPrims &bs, const double *coords, int natm, int nprim, double *tab) {
    if (idx >= nprim * nprim) return;
    const int pa = idx / nprim, pb = idx - pa * nprim;
    const double a = bs.ex[pa], b = bs.ex[pb];
    const double *Ra = coords + ((int64_t)g * natm + bs.atom[pa]) * 3, *Rb = coords + ((int64_t)g * natm + bs.atom[pb]) * 3;
    const double p = a + b, mu = a * b / p;
    double *row = tab + ((int64_t)g * nprim * nprim + idx) * kSpdRow;
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

__global__ __launch_bounds__(256) void spdgto_pair_kernel(SpdPrims bs, const double *__restrict__ coords, int natm, int nprim,
                                                           double *__restrict__ tab) {
    spd_pair_body(blockIdx.x * 256 + threadIdx.x, blockIdx.y, bs, coords, natm, nprim, tab);
}

// ---- two-electron integrals ----------------------------------------------------------------
// M: the highest Hermite order, 9 with the gradient and 8 without.
template <bool GRAD>
SPD_HD void spd_two_body(int mu, int nu, int v, int g, const SpdAos &ao, const double *tab, int N, int nprim, int s4,
                         int s2kl, double *eri, double *ip1) {
    constexpr int M = GRAD ? 9 : 8;
    const int Ms = N * (N + 1) / 2;
    if (v >= Ms) return;
    const int kap = spd_tri_row(v), lam = v - kap * (kap + 1) / 2;
    const double *tg = tab + (int64_t)g * nprim * nprim * kSpdRow;
    const int km = ao.kind[mu], kn = ao.kind[nu], kk = ao.kind[kap], kl = ao.kind[lam];
    const int nm = spd_nmono(km), nn = spd_nmono(kn), nk = spd_nmono(kk), nl = spd_nmono(kl);
    double acc = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    for (int pc = ao.off[kap]; pc < ao.off[kap] + ao.np[kap]; ++pc)
        for (int pd = ao.off[lam]; pd < ao.off[lam] + ao.np[lam]; ++pd) {
            const double *kr = tg + ((int64_t)pc * nprim + pd) * kSpdRow;
            const double q = kr[0], qx = kr[1], qy = kr[2], qz = kr[3], ck = kr[4];
            for (int pa = ao.off[mu]; pa < ao.off[mu] + ao.np[mu]; ++pa)
                for (int pb = ao.off[nu]; pb < ao.off[nu] + ao.np[nu]; ++pb) {
                    const double *br = tg + ((int64_t)pa * nprim + pb) * kSpdRow;
                    const double p = br[0], X[3] = {br[1] - qx, br[2] - qy, br[3] - qz};
                    const double s = p + q, pq = p * q;
                    const double alpha = pq / s;
                    double H[M + 1];
                    spd_boys<M>(alpha * (X[0] * X[0] + X[1] * X[1] + X[2] * X[2]), H);
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
                                    spd_conv<M>(A[1], A[2], yz);
                                    acc = acc + wt * spd_dot<M>(H, A[0], yz);
                                    if (GRAD) {
                                        // electron gradient = - centre gradient; one direction at a time
                                        double c[M + 1], D[M + 1], oth[M + 1];
                                        spd_fold<M>(der[0], ek[0], c);
                                        spd_poly<M>(c, X[0], D);
                                        gx = gx - wt * spd_dot<M>(H, D, yz);
                                        spd_fold<M>(der[1], ek[1], c);
                                        spd_poly<M>(c, X[1], D);
                                        spd_conv<M>(A[0], A[2], oth);
                                        gy = gy - wt * spd_dot<M>(H, D, oth);
                                        spd_fold<M>(der[2], ek[2], c);
                                        spd_poly<M>(c, X[2], D);
                                        spd_conv<M>(A[0], A[1], oth);
                                        gz = gz - wt * spd_dot<M>(H, D, oth);
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
        mu = spd_tri_row(by);
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
SPD_HD void spd_os_table(double XA, double XB, double ip, double (&s)[4][5]) {
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

SPD_HD void spd_st_dim(int i, int j, double a, double b, double XA, double XB, double ip, double (&out)[4]) {
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

// Overlap s, kinetic energy t and their derivatives for the centre of the first function of one primitive pair (without
// the pair's weight): d[x] of three dimensions.
SPD_HD void spd_overlap_kinetic(const double (&d)[3][4], double &s, double &t, double (&ds)[3], double (&dt)[3]) {
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
SPD_HD void spd_one_body(int e, int g, const SpdAos &ao, const double *tab, const double *coords, const double *charges,
                         int N, int natm, int nprim, double *S, double *hcore, double *ipovlp, double *dhcore) {
    constexpr int M = GRAD ? 5 : 4;
    if (e >= N * (N + 1) / 2) return;
    const int mu = spd_tri_row(e), nu = e - mu * (mu + 1) / 2;
    const int km = ao.kind[mu], kn = ao.kind[nu], am = ao.atom[mu], an = ao.atom[nu];
    const int nm = spd_nmono(km), nn = spd_nmono(kn);
    const double *Rg = coords + (int64_t)g * natm * 3;
    const double *tg = tab + (int64_t)g * nprim * nprim * kSpdRow;
    const int64_t n2 = (int64_t)N * N, ij = (int64_t)mu * N + nu, ji = (int64_t)nu * N + mu;
    // overlap and kinetic energy; dsa, dta: derivatives for the centre of mu; dsb, dtb: for the centre of nu
    double s = 0.0, tk = 0.0, dsa[3] = {0.0, 0.0, 0.0}, dta[3] = {0.0, 0.0, 0.0}, dsb[3] = {0.0, 0.0, 0.0},
           dtb[3] = {0.0, 0.0, 0.0};
    for (int pa = ao.off[mu]; pa < ao.off[mu] + ao.np[mu]; ++pa)
        for (int pb = ao.off[nu]; pb < ao.off[nu] + ao.np[nu]; ++pb) {
            const double *r = tg + ((int64_t)pa * nprim + pb) * kSpdRow;
            const double pip = kSpdPi / r[0], w0 = pip * sqrt(pip) * r[4];
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
                    spd_overlap_kinetic(d, sp, tp, ds, dt);
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
                        spd_overlap_kinetic(d, sp, tp, ds, dt);
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
                const double *r = tg + ((int64_t)pa * nprim + pb) * kSpdRow;
                const double p = r[0], X[3] = {r[1] - C[0], r[2] - C[1], r[3] - C[2]};
                double H[M + 1];
                spd_boys<M>(p * (X[0] * X[0] + X[1] * X[1] + X[2] * X[2]), H);
                double w = -z * (2.0 * kSpdPi / p) * r[4];
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
                        spd_conv<M>(A[1], A[2], yz);
                        vn = vn + wt * spd_dot<M>(H, A[0], yz);
                        if (GRAD) {
                            double xz[M + 1], xy[M + 1];
                            spd_conv<M>(A[0], A[2], xz);
                            spd_conv<M>(A[0], A[1], xy);
                            dva[0] = dva[0] + wt * spd_dot<M>(H, Da[0], yz);
                            dva[1] = dva[1] + wt * spd_dot<M>(H, Da[1], xz);
                            dva[2] = dva[2] + wt * spd_dot<M>(H, Da[2], xy);
                            dvb[0] = dvb[0] + wt * spd_dot<M>(H, Db[0], yz);
                            dvb[1] = dvb[1] + wt * spd_dot<M>(H, Db[1], xz);
                            dvb[2] = dvb[2] + wt * spd_dot<M>(H, Db[2], xy);
                            op[0] = op[0] + wt * spd_dot<M>(H, Op[0], yz);
                            op[1] = op[1] + wt * spd_dot<M>(H, Op[1], xz);
                            op[2] = op[2] + wt * spd_dot<M>(H, Op[2], xy);
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
SPD_HD void spd_dipole_body(int e, int g, const SpdPrims &bs, const SpdAos &ao, const double *coords, int N, int natm,
                            double ox, double oy, double oz, double *dip) {
    if (e >= N * (N + 1) / 2) return;
    const int mu = spd_tri_row(e), nu = e - mu * (mu + 1) / 2;
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
            const double pip = kSpdPi / p, w0 = pip * sqrt(pip) * exp(-mup * r2) * bs.cn[pa] * bs.cn[pb];
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

// ---- host side ---------------------------------------------------------------------------------
static int spdgto_shape(const char *who, int natm, int nshell, int nprim, int nao, int count) {
    EVC_REQUIRE(natm >= 1 && natm <= kSpdMaxAtoms, "%s: natm=%d, supported 1 ... %d", who, natm, kSpdMaxAtoms);
    EVC_REQUIRE(nshell >= 1 && nshell <= kSpdMaxShells, "%s: nshell=%d, supported 1 ... %d", who, nshell, kSpdMaxShells);
    EVC_REQUIRE(nprim >= nshell && nprim <= kSpdMaxPrim, "%s: nprim_total=%d, supported nshell ... %d", who, nprim,
                kSpdMaxPrim);
    EVC_REQUIRE(nao >= nshell && nao <= kSpdMaxAo && nao <= 5 * nshell, "%s: nao=%d, supported nshell ... %d", who, nao,
                kSpdMaxAo);
    EVC_REQUIRE(count >= 1 && count <= kSpdMaxCount, "%s: count=%d, supported 1 ... %d", who, count, kSpdMaxCount);
    return 0;
}

static size_t spdgto_table_bytes(int nprim, int count) {
    return align_up((size_t)count * nprim * nprim * kSpdRow * sizeof(double), 256);
}

// The basis as the kernels take it; every refusal that concerns it.
static int spdgto_describe(const char *who, int natm, int nshell, int count, const int *shell_atom, const int *shell_l,
                           const int *shell_prim_offset, const double *exponents, const double *coefficients, SpdPrims &bs,
                           SpdAos &ao, int &nprim, int &nao) {
    EVC_REQUIRE(natm >= 1 && natm <= kSpdMaxAtoms, "%s: natm=%d, supported 1 ... %d", who, natm, kSpdMaxAtoms);
    EVC_REQUIRE(nshell >= 1 && nshell <= kSpdMaxShells, "%s: nshell=%d, supported 1 ... %d", who, nshell, kSpdMaxShells);
    EVC_REQUIRE(shell_atom && shell_l && shell_prim_offset && exponents && coefficients, "%s: null pointer", who);
    EVC_REQUIRE(shell_prim_offset[0] == 0, "%s: shell_prim_offset[0]=%d, must be 0", who, shell_prim_offset[0]);
    nao = 0;
    for (int s = 0; s < nshell; ++s) {
        const int l = shell_l[s], k = shell_prim_offset[s + 1] - shell_prim_offset[s];
        EVC_REQUIRE(l >= 0 && l <= 2, "%s: shell %d has l=%d, supported 0, 1 and 2", who, s, l);
        EVC_REQUIRE(k >= 1 && k <= kSpdMaxShellPrim, "%s: shell %d has %d primitives, supported 1 ... %d", who, s, k,
                    kSpdMaxShellPrim);
        EVC_REQUIRE(shell_prim_offset[s + 1] <= kSpdMaxPrim, "%s: more than %d primitives in all", who, kSpdMaxPrim);
        EVC_REQUIRE(shell_atom[s] >= 0 && shell_atom[s] < natm, "%s: shell_atom[%d]=%d outside 0 ... natm-1", who, s,
                    shell_atom[s]);
        EVC_REQUIRE(s == 0 || shell_atom[s] >= shell_atom[s - 1], "%s: shell_atom must be ascending (shell %d)", who, s);
        nao += 2 * l + 1;
    }
    nprim = shell_prim_offset[nshell];
    if (int rc = spdgto_shape(who, natm, nshell, nprim, nao, count)) return rc;
    int f = 0;
    for (int s = 0; s < nshell; ++s) {
        const int l = shell_l[s];
        for (int k = shell_prim_offset[s]; k < shell_prim_offset[s + 1]; ++k) {
            const double a = exponents[k];
            EVC_REQUIRE(a > 0.0 && isfinite(a), "%s: exponent %d is %g, must be positive", who, k, a);
            // the norm of exp(-a r^2), x exp(-a r^2), x y exp(-a r^2)
            const double norm = pow(2.0 * a / kSpdPi, 0.75) * (l == 0 ? 1.0 : (l == 1 ? 2.0 * sqrt(a) : 4.0 * a));
            bs.ex[k] = a;
            bs.cn[k] = coefficients[k] * norm;
            bs.atom[k] = (uint8_t)shell_atom[s];
        }
        for (int c = 0; c < 2 * l + 1; ++c, ++f) {
            ao.off[f] = (uint8_t)shell_prim_offset[s];
            ao.np[f] = (uint8_t)(shell_prim_offset[s + 1] - shell_prim_offset[s]);
            ao.kind[f] = (uint8_t)(l == 0 ? 0 : (l == 1 ? 1 + c : 4 + c));
            ao.atom[f] = (uint8_t)shell_atom[s];
        }
    }
    for (int k = nprim; k < kSpdMaxPrim; ++k) {
        bs.ex[k] = 1.0;
        bs.cn[k] = 0.0;
        bs.atom[k] = 0;
    }
    for (; f < kSpdMaxAo; ++f) {
        ao.off[f] = 0;
        ao.np[f] = 0;
        ao.kind[f] = 0;
        ao.atom[f] = 0;
    }
    return 0;
}

}  // namespace evc

using namespace evc;

extern "C" size_t evc_spdgto_workspace_bytes(int natm, int nshell, int nprim_total, int nao, int count) {
    if (spdgto_shape("evc_spdgto_workspace_bytes", natm, nshell, nprim_total, nao, count)) return 0;
    return spdgto_table_bytes(nprim_total, count);
}

extern "C" int evc_spdgto_integrals_batch(int natm, int nshell, int count, const double *coords, const double *charges,
                                          const int *shell_atom, const int *shell_l, const int *shell_prim_offset,
                                          const double *exponents, const double *coefficients, const evc_sgto_outputs *out,
                                          int flags, void *ws, size_t ws_bytes, void *stream) {
    const char *who = "evc_spdgto_integrals_batch";
    SpdPrims bs;
    SpdAos ao;
    int nprim = 0, N = 0;
    if (int rc = spdgto_describe(who, natm, nshell, count, shell_atom, shell_l, shell_prim_offset, exponents, coefficients,
                                 bs, ao, nprim, N))
        return rc;
    EVC_REQUIRE((flags & ~kSpdFlags) == 0, "%s: flags=%d, accepted EVC_FLAG_ENERGY_ONLY, EVC_FLAG_ERI_S4 and "
                "EVC_FLAG_IP1_S2KL", who, flags);
    const bool grad = !(flags & EVC_FLAG_ENERGY_ONLY);
    const int s4 = (flags & EVC_FLAG_ERI_S4) != 0, s2kl = (flags & EVC_FLAG_IP1_S2KL) != 0;
    EVC_REQUIRE(coords && charges && out && ws, "%s: null pointer", who);
    EVC_REQUIRE(out->enuc && out->S && out->hcore && out->eri, "%s: null pointer among enuc, S, hcore, eri", who);
    EVC_REQUIRE(!grad || (out->ipovlp && out->dhcore && out->eri_ip1 && out->gnuc), "%s: null pointer among ipovlp, dhcore, "
                "eri_ip1, gnuc (allowed only with EVC_FLAG_ENERGY_ONLY)", who);
    EVC_REQUIRE(aligned16(ws), "%s: workspace not 16-byte aligned", who);
    const size_t need = spdgto_table_bytes(nprim, count);
    EVC_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, %zu needed for %d primitives, %d geometries", who, ws_bytes,
                need, nprim, count);
    hipStream_t st = as_stream(stream);
    const int Ms = N * (N + 1) / 2;
    double *tab = static_cast<double *>(ws);
    spdgto_launch(spdgto_pair_kernel, dim3((unsigned)ceil_div((int64_t)nprim * nprim, 256), (unsigned)count), dim3(256), st,
                  bs, coords, natm, nprim, tab);
    EVC_LAUNCH_CHECK("spdgto_pair_kernel");
    const dim3 grid1((unsigned)ceil_div(Ms, 64), (unsigned)count),
        grid2((unsigned)ceil_div(Ms, 64), (unsigned)(grad ? N * N : Ms), (unsigned)count);
    if (grad) {
        spdgto_launch(spdgto_one_kernel<true>, grid1, dim3(64), st, ao, (const double *)tab, coords, charges, N, natm, nprim,
                      out->S, out->hcore, out->ipovlp, out->dhcore);
        EVC_LAUNCH_CHECK("spdgto_one_kernel");
        spdgto_launch(spdgto_nuc_kernel<true>, dim3((unsigned)count), dim3(64), st, coords, charges, natm, out->enuc,
                      out->gnuc);
        EVC_LAUNCH_CHECK("spdgto_nuc_kernel");
        spdgto_launch(spdgto_two_kernel<true>, grid2, dim3(64), st, ao, (const double *)tab, N, nprim, s4, s2kl, out->eri,
                      out->eri_ip1);
    } else {
        spdgto_launch(spdgto_one_kernel<false>, grid1, dim3(64), st, ao, (const double *)tab, coords, charges, N, natm, nprim,
                      out->S, out->hcore, (double *)nullptr, (double *)nullptr);
        EVC_LAUNCH_CHECK("spdgto_one_kernel");
        spdgto_launch(spdgto_nuc_kernel<false>, dim3((unsigned)count), dim3(64), st, coords, charges, natm, out->enuc,
                      (double *)nullptr);
        EVC_LAUNCH_CHECK("spdgto_nuc_kernel");
        spdgto_launch(spdgto_two_kernel<false>, grid2, dim3(64), st, ao, (const double *)tab, N, nprim, s4, 0, out->eri,
                      (double *)nullptr);
    }
    EVC_LAUNCH_CHECK("spdgto_two_kernel");
    return 0;
}

extern "C" int evc_spdgto_dipole_batch(int natm, int nshell, int count, const double *coords, const int *shell_atom,
                                       const int *shell_l, const int *shell_prim_offset, const double *exponents,
                                       const double *coefficients, const double origin[3], double *dip, void *stream) {
    const char *who = "evc_spdgto_dipole_batch";
    SpdPrims bs;
    SpdAos ao;
    int nprim = 0, N = 0;
    if (int rc = spdgto_describe(who, natm, nshell, count, shell_atom, shell_l, shell_prim_offset, exponents, coefficients,
                                 bs, ao, nprim, N))
        return rc;
    EVC_REQUIRE(coords && origin && dip, "%s: null pointer", who);
    spdgto_launch(spdgto_dipole_kernel, dim3((unsigned)ceil_div(N * (N + 1) / 2, 64), (unsigned)count), dim3(64),
                  as_stream(stream), bs, ao, coords, N, natm, origin[0], origin[1], origin[2], dip);
    EVC_LAUNCH_CHECK("spdgto_dipole_kernel");
    return 0;
}
