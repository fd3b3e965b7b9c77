// What the from-coordinates AO-integral routes of contracted Gaussian shells share: spgto.hip (s and p shells) and
// spdgto.hip (s, p and real spherical d shells) take all of it, sgto.hip the launch helper and the accepted flags.
//   limits and the primitive table (GtoPrims), the Boys functions, the power-raising step, the convolutions of the factored
//   Hermite Coulomb integrals, the pair-table body (the routes' pair kernels are wrappers of it), and the host side: every
//   refusal, the basis as the kernels take it, and the three calls of a route.
// A route is a struct (SpRoute, SpdRoute) with
//   Prims, Aos       the by-value kernel arguments: Prims a struct of its own name derived from GtoPrims (the name is part
//                    of the kernel symbols), Aos with off / np / atom per function and the route's own tag;
//   kMaxL, kLs       the highest l and the wording of its refusal;
//   tag(ao, f, l, c) sets the tag of function f, component c of a shell of l; padding gets the tag of an s function;
//   kPair, kOne, kOneE, kNuc, kNucE, kTwo, kTwoE, kDipole   the kernels (E: EVC_FLAG_ENERGY_ONLY), kName their prefix.
// The device maths that depends on the powers a route reaches (bra_dim, ket_dim, fold, poly, st_dim, the one / two / dipole
// bodies) stays in the route's file; the scheme is described in spgto.hip.  The nuclear-repulsion kernel stays written out
// in both files: called as a shared body, the compiler lays out its energy-only instantiation in another block order.
#pragma once
#include <math.h>
#include <stdint.h>

#include "common.hpp"

namespace evc {

constexpr int kGtoMaxAtoms = 64;        // centres
constexpr int kGtoMaxAo = 64;           // contracted functions
constexpr int kGtoMaxShells = 64;
constexpr int kGtoMaxShellPrim = 8;     // primitives of one shell
constexpr int kGtoMaxPrim = 128;        // primitives of all shells
constexpr int kGtoMaxCount = 65535;     // geometries per call (gridDim.z)
constexpr int kGtoRow = 14;             // doubles of a row of the pair table
constexpr int kGtoFlags = EVC_FLAG_ENERGY_ONLY | EVC_FLAG_ERI_S4 | EVC_FLAG_IP1_S2KL;
constexpr double kGtoBoysCrossover = 12.0;
constexpr double kGtoPi = 3.141592653589793;

struct GtoPrims {
    double ex[kGtoMaxPrim];      // exponents
    double cn[kGtoMaxPrim];      // coefficient x norm of the primitive
    uint8_t atom[kGtoMaxPrim];   // its centre
};

// Every launch of the three files: the runtime call, not the chevrons (tests/test_s*gto_closure.py).
template <typename T>
struct gto_same_type {
    using type = T;
};
template <typename... P>
static void gto_launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t st,
                       typename gto_same_type<P>::type... a) {
    void *args[] = {(void *)&a...};
    // the result is read by the EVC_LAUNCH_CHECK (hipGetLastError) that follows the call
    (void)hipLaunchKernel(reinterpret_cast<const void *>(kernel), grid, block, args, 0, st);
}

#define GTO_HD __host__ __device__ __forceinline__

// row of the packed index m = row (row + 1) / 2 + col, col <= row
GTO_HD int gto_tri_row(int m) {
    int r = (int)((sqrt(8.0 * m + 1.0) - 1.0) * 0.5);
    if (r * (r + 1) / 2 > m) --r;
    if ((r + 1) * (r + 2) / 2 <= m) ++r;
    return r;
}

// ---- monomials of a function of s, p and real spherical d shells (spdgto.hip, field.hip) -----------------------
// kind: 0: s; 1, 2, 3: p_x, p_y, p_z; 4 ... 8: d_xy, d_yz, d_z2, d_xz, d_x2-y2
GTO_HD int spd_nmono(int kind) { return kind == 6 ? 3 : (kind == 8 ? 2 : 1); }

// Powers (i0, i1, i2) of x, y, z and weight of monomial k of a function of `kind`, for primitives normalised as
// x y exp(-a r^2): 2 z^2 - x^2 - y^2 carries 1 / sqrt(12), x^2 - y^2 carries 1 / 2.
GTO_HD void spd_mono(int kind, int k, int &i0, int &i1, int &i2, double &w) {
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

GTO_HD double spd_sel3(int i, double v0, double v1, double v2) { return i == 0 ? v0 : (i == 1 ? v1 : v2); }

// ---- Boys functions ------------------------------------------------------------------------
// Eight more terms of the series of F_L from term K0 on, and eight more while they still count.
template <int L, int K0>
GTO_HD void gto_series(double t2, double &term, double &s) {
#pragma unroll
    for (int k = K0; k < K0 + 8; ++k) {
        term = term * (t2 * (1.0 / (2 * L + 2 * k + 1)));
        s = s + term;
    }
    if constexpr (K0 + 8 < 64) {
        if (!(term < s * 1e-17)) gto_series<L, K0 + 8>(t2, term, s);
    }
}

// F_0 ... F_L of t in f[0 .. L].
template <int L>
GTO_HD void gto_boys(double t, double (&f)[L + 1]) {
    if (t < kGtoBoysCrossover) {
        // F_L(t) = e^-t sum_k (2t)^k / ((2L + 1)(2L + 3) ... (2L + 2k + 1)): all terms positive, at most 65 of them
        const double t2 = 2.0 * t, et = exp(-t);
        double term = 1.0 / (2 * L + 1), s = term;
        gto_series<L, 1>(t2, term, s);
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
GTO_HD void gto_raise(const double (&e)[T], double X, double ip, double (&o)[T]) {
#pragma unroll
    for (int t = 0; t < T; ++t)
        o[t] = (t > 0 ? ip * e[t - 1] : 0.0) + X * e[t] + (t + 1 < T ? (t + 1) * e[t + 1] : 0.0);
}

// W[m] = sum_{j + k = m} U[j] V[k], m <= M.
template <int M>
GTO_HD void gto_conv(const double (&U)[M + 1], const double (&V)[M + 1], double (&W)[M + 1]) {
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
GTO_HD double gto_dot(const double (&H)[M + 1], const double (&U)[M + 1], const double (&V)[M + 1]) {
    double W[M + 1], s = 0.0;
    gto_conv<M>(U, V, W);
#pragma unroll
    for (int m = 0; m <= M; ++m) s = fma(H[m], W[m], s);
    return s;
}

// Overlap s, kinetic energy t and their derivatives for the centre of the first function of one primitive pair (without
// the pair's weight): d[x] of three dimensions, each the out[] of the route's st_dim.
GTO_HD void gto_overlap_kinetic(const double (&d)[3][4], double &s, double &t, double (&ds)[3], double (&dt)[3]) {
    s = d[0][0] * d[1][0] * d[2][0];
    t = d[0][1] * d[1][0] * d[2][0] + d[0][0] * d[1][1] * d[2][0] + d[0][0] * d[1][0] * d[2][1];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const int y = (x + 1) % 3, z = (x + 2) % 3;
        ds[x] = d[x][2] * d[y][0] * d[z][0];
        dt[x] = d[x][3] * d[y][0] * d[z][0] + d[x][2] * (d[y][1] * d[z][0] + d[y][0] * d[z][1]);
    }
}

// ---- pair table ------------------------------------------------------------------------
// idx = pa nprim + pb of geometry g; the row: p, P, Kab cn_a cn_b, a, b, 1/2p, P - A, P - B
GTO_HD void gto_pair_body(int idx, int g, const GtoPrims &bs, const double *coords, int natm, int nprim, double *tab) {
    if (idx >= nprim * nprim) return;
    const int pa = idx / nprim, pb = idx - pa * nprim;
    const double a = bs.ex[pa], b = bs.ex[pb];
    const double *Ra = coords + ((int64_t)g * natm + bs.atom[pa]) * 3, *Rb = coords + ((int64_t)g * natm + bs.atom[pb]) * 3;
    const double p = a + b, mu = a * b / p;
    double *row = tab + ((int64_t)g * nprim * nprim + idx) * kGtoRow;
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

// ---- host side ---------------------------------------------------------------------------------
// shell_ao: the most functions of one shell, 2 kMaxL + 1
static int gto_shape(const char *who, int shell_ao, int natm, int nshell, int nprim, int nao, int count) {
    EVC_REQUIRE(natm >= 1 && natm <= kGtoMaxAtoms, "%s: natm=%d, supported 1 ... %d", who, natm, kGtoMaxAtoms);
    EVC_REQUIRE(nshell >= 1 && nshell <= kGtoMaxShells, "%s: nshell=%d, supported 1 ... %d", who, nshell, kGtoMaxShells);
    EVC_REQUIRE(nprim >= nshell && nprim <= kGtoMaxPrim, "%s: nprim_total=%d, supported nshell ... %d", who, nprim,
                kGtoMaxPrim);
    EVC_REQUIRE(nao >= nshell && nao <= kGtoMaxAo && nao <= shell_ao * nshell, "%s: nao=%d, supported nshell ... %d", who,
                nao, kGtoMaxAo);
    EVC_REQUIRE(count >= 1 && count <= kGtoMaxCount, "%s: count=%d, supported 1 ... %d", who, count, kGtoMaxCount);
    return 0;
}

static size_t gto_table_bytes(int nprim, int count) {
    return align_up((size_t)count * nprim * nprim * kGtoRow * sizeof(double), 256);
}

// The basis as the kernels of route R take it; every refusal that concerns it.
template <class R>
static int gto_describe(const char *who, int natm, int nshell, int count, const int *shell_atom, const int *shell_l,
                        const int *shell_prim_offset, const double *exponents, const double *coefficients,
                        typename R::Prims &bs, typename R::Aos &ao, int &nprim, int &nao) {
    EVC_REQUIRE(natm >= 1 && natm <= kGtoMaxAtoms, "%s: natm=%d, supported 1 ... %d", who, natm, kGtoMaxAtoms);
    EVC_REQUIRE(nshell >= 1 && nshell <= kGtoMaxShells, "%s: nshell=%d, supported 1 ... %d", who, nshell, kGtoMaxShells);
    EVC_REQUIRE(shell_atom && shell_l && shell_prim_offset && exponents && coefficients, "%s: null pointer", who);
    EVC_REQUIRE(shell_prim_offset[0] == 0, "%s: shell_prim_offset[0]=%d, must be 0", who, shell_prim_offset[0]);
    nao = 0;
    for (int s = 0; s < nshell; ++s) {
        const int l = shell_l[s], k = shell_prim_offset[s + 1] - shell_prim_offset[s];
        EVC_REQUIRE(l >= 0 && l <= R::kMaxL, "%s: shell %d has l=%d, supported %s", who, s, l, R::kLs);
        EVC_REQUIRE(k >= 1 && k <= kGtoMaxShellPrim, "%s: shell %d has %d primitives, supported 1 ... %d", who, s, k,
                    kGtoMaxShellPrim);
        EVC_REQUIRE(shell_prim_offset[s + 1] <= kGtoMaxPrim, "%s: more than %d primitives in all", who, kGtoMaxPrim);
        EVC_REQUIRE(shell_atom[s] >= 0 && shell_atom[s] < natm, "%s: shell_atom[%d]=%d outside 0 ... natm-1", who, s,
                    shell_atom[s]);
        EVC_REQUIRE(s == 0 || shell_atom[s] >= shell_atom[s - 1], "%s: shell_atom must be ascending (shell %d)", who, s);
        nao += 2 * l + 1;
    }
    nprim = shell_prim_offset[nshell];
    if (int rc = gto_shape(who, 2 * R::kMaxL + 1, natm, nshell, nprim, nao, count)) return rc;
    int f = 0;
    for (int s = 0; s < nshell; ++s) {
        const int l = shell_l[s];
        for (int k = shell_prim_offset[s]; k < shell_prim_offset[s + 1]; ++k) {
            const double a = exponents[k];
            EVC_REQUIRE(a > 0.0 && isfinite(a), "%s: exponent %d is %g, must be positive", who, k, a);
            // the norm of exp(-a r^2), x exp(-a r^2), x y exp(-a r^2), x y z exp(-a r^2)
            const double norm = pow(2.0 * a / kGtoPi, 0.75) *
                                (l == 3 ? 8.0 * a * sqrt(a) : (l == 0 ? 1.0 : (l == 1 ? 2.0 * sqrt(a) : 4.0 * a)));
            bs.ex[k] = a;
            bs.cn[k] = coefficients[k] * norm;
            bs.atom[k] = (uint8_t)shell_atom[s];
        }
        for (int c = 0; c < 2 * l + 1; ++c, ++f) {
            ao.off[f] = (uint8_t)shell_prim_offset[s];
            ao.np[f] = (uint8_t)(shell_prim_offset[s + 1] - shell_prim_offset[s]);
            R::tag(ao, f, l, c);
            ao.atom[f] = (uint8_t)shell_atom[s];
        }
    }
    for (int k = nprim; k < kGtoMaxPrim; ++k) {
        bs.ex[k] = 1.0;
        bs.cn[k] = 0.0;
        bs.atom[k] = 0;
    }
    for (; f < kGtoMaxAo; ++f) {
        ao.off[f] = 0;
        ao.np[f] = 0;
        R::tag(ao, f, 0, 0);
        ao.atom[f] = 0;
    }
    return 0;
}

// ---- the three calls of a route ------------------------------------------------------------------
// EVC_LAUNCH_CHECK of the kernel <route>_<stem>_kernel
static int gto_launch_check(const char *route, const char *stem) {
    char name[32];
    snprintf(name, sizeof name, "%s_%s_kernel", route, stem);
    EVC_LAUNCH_CHECK(name);
    return 0;
}

template <class R>
static size_t gto_workspace_bytes(const char *who, int natm, int nshell, int nprim_total, int nao, int count) {
    if (gto_shape(who, 2 * R::kMaxL + 1, natm, nshell, nprim_total, nao, count)) return 0;
    return gto_table_bytes(nprim_total, count);
}

template <class R>
static int gto_integrals_batch(const char *who, int natm, int nshell, int count, const double *coords, const double *charges,
                               const int *shell_atom, const int *shell_l, const int *shell_prim_offset,
                               const double *exponents, const double *coefficients, const evc_sgto_outputs *out, int flags,
                               void *ws, size_t ws_bytes, void *stream) {
    typename R::Prims bs;
    typename R::Aos ao;
    int nprim = 0, N = 0;
    if (int rc = gto_describe<R>(who, natm, nshell, count, shell_atom, shell_l, shell_prim_offset, exponents, coefficients,
                                 bs, ao, nprim, N))
        return rc;
    EVC_REQUIRE((flags & ~kGtoFlags) == 0, "%s: flags=%d, accepted EVC_FLAG_ENERGY_ONLY, EVC_FLAG_ERI_S4 and "
                "EVC_FLAG_IP1_S2KL", who, flags);
    const bool grad = !(flags & EVC_FLAG_ENERGY_ONLY);
    const int s4 = (flags & EVC_FLAG_ERI_S4) != 0, s2kl = (flags & EVC_FLAG_IP1_S2KL) != 0;
    EVC_REQUIRE(coords && charges && out && ws, "%s: null pointer", who);
    EVC_REQUIRE(out->enuc && out->S && out->hcore && out->eri, "%s: null pointer among enuc, S, hcore, eri", who);
    EVC_REQUIRE(!grad || (out->ipovlp && out->dhcore && out->eri_ip1 && out->gnuc), "%s: null pointer among ipovlp, dhcore, "
                "eri_ip1, gnuc (allowed only with EVC_FLAG_ENERGY_ONLY)", who);
    EVC_REQUIRE(aligned16(ws), "%s: workspace not 16-byte aligned", who);
    const size_t need = gto_table_bytes(nprim, count);
    EVC_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, %zu needed for %d primitives, %d geometries", who, ws_bytes,
                need, nprim, count);
    hipStream_t st = as_stream(stream);
    const int Ms = N * (N + 1) / 2;
    double *tab = static_cast<double *>(ws);
    gto_launch(R::kPair, dim3((unsigned)ceil_div((int64_t)nprim * nprim, 256), (unsigned)count), dim3(256), st, bs, coords,
               natm, nprim, tab);
    if (int rc = gto_launch_check(R::kName, "pair")) return rc;
    const dim3 grid1((unsigned)ceil_div(Ms, 64), (unsigned)count),
        grid2((unsigned)ceil_div(Ms, 64), (unsigned)(grad ? N * N : Ms), (unsigned)count);
    // without the gradient: null pointers for its arrays, and eri_ip1 has no form
    gto_launch(grad ? R::kOne : R::kOneE, grid1, dim3(64), st, ao, (const double *)tab, coords, charges, N, natm, nprim,
               out->S, out->hcore, grad ? out->ipovlp : nullptr, grad ? out->dhcore : nullptr);
    if (int rc = gto_launch_check(R::kName, "one")) return rc;
    gto_launch(grad ? R::kNuc : R::kNucE, dim3((unsigned)count), dim3(64), st, coords, charges, natm, out->enuc,
               grad ? out->gnuc : nullptr);
    if (int rc = gto_launch_check(R::kName, "nuc")) return rc;
    gto_launch(grad ? R::kTwo : R::kTwoE, grid2, dim3(64), st, ao, (const double *)tab, N, nprim, s4, grad ? s2kl : 0,
               out->eri, grad ? out->eri_ip1 : nullptr);
    return gto_launch_check(R::kName, "two");
}

template <class R>
static int gto_dipole_batch(const char *who, int natm, int nshell, int count, const double *coords, const int *shell_atom,
                            const int *shell_l, const int *shell_prim_offset, const double *exponents,
                            const double *coefficients, const double origin[3], double *dip, void *stream) {
    typename R::Prims bs;
    typename R::Aos ao;
    int nprim = 0, N = 0;
    if (int rc = gto_describe<R>(who, natm, nshell, count, shell_atom, shell_l, shell_prim_offset, exponents, coefficients,
                                 bs, ao, nprim, N))
        return rc;
    EVC_REQUIRE(coords && origin && dip, "%s: null pointer", who);
    gto_launch(R::kDipole, dim3((unsigned)ceil_div(N * (N + 1) / 2, 64), (unsigned)count), dim3(64), as_stream(stream), bs,
               ao, coords, N, natm, origin[0], origin[1], origin[2], dip);
    return gto_launch_check(R::kName, "dipole");
}

}  // namespace evc
