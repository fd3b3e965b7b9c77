// A uniform electric field on the device (evc_sgto_dipole_grad_batch, evc_gto_dipole_grad_batch, evc_field_fold_batch):
// the device statement of evcont_amd/field.py.  H(F) = H0 - mu . F changes hcore, dhcore, enuc and gnuc of a geometry and
// nothing else of the chain; what was missing is the nuclear derivative of the dipole integrals, which comes from
//   ipdip[x,c,mu,nu] = <d_x mu| r_c - O_c |nu>      (electron-coordinate gradient on the bra, the convention of ipovlp)
//   d dip_c[mu,nu] / dR_Ax = - ipdip[x,c,mu,nu] [mu in A] - ipdip[x,c,nu,mu] [nu in A].
//
// Kernels, each a launch of its own through gto_launch of gto_shells.hpp (FP64 VALU; the work is O(N^2 nprim^2), one-electron):
//   field_sgrad_kernel   ipdip of one contracted s function per centre (the molecules of sgto.hip): one thread per ORDERED
//                        pair (i, j), closed form per primitive pair, delta_xc (a/p) S - 2 mu (A - B)_x (P_c - O_c) S, with
//                        the pair centre of prop_sdip_kernel (on coincident coordinates the centre exactly).  Its basis is
//                        the contraction alone (at most 8 primitives by value): H30 / STO-6G has 180 primitive entries, more
//                        than the shell table of the general kernel holds.
//   field_grad_kernel    ipdip of shells with l <= 2 (the molecules of spgto.hip and spdgto.hip): one thread per ORDERED
//                        contracted pair, primitive pairs and monomials (spd_mono) in one fixed ascending order.  Per
//                        dimension the overlap table s(i', j) of the Obara-Saika recursion up to i' = l + 2 = 4 (the centre
//                        derivative and the operator each raise the first power by one), the wanted entries picked by
//                        selects: every loop has fixed bounds and no register array is indexed at run time.
//   field_fold_kernel    one thread per element pair mu >= nu of a geometry: hcore and the two dhcore blocks of the atoms of
//                        mu and nu, read at (mu, nu) and written mirrored; thread 0 of a geometry also updates enuc and gnuc,
//                        the atoms in ascending order.
// No sum is split across threads and there are no read-modify-write operations between threads: the same bits from run to
// run and for every batch size.  Every refusal happens on the host, before a launch.
#include "gto_shells.hpp"

namespace evc {

constexpr int kFieldSMaxAtoms = 96;    // the limits of evc_sgto_dipole_batch
constexpr int kFieldSMaxPrim = 8;
constexpr int kFieldMaxCount = 65535;  // gridDim.y
constexpr int kFieldMaxN = 96;         // the evaluators' limit
constexpr int kFieldMaxAtoms = 65535;

struct FieldSBasis {
    double ex[kFieldSMaxPrim];   // exponents
    double cn[kFieldSMaxPrim];   // coefficient x norm of the primitive
};
struct FieldPrims : GtoPrims {};
struct FieldAos {
    uint8_t off[kGtoMaxAo];      // first primitive of the function's shell
    uint8_t np[kGtoMaxAo];       // primitives of the shell
    uint8_t kind[kGtoMaxAo];     // 0: s; 1, 2, 3: p_x, p_y, p_z; 4 ... 8: the d functions (spd_mono)
    uint8_t atom[kGtoMaxAo];
};

// ---- s functions -------------------------------------------------------------------------------
// thread idx = i N + j of geometry blockIdx.y
__global__ __launch_bounds__(256) void field_sgrad_kernel(FieldSBasis bs, const double *__restrict__ coords, int N, int K,
                                                           double ox, double oy, double oz, double *__restrict__ ipdip) {
    const int idx = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y, n2 = N * N;
    if (idx >= n2) return;
    const int i = idx / N, j = idx - i * N;
    const double *Ri = coords + ((int64_t)g * N + i) * 3, *Rj = coords + ((int64_t)g * N + j) * 3;
    const double A[3] = {Ri[0], Ri[1], Ri[2]}, B[3] = {Rj[0], Rj[1], Rj[2]}, O[3] = {ox, oy, oz};
    const double d[3] = {A[0] - B[0], A[1] - B[1], A[2] - B[2]}, r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    double acc[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    for (int ia = 0; ia < K; ++ia)
        for (int ib = 0; ib < K; ++ib) {
            const double ea = bs.ex[ia], eb = bs.ex[ib], pp = ea + eb, mu = ea * eb / pp, pip = kGtoPi / pp;
            const double sp = pip * sqrt(pip) * exp(-mu * r2) * (bs.cn[ia] * bs.cn[ib]), own = ea / pp;
            double po[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) po[c] = (A[c] == B[c] ? A[c] : (ea * A[c] + eb * B[c]) / pp) - O[c];
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const double ds = -2.0 * mu * d[x];   // d/dA_x of the overlap, per unit of it
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[x][c] = fma(ds * po[c] + (x == c ? own : 0.0), sp, acc[x][c]);
            }
        }
    double *o = ipdip + (int64_t)g * 9 * n2 + idx;
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(int64_t)(x * 3 + c) * n2] = -acc[x][c];   // electron gradient = - centre gradient
}

// ---- shells with l <= 2 ------------------------------------------------------------------------
// One dimension of the overlap of a primitive pair without sqrt(pi / p) and the exponential: s(i', j) for i' <= 4, j <= 2.
GTO_HD void field_os_table(double XA, double XB, double ip, double (&s)[5][3]) {
    s[0][0] = 1.0;
#pragma unroll
    for (int jj = 1; jj < 3; ++jj) s[0][jj] = XB * s[0][jj - 1] + (jj > 1 ? ip * (jj - 1) * s[0][jj - 2] : 0.0);
#pragma unroll
    for (int ii = 1; ii < 5; ++ii)
#pragma unroll
        for (int jj = 0; jj < 3; ++jj)
            s[ii][jj] = XA * s[ii - 1][jj] + (ii > 1 ? ip * (ii - 1) * s[ii - 2][jj] : 0.0) +
                        (jj > 0 ? ip * jj * s[ii - 1][jj - 1] : 0.0);
}

// idx = mu N + nu of geometry g.  Per dimension and monomial pair: the overlap factor s0 and the dipole factor
// r0 = s(i + 1) + (A - O) s(i), and their derivatives for the centre of mu, 2a f(i + 1) - i f(i - 1).
GTO_HD void field_grad_body(int idx, int g, const FieldPrims &bs, const FieldAos &ao, const double *coords, int N, int natm,
                            double ox, double oy, double oz, double *ipdip) {
    if (idx >= N * N) return;
    const int mu = idx / N, nu = idx - mu * N;
    const int km = ao.kind[mu], kn = ao.kind[nu];
    const int nm = spd_nmono(km), nn = spd_nmono(kn);
    const double *Ra = coords + ((int64_t)g * natm + ao.atom[mu]) * 3, *Rb = coords + ((int64_t)g * natm + ao.atom[nu]) * 3;
    const double AO[3] = {Ra[0] - ox, Ra[1] - oy, Ra[2] - oz};
    double acc[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    for (int pa = ao.off[mu]; pa < ao.off[mu] + ao.np[mu]; ++pa)
        for (int pb = ao.off[nu]; pb < ao.off[nu] + ao.np[nu]; ++pb) {
            const double a = bs.ex[pa], b = bs.ex[pb], p = a + b, mup = a * b / p, ip = 0.5 / p, a2 = 2.0 * a;
            double r2 = 0.0, tb[3][5][3];
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const double d = Ra[x] - Rb[x];
                r2 = r2 + d * d;
                field_os_table(-(b / p) * d, (a / p) * d, ip, tb[x]);
            }
            const double pip = kGtoPi / p, w0 = pip * sqrt(pip) * exp(-mup * r2) * bs.cn[pa] * bs.cn[pb];
            for (int im = 0; im < nm; ++im)
                for (int in = 0; in < nn; ++in) {
                    int pm[3], pn[3];
                    double wm, wn, s0[3], r0[3], ds[3], dr[3];
                    spd_mono(km, im, pm[0], pm[1], pm[2], wm);
                    spd_mono(kn, in, pn[0], pn[1], pn[2], wn);
#pragma unroll
                    for (int x = 0; x < 3; ++x) {
                        // s(i', j) for i' <= 4 at the column j
                        double col[5];
#pragma unroll
                        for (int r = 0; r < 5; ++r) col[r] = spd_sel3(pn[x], tb[x][r][0], tb[x][r][1], tb[x][r][2]);
                        const int i = pm[x];
                        const double di = (double)i;
                        const double sm = spd_sel3(i, 0.0, col[0], col[1]), sp1 = spd_sel3(i, col[1], col[2], col[3]),
                                     sp2 = spd_sel3(i, col[2], col[3], col[4]);
                        s0[x] = spd_sel3(i, col[0], col[1], col[2]);
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

__global__ __launch_bounds__(64) void field_grad_kernel(FieldPrims bs, FieldAos ao, const double *__restrict__ coords, int N,
                                                         int natm, double ox, double oy, double oz,
                                                         double *__restrict__ ipdip) {
    field_grad_body(blockIdx.x * 64 + threadIdx.x, blockIdx.y, bs, ao, coords, N, natm, ox, oy, oz, ipdip);
}

// ---- the fold -----------------------------------------------------------------------------------
struct FieldFoldArgs {
    const double *dip, *ipdip, *charges, *coords, *field;
    const int64_t *aoslices;
    double *hcore, *dhcore, *enuc, *gnuc;
    double o[3];
    int n, natm, grad;
};

// the atom whose [start, stop) holds function f; -1 if none does
__device__ __forceinline__ int field_owner(const int64_t *aoslices, int natm, int f) {
    int at = -1;
    for (int a = 0; a < natm; ++a)
        if (f >= aoslices[2 * a] && f < aoslices[2 * a + 1] && at < 0) at = a;
    return at;
}

// thread e = the element pair mu >= nu of geometry blockIdx.y
__global__ __launch_bounds__(256) void field_fold_kernel(FieldFoldArgs a) {
    const int e = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y, N = a.n, natm = a.natm;
    if (e >= N * (N + 1) / 2) return;
    const int mu = gto_tri_row(e), nu = e - mu * (mu + 1) / 2;
    const int64_t n2 = (int64_t)N * N, ij = (int64_t)mu * N + nu, ji = (int64_t)nu * N + mu;
    const double F[3] = {a.field[(int64_t)g * 3], a.field[(int64_t)g * 3 + 1], a.field[(int64_t)g * 3 + 2]};
    {
        const double *d = a.dip + (int64_t)g * 3 * n2;
        double *h = a.hcore + (int64_t)g * n2;
        const double v = h[ij] + (F[0] * d[ij] + F[1] * d[n2 + ij] + F[2] * d[2 * n2 + ij]);
        h[ij] = v;
        h[ji] = v;
    }
    if (a.grad) {
        const int am = field_owner(a.aoslices, natm, mu), an = field_owner(a.aoslices, natm, nu);
        const double *ip = a.ipdip + (int64_t)g * 9 * n2;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            // the row term of mu on the atom of mu, the column term of nu on the atom of nu
            const double ta = -(F[0] * ip[(x * 3) * n2 + ij] + F[1] * ip[(x * 3 + 1) * n2 + ij] + F[2] * ip[(x * 3 + 2) * n2 + ij]);
            const double tb = -(F[0] * ip[(x * 3) * n2 + ji] + F[1] * ip[(x * 3 + 1) * n2 + ji] + F[2] * ip[(x * 3 + 2) * n2 + ji]);
            if (am >= 0 && am == an) {
                double *da = a.dhcore + (((int64_t)g * natm + am) * 3 + x) * n2;
                const double v = da[ij] + (ta + tb);
                da[ij] = v;
                da[ji] = v;
            } else {
                if (am >= 0) {
                    double *da = a.dhcore + (((int64_t)g * natm + am) * 3 + x) * n2;
                    const double v = da[ij] + ta;
                    da[ij] = v;
                    da[ji] = v;
                }
                if (an >= 0) {
                    double *db = a.dhcore + (((int64_t)g * natm + an) * 3 + x) * n2;
                    const double v = db[ij] + tb;
                    db[ij] = v;
                    db[ji] = v;
                }
            }
        }
    }
    if (e != 0) return;
    // nuclear terms, the atoms in ascending order
    const double *Rg = a.coords + (int64_t)g * natm * 3;
    double en = 0.0;
    for (int c = 0; c < natm; ++c) {
        const double z = a.charges[c];
        en = en + z * (F[0] * (Rg[c * 3] - a.o[0]) + F[1] * (Rg[c * 3 + 1] - a.o[1]) + F[2] * (Rg[c * 3 + 2] - a.o[2]));
        if (a.grad) {
            double *gn = a.gnuc + ((int64_t)g * natm + c) * 3;
            gn[0] = gn[0] - z * F[0];
            gn[1] = gn[1] - z * F[1];
            gn[2] = gn[2] - z * F[2];
        }
    }
    a.enuc[g] = a.enuc[g] - en;
}

// ---- host side ----------------------------------------------------------------------------------
struct FieldRoute {
    using Prims = FieldPrims;
    using Aos = FieldAos;
    static constexpr int kMaxL = 2;
    static constexpr const char *kLs = "0, 1 and 2", *kName = "field";
    static void tag(FieldAos &ao, int f, int l, int c) { ao.kind[f] = (uint8_t)(l == 0 ? 0 : (l == 1 ? 1 + c : 4 + c)); }
};

static bool field_aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace evc

using namespace evc;

extern "C" int evc_sgto_dipole_grad_batch(int natm, int nprim, int count, const double *coords, const double *ex,
                                          const double *co, const double origin[3], double *ipdip, void *stream) {
    const char *who = "evc_sgto_dipole_grad_batch";
    EVC_REQUIRE(natm >= 1 && natm <= kFieldSMaxAtoms, "%s: natm=%d, supported 1 ... %d", who, natm, kFieldSMaxAtoms);
    EVC_REQUIRE(nprim >= 1 && nprim <= kFieldSMaxPrim, "%s: nprim=%d, supported 1 ... %d", who, nprim, kFieldSMaxPrim);
    EVC_REQUIRE(count >= 1 && count <= kFieldMaxCount, "%s: count=%d, supported 1 ... %d", who, count, kFieldMaxCount);
    EVC_REQUIRE(coords && ex && co && origin && ipdip, "%s: null pointer", who);
    EVC_REQUIRE(field_aligned8(coords) && field_aligned8(ipdip), "%s: misaligned pointer (8 bytes)", who);
    FieldSBasis bs;
    for (int k = 0; k < kFieldSMaxPrim; ++k) {
        bs.ex[k] = 1.0;
        bs.cn[k] = 0.0;
    }
    for (int k = 0; k < nprim; ++k) {
        EVC_REQUIRE(ex[k] > 0.0 && isfinite(ex[k]), "%s: exponent %d is %g, must be positive", who, k, ex[k]);
        bs.ex[k] = ex[k];
        bs.cn[k] = co[k] * pow(2.0 * ex[k] / kGtoPi, 0.75);
    }
    gto_launch(field_sgrad_kernel, dim3((unsigned)ceil_div((int64_t)natm * natm, 256), (unsigned)count), dim3(256),
               as_stream(stream), bs, coords, natm, nprim, origin[0], origin[1], origin[2], ipdip);
    EVC_LAUNCH_CHECK("field_sgrad_kernel");
    return 0;
}

extern "C" int evc_gto_dipole_grad_batch(int natm, int nshell, int count, const double *coords, const int *shell_atom,
                                         const int *shell_l, const int *shell_prim_offset, const double *exponents,
                                         const double *coefficients, const double origin[3], double *ipdip, void *stream) {
    const char *who = "evc_gto_dipole_grad_batch";
    FieldPrims bs;
    FieldAos ao;
    int nprim = 0, N = 0;
    if (int rc = gto_describe<FieldRoute>(who, natm, nshell, count, shell_atom, shell_l, shell_prim_offset, exponents,
                                          coefficients, bs, ao, nprim, N))
        return rc;
    EVC_REQUIRE(coords && origin && ipdip, "%s: null pointer", who);
    EVC_REQUIRE(field_aligned8(coords) && field_aligned8(ipdip), "%s: misaligned pointer (8 bytes)", who);
    gto_launch(field_grad_kernel, dim3((unsigned)ceil_div((int64_t)N * N, 64), (unsigned)count), dim3(64), as_stream(stream),
               bs, ao, coords, N, natm, origin[0], origin[1], origin[2], ipdip);
    EVC_LAUNCH_CHECK("field_grad_kernel");
    return 0;
}

extern "C" int evc_field_fold_batch(int n, int natm, int count, const double *dip, const double *ipdip,
                                    const int64_t *aoslices, const double *charges, const double *coords,
                                    const double *field, const double origin[3], int flags, double *hcore, double *dhcore,
                                    double *enuc, double *gnuc, void *stream) {
    const char *who = "evc_field_fold_batch";
    EVC_REQUIRE(n >= 1 && n <= kFieldMaxN, "%s: n=%d, supported 1 ... %d", who, n, kFieldMaxN);
    EVC_REQUIRE(natm >= 1 && natm <= kFieldMaxAtoms, "%s: natm=%d, supported 1 ... %d", who, natm, kFieldMaxAtoms);
    EVC_REQUIRE(count >= 1 && count <= kFieldMaxCount, "%s: count=%d, supported 1 ... %d", who, count, kFieldMaxCount);
    EVC_REQUIRE((flags & ~EVC_FLAG_ENERGY_ONLY) == 0, "%s: flags=%d, accepted EVC_FLAG_ENERGY_ONLY", who, flags);
    const bool grad = !(flags & EVC_FLAG_ENERGY_ONLY);
    EVC_REQUIRE(dip && charges && coords && field && origin && hcore && enuc, "%s: null pointer among dip, charges, coords, "
                "field, origin, hcore, enuc", who);
    EVC_REQUIRE(!grad || (ipdip && aoslices && dhcore && gnuc), "%s: null pointer among ipdip, aoslices, dhcore, gnuc "
                "(allowed only with EVC_FLAG_ENERGY_ONLY)", who);
    EVC_REQUIRE(field_aligned8(dip) && field_aligned8(ipdip) && field_aligned8(aoslices) && field_aligned8(charges) &&
                field_aligned8(coords) && field_aligned8(field) && field_aligned8(hcore) && field_aligned8(dhcore) &&
                field_aligned8(enuc) && field_aligned8(gnuc), "%s: misaligned pointer (8 bytes)", who);
    FieldFoldArgs a;
    a.dip = dip;
    a.ipdip = grad ? ipdip : nullptr;
    a.charges = charges;
    a.coords = coords;
    a.field = field;
    a.aoslices = grad ? aoslices : nullptr;
    a.hcore = hcore;
    a.dhcore = grad ? dhcore : nullptr;
    a.enuc = enuc;
    a.gnuc = grad ? gnuc : nullptr;
    a.o[0] = origin[0];
    a.o[1] = origin[1];
    a.o[2] = origin[2];
    a.n = n;
    a.natm = natm;
    a.grad = grad ? 1 : 0;
    gto_launch(field_fold_kernel, dim3((unsigned)ceil_div((int64_t)n * (n + 1) / 2, 256), (unsigned)count), dim3(256),
               as_stream(stream), a);
    EVC_LAUNCH_CHECK("field_fold_kernel");
    return 0;
}
