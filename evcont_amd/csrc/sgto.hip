// AO integrals and their first nuclear derivatives of a molecule built from one contracted s Gaussian per centre, the same
// contraction on every centre (evc_sgto_integrals_batch): the device statement of evcont_amd/hchain.py s_gaussian_mol,
// term for term, written straight into the arrays of an evc_geometry_batch.  Closed forms over primitives, Boys F0 / F1.
//   primitive pair (a on centre i, b on centre j):  p = a + b, mu = a b / p, AB = R_i - R_j, Kab = exp(-mu |AB|^2),
//                                                    P = (a R_i + b R_j) / p, cn_a = c_a (2 a / pi)^(3/4)
//   (ij|kl)              = sum_abcd  w F0(t),        w = 2 pi^2.5 / (p q sqrt(p + q)) Kab cn_a cn_b Kcd cn_c cn_d,
//                                                    rho = p q / (p + q), t = rho |P - Q|^2
//   int2e_ip1[x,i,j,k,l] = sum_abcd  w (2 mu AB_x F0(t) + 2 rho (a / p) (P - Q)_x F1(t))
// Four VALU kernels in launches of their own (FP64 MFMA blocks its SIMD's vector issue):
//   sgto_pair_kernel   the pair table, one launch per call, one thread per ORDERED contracted pair (i, j) and primitive pair
//                      ab = a K + b (a on i).  Per geometry it has two parts:
//                        ket  [field][ab][e], e = i(i+1)/2 + j, i >= j; fields p, P, Kab cn_a cn_b: lanes that run over e
//                             read consecutive doubles;
//                        bra  [i N + j][ab][12]: p, P, Kab cn_a cn_b, mu AB, a / p, mu, a, b: one row is what a block of the
//                             kernels below reads for a primitive pair, at a wave-uniform address (scalar loads).
//   sgto_two_kernel    one thread per (mu, nu, kappa >= lambda): blockIdx.y names the bra pair, the threads run over the
//                      packed ket index v, blockIdx.z is the geometry -- the cut of fci_row_pack_kernel.  Every thread walks
//                      the K^4 primitive quartets in one fixed order (ket pair outer, bra pair inner), evaluates F0 and F1
//                      once per quartet and keeps int2e and the three components of int2e_ip1 in registers.  int2e is stored
//                      by the blocks mu >= nu alone, to every image they own, so it has the same bits with and without
//                      EVC_FLAG_ENERGY_ONLY (<false>: blocks mu >= nu only, F0 only) and is exactly symmetric within each
//                      index pair.  No screening: every quartet is evaluated.
//   sgto_one_kernel    one wave per contracted pair i >= j; the lanes run over the nuclei, each sums the attraction terms of
//                      its nuclei over the K^2 primitive pairs and the wave adds them up in a fixed order (wave_sum).  S and
//                      hcore are mirrored, so both are exactly symmetric; dhcore gets the operator term of every nucleus and
//                      the moving-basis rows and columns of hchain.py (element [at, :, at, at] twice).
//   sgto_nuc_kernel    nuclear repulsion and its gradient, one thread per centre.
// The contraction is a HOST argument and reaches the pair kernel by value.  fp contraction is off in the kernels and every
// fused multiply-add is written out: the two instantiations of sgto_two_kernel must round int2e alike.
// Of gto_shells.hpp, the core of the shell routes, this file takes the launch helper gto_launch and the flags kGtoFlags.
#include "gto_shells.hpp"

namespace evc {

constexpr int kSgtoMaxAtoms = 96;        // centres
constexpr int kSgtoMaxPacked = 64;       // ... with EVC_FLAG_ERI_S4 / EVC_FLAG_IP1_S2KL (the evaluator's limit)
constexpr int kSgtoMaxPrim = 8;          // primitives of the contraction
constexpr int kSgtoMaxCount = 65535;     // geometries per call (gridDim.z)
constexpr int kSgtoKet = 5;            // fields of the ket part of the pair table
constexpr int kSgtoBra = 12;           // doubles of a row of its bra part

struct SgtoBasis {
    double ex[kSgtoMaxPrim];   // exponents
    double cn[kSgtoMaxPrim];   // coefficient x norm of the primitive
};

// doubles of the pair table of one geometry: the ket part, then the bra part
__host__ __device__ __forceinline__ int64_t sgto_ket_doubles(int N, int K) {
    return (int64_t)kSgtoKet * K * K * (N * (N + 1) / 2);
}
__host__ __device__ __forceinline__ int64_t sgto_table_doubles(int N, int K) {
    return sgto_ket_doubles(N, K) + (int64_t)kSgtoBra * K * K * N * N;
}

// F0(t) and, with F1, F1(t) = -F0'(t) as hchain.boys01 evaluates them: nine Taylor terms below t = 1e-2 (the divisions
// by 2k + 1, 2k + 3 and k + 1 as products with the rounded reciprocals), erf / exp above.
template <bool F1>
__device__ __forceinline__ void sgto_boys(double t, double &f0, double &f1) {
#pragma clang fp contract(off)
    if (t < 1e-2) {
        double term = 1.0, s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            s0 = fma(term, 1.0 / (2 * k + 1), s0);
            if (F1) s1 = fma(term, 1.0 / (2 * k + 3), s1);
            term = term * -t * (1.0 / (k + 1));
        }
        f0 = s0;
        f1 = s1;
    } else {
        const double rt = sqrt(t);
        f0 = 0.8862269254527579 / rt * erf(rt);   // sqrt(pi) / 2
        f1 = F1 ? (f0 - exp(-t)) / (2.0 * t) : 0.0;
    }
}

// ---- pair table ------------------------------------------------------------------------
// thread idx = ab N^2 + (i N + j) of geometry blockIdx.y
__global__ __launch_bounds__(256) void sgto_pair_kernel(SgtoBasis bs, const double *__restrict__ coords, int N, int K,
                                                         double *__restrict__ tab) {
#pragma clang fp contract(off)
    const int K2 = K * K, n2 = N * N, Ms = N * (N + 1) / 2, idx = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
    if (idx >= K2 * n2) return;
    const int ab = idx / n2, o = idx - ab * n2;
    const int ia = ab / K, ib = ab - ia * K;
    const int i = o / N, j = o - i * N;
    const double a = bs.ex[ia], b = bs.ex[ib], w = bs.cn[ia] * bs.cn[ib];
    const double *Ri = coords + ((int64_t)g * N + i) * 3, *Rj = coords + ((int64_t)g * N + j) * 3;
    const double ax = Ri[0], ay = Ri[1], az = Ri[2], bx = Rj[0], by = Rj[1], bz = Rj[2];
    const double p = a + b, mu = a * b / p;
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    // where A_x = B_x (a pair on one centre) P_x is A_x exactly, not within a rounding of it: P - Q and P - C vanish
    // exactly where they do mathematically
    const double px = ax == bx ? ax : (a * ax + b * bx) / p, py = ay == by ? ay : (a * ay + b * by) / p;
    const double pz = az == bz ? az : (a * az + b * bz) / p;
    const double c = exp(-mu * (dx * dx + dy * dy + dz * dz)) * w;
    double *tg = tab + (int64_t)g * sgto_table_doubles(N, K);
    double *row = tg + sgto_ket_doubles(N, K) + ((int64_t)o * K2 + ab) * kSgtoBra;
    row[0] = p;
    row[1] = px;
    row[2] = py;
    row[3] = pz;
    row[4] = c;
    row[5] = mu * dx;
    row[6] = mu * dy;
    row[7] = mu * dz;
    row[8] = a / p;
    row[9] = mu;
    row[10] = a;
    row[11] = b;
    if (i < j) return;
    const int64_t stride = (int64_t)K2 * Ms;
    double *ket = tg + (int64_t)ab * Ms + i * (i + 1) / 2 + j;
    ket[0] = p;
    ket[stride] = px;
    ket[2 * stride] = py;
    ket[3 * stride] = pz;
    ket[4 * stride] = c;
}

// ---- two-electron integrals ----------------------------------------------------------------
// GRAD: gridDim.y = N^2, blockIdx.y = mu N + nu; otherwise gridDim.y = Ms, blockIdx.y = mu (mu + 1) / 2 + nu.
// s4 / s2kl: the forms of eri / eri_ip1 (EVC_FLAG_ERI_S4 / EVC_FLAG_IP1_S2KL).
template <bool GRAD>
__global__ __launch_bounds__(64) void sgto_two_kernel(const double *__restrict__ tab, int N, int K, int s4, int s2kl,
                                                       double *__restrict__ eri, double *__restrict__ ip1) {
#pragma clang fp contract(off)
    const int by = blockIdx.y, g = blockIdx.z, Ms = N * (N + 1) / 2;
    int mu, nu;
    if (GRAD) {
        mu = by / N;
        nu = by - mu * N;
    } else {
        mu = tri_row_small(by);
        nu = by - mu * (mu + 1) / 2;
    }
    const int v = blockIdx.x * 64 + threadIdx.x;
    const bool live = v < Ms;
    const int K2 = K * K;
    const int64_t stride = (int64_t)K2 * Ms;
    const double *tg = tab + (int64_t)g * sgto_table_doubles(N, K);
    const double *bra = tg + sgto_ket_doubles(N, K) + ((int64_t)mu * N + nu) * K2 * kSgtoBra;
    const double *ket = tg + (live ? v : Ms - 1);
    double acc = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    for (int cd = 0; cd < K2; ++cd, ket += Ms) {
        const double q = ket[0], qx = ket[stride], qy = ket[2 * stride], qz = ket[3 * stride], ck = ket[4 * stride];
        for (int ab = 0; ab < K2; ++ab) {
            const double *row = bra + ab * kSgtoBra;
            const double p = row[0], dx = row[1] - qx, dy = row[2] - qy, dz = row[3] - qz;
            const double s = p + q, pq = p * q;
            const double rho = pq / s;
            const double t = rho * (dx * dx + dy * dy + dz * dz);
            const double w = 34.986836655249725 / (pq * sqrt(s)) * row[4] * ck;   // 2 pi^2.5
            double f0, f1;
            sgto_boys<GRAD>(t, f0, f1);
            acc = fma(w, f0, acc);
            if (GRAD) {
                const double w0 = 2.0 * w * f0, w1 = 2.0 * rho * row[8] * w * f1;
                gx = fma(row[5], w0, fma(dx, w1, gx));
                gy = fma(row[6], w0, fma(dy, w1, gy));
                gz = fma(row[7], w0, fma(dz, w1, gz));
            }
        }
    }
    if (!live) return;
    const int kap = tri_row_small(v), lam = v - kap * (kap + 1) / 2;
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

// ---- one-electron integrals ------------------------------------------------------------------
// blockIdx.x = e (contracted pair i >= j), blockIdx.y = geometry; lane l serves the nuclei l and l + 64.  The primitive
// pairs come from the bra row of (i, j) in the pair table.
template <bool GRAD>
__global__ __launch_bounds__(64) void sgto_one_kernel(const double *__restrict__ tab, const double *__restrict__ coords,
                                                       const double *__restrict__ charges, int N, int K,
                                                       double *__restrict__ S, double *__restrict__ hcore,
                                                       double *__restrict__ ipovlp, double *__restrict__ dhcore) {
#pragma clang fp contract(off)
    constexpr double kPi = 3.141592653589793;
    const int e = blockIdx.x, g = blockIdx.y, lane = threadIdx.x, K2 = K * K;
    const int i = tri_row_small(e), j = e - i * (i + 1) / 2;
    const double *Rg = coords + (int64_t)g * N * 3;
    const double *bra = tab + (int64_t)g * sgto_table_doubles(N, K) + sgto_ket_doubles(N, K) +
                        ((int64_t)i * N + j) * K2 * kSgtoBra;
    const double dx = Rg[i * 3] - Rg[j * 3], dy = Rg[i * 3 + 1] - Rg[j * 3 + 1], dz = Rg[i * 3 + 2] - Rg[j * 3 + 2];
    const double r2 = dx * dx + dy * dy + dz * dz;
    // overlap and kinetic energy with their derivatives for the centre of i (those for the centre of j: the negatives)
    double s = 0.0, tk = 0.0, ds[3] = {0.0, 0.0, 0.0}, dt[3] = {0.0, 0.0, 0.0};
    for (int ab = 0; ab < K2; ++ab) {
        const double *row = bra + ab * kSgtoBra;
        const double mu = row[9], pip = kPi / row[0];
        const double sp = pip * sqrt(pip) * row[4], kin = 3.0 - 2.0 * mu * r2;
        s = s + sp;
        tk = fma(mu * kin, sp, tk);
        if (GRAD) {
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const double dsp = -2.0 * row[5 + x] * sp;
                ds[x] = ds[x] + dsp;
                dt[x] = fma(mu, -4.0 * row[5 + x] * sp + kin * dsp, dt[x]);
            }
        }
    }
    // nuclear attraction: this lane's nuclei
    double vn = 0.0, dvi[3] = {0.0, 0.0, 0.0}, dvj[3] = {0.0, 0.0, 0.0}, op[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int c = lane + 64 * r;
        const bool on = c < N;
        const int cc = on ? c : 0;
        const double z = on ? charges[cc] : 0.0;
        const double cx = Rg[cc * 3], cy = Rg[cc * 3 + 1], cz = Rg[cc * 3 + 2];
        double o[3] = {0.0, 0.0, 0.0};
        if (r == 0 || N > 64)   // (wave-uniform)
            for (int ab = 0; ab < K2; ++ab) {
                const double *row = bra + ab * kSgtoBra;
                const double p = row[0], pc[3] = {row[1] - cx, row[2] - cy, row[3] - cz};
                double f0, f1;
                sgto_boys<GRAD>(p * (pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]), f0, f1);
                const double pref = -z * (2.0 * kPi / p) * row[4];
                vn = fma(pref, f0, vn);
                if (GRAD) {
#pragma unroll
                    for (int x = 0; x < 3; ++x) {
                        const double m0 = 2.0 * row[5 + x] * f0;
                        dvi[x] = fma(pref, -m0 - 2.0 * row[10] * pc[x] * f1, dvi[x]);
                        dvj[x] = fma(pref, m0 - 2.0 * row[11] * pc[x] * f1, dvj[x]);
                        o[x] = fma(pref, 2.0 * p * pc[x] * f1, o[x]);
                    }
                }
            }
#pragma unroll
        for (int x = 0; x < 3; ++x) op[r][x] = o[x];
    }
    const double h = tk + wave_sum(vn);
    const int64_t n2 = (int64_t)N * N, ij = (int64_t)i * N + j, ji = (int64_t)j * N + i;
    if (lane == 0) {
        S[g * n2 + ij] = s;
        S[g * n2 + ji] = s;
        hcore[g * n2 + ij] = h;
        hcore[g * n2 + ji] = h;
    }
    if (!GRAD) return;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        // d hcore_ij / d(centre of i) and d hcore_ji / d(centre of j), nuclei fixed
        const double dhi = dt[x] + wave_sum(dvi[x]), dhj = -dt[x] + wave_sum(dvj[x]);
        if (lane == 0) {
            ipovlp[((int64_t)g * 3 + x) * n2 + ij] = -ds[x];
            if (i != j) ipovlp[((int64_t)g * 3 + x) * n2 + ji] = ds[x];
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int c = lane + 64 * r;
            if (c >= N) continue;
            double *d = dhcore + (((int64_t)g * N + c) * 3 + x) * n2;
            // row `at` first, then column `at`, as hchain.py adds them: [at, :, at, at] gets the term twice
            double vij = op[r][x];
            if (c == i) vij = vij + dhi;
            if (c == j) vij = vij + dhj;
            d[ij] = vij;
            if (i != j) {
                double vji = op[r][x];
                if (c == j) vji = vji + dhj;
                if (c == i) vji = vji + dhi;
                d[ji] = vji;
            }
        }
    }
}

// ---- nuclear repulsion -------------------------------------------------------------------------
// blockIdx.x = geometry; thread i < natm sums over the other centres in ascending order.
template <bool GRAD>
__global__ __launch_bounds__(128) void sgto_nuc_kernel(const double *__restrict__ coords, const double *__restrict__ charges,
                                                        int natm, double *__restrict__ enuc, double *__restrict__ gnuc) {
#pragma clang fp contract(off)
    __shared__ double scratch[2];
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
    const double total = block_sum<2>(on ? en : 0.0, scratch);
    if (i == 0) enuc[g] = total;
}

static int sgto_shape(const char *who, int natm, int nprim, int count) {
    EVC_REQUIRE(natm >= 1 && natm <= kSgtoMaxAtoms, "%s: natm=%d, supported 1 ... %d", who, natm, kSgtoMaxAtoms);
    EVC_REQUIRE(nprim >= 1 && nprim <= kSgtoMaxPrim, "%s: nprim=%d, supported 1 ... %d", who, nprim, kSgtoMaxPrim);
    EVC_REQUIRE(count >= 1 && count <= kSgtoMaxCount, "%s: count=%d, supported 1 ... %d", who, count, kSgtoMaxCount);
    return 0;
}

static size_t sgto_table_bytes(int natm, int nprim, int count) {
    return align_up((size_t)count * (size_t)sgto_table_doubles(natm, nprim) * sizeof(double), 256);
}

}  // namespace evc

using namespace evc;

extern "C" size_t evc_sgto_workspace_bytes(int natm, int nprim, int count) {
    if (sgto_shape("evc_sgto_workspace_bytes", natm, nprim, count)) return 0;
    return sgto_table_bytes(natm, nprim, count);
}

extern "C" int evc_sgto_integrals_batch(int natm, int nprim, int count, const double *coords, const double *charges,
                                        const double *exponents, const double *coefficients, const evc_sgto_outputs *out,
                                        int flags, void *ws, size_t ws_bytes, void *stream) {
    const char *who = "evc_sgto_integrals_batch";
    if (int rc = sgto_shape(who, natm, nprim, count)) return rc;
    EVC_REQUIRE((flags & ~kGtoFlags) == 0, "%s: flags=%d, accepted EVC_FLAG_ENERGY_ONLY, EVC_FLAG_ERI_S4 and "
                "EVC_FLAG_IP1_S2KL", who, flags);
    const bool grad = !(flags & EVC_FLAG_ENERGY_ONLY);
    const int s4 = (flags & EVC_FLAG_ERI_S4) != 0, s2kl = (flags & EVC_FLAG_IP1_S2KL) != 0;
    EVC_REQUIRE(!(s4 || s2kl) || natm <= kSgtoMaxPacked, "%s: the packed forms (EVC_FLAG_ERI_S4, EVC_FLAG_IP1_S2KL) need "
                "natm <= %d, got %d", who, kSgtoMaxPacked, natm);
    EVC_REQUIRE(coords && charges && exponents && coefficients && out && ws, "%s: null pointer", who);
    EVC_REQUIRE(out->enuc && out->S && out->hcore && out->eri, "%s: null pointer among enuc, S, hcore, eri", who);
    EVC_REQUIRE(!grad || (out->ipovlp && out->dhcore && out->eri_ip1 && out->gnuc), "%s: null pointer among ipovlp, dhcore, "
                "eri_ip1, gnuc (allowed only with EVC_FLAG_ENERGY_ONLY)", who);
    SgtoBasis bs;
    for (int k = 0; k < kSgtoMaxPrim; ++k) {
        bs.ex[k] = 1.0;
        bs.cn[k] = 0.0;
    }
    for (int k = 0; k < nprim; ++k) {
        EVC_REQUIRE(exponents[k] > 0.0 && isfinite(exponents[k]), "%s: exponent %d is %g, must be positive", who, k,
                    exponents[k]);
        bs.ex[k] = exponents[k];
        bs.cn[k] = coefficients[k] * pow(2.0 * exponents[k] / 3.141592653589793, 0.75);
    }
    EVC_REQUIRE(aligned16(ws), "%s: workspace not 16-byte aligned", who);
    const size_t need = sgto_table_bytes(natm, nprim, count);
    EVC_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, %zu needed for %d centres, %d primitives, %d geometries", who,
                ws_bytes, need, natm, nprim, count);
    hipStream_t st = as_stream(stream);
    const int N = natm, K = nprim, Ms = N * (N + 1) / 2;
    double *tab = static_cast<double *>(ws);
    gto_launch(sgto_pair_kernel, dim3((unsigned)ceil_div((int64_t)K * K * N * N, 256), (unsigned)count), dim3(256), st, bs,
               coords, N, K, tab);
    EVC_LAUNCH_CHECK("sgto_pair_kernel");
    const dim3 grid1((unsigned)Ms, (unsigned)count), grid2((unsigned)ceil_div(Ms, 64), (unsigned)(grad ? N * N : Ms),
                                                           (unsigned)count);
    if (grad) {
        gto_launch(sgto_one_kernel<true>, grid1, dim3(64), st, (const double *)tab, coords, charges, N, K, out->S,
                   out->hcore, out->ipovlp, out->dhcore);
        EVC_LAUNCH_CHECK("sgto_one_kernel");
        gto_launch(sgto_nuc_kernel<true>, dim3((unsigned)count), dim3(128), st, coords, charges, N, out->enuc, out->gnuc);
        EVC_LAUNCH_CHECK("sgto_nuc_kernel");
        gto_launch(sgto_two_kernel<true>, grid2, dim3(64), st, (const double *)tab, N, K, s4, s2kl, out->eri, out->eri_ip1);
    } else {
        gto_launch(sgto_one_kernel<false>, grid1, dim3(64), st, (const double *)tab, coords, charges, N, K, out->S,
                   out->hcore, (double *)nullptr, (double *)nullptr);
        EVC_LAUNCH_CHECK("sgto_one_kernel");
        gto_launch(sgto_nuc_kernel<false>, dim3((unsigned)count), dim3(128), st, coords, charges, N, out->enuc,
                   (double *)nullptr);
        EVC_LAUNCH_CHECK("sgto_nuc_kernel");
        gto_launch(sgto_two_kernel<false>, grid2, dim3(64), st, (const double *)tab, N, K, s4, 0, out->eri,
                   (double *)nullptr);
    }
    EVC_LAUNCH_CHECK("sgto_two_kernel");
    return 0;
}
