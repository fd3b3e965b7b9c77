// Observables of continuation states (evc_properties_roots_batch): the predicted (transition) 1-RDM of every root pair of
// every geometry of a batch, its back-rotation to the AO basis, dipole moments, Mulliken and Loewdin populations -- the
// device statement of evcont_amd/properties.py -- and the one AO integral they need that evc_sgto_integrals_batch does not
// produce, the dipole integrals of s-Gaussian molecules (evc_sgto_dipole_batch).
// Slots s = p * count + g as in roots.hip: pair p = (k, l) of geometry g, weighting W = (c_k c_l^T + c_l c_k^T) / 2.
// Three VALU kernels, every launch through prop_launch (tests/test_properties_closure.py):
//   prop_d1_kernel<NS>  D[s] = sum_ab W_s[a,b] one_rdm[a T + b, :N^2] for a group of up to 32 consecutive slots: one thread
//                       per column, blockIdx.y a chunk of rows of one_rdm, blockIdx.x a tile of 256 columns.  The weights
//                       of 64 rows x NS slots are formed in LDS from the coefficient rows as they are used (the left
//                       operand is never in memory); every element of one_rdm a block loads feeds NS accumulators, so
//                       one_rdm is read once per group.  NS: the group's slots rounded up to a power of two (absent slots
//                       get zero weights and are not stored).  Chunk c of slot s goes to part[c][s][:N^2] in the caller's
//                       scratch; the chunks are a function of T alone (prop_rows_per_chunk), so no result depends on the
//                       grid.  Vector FMA, not FP64 MFMA: the product has K = T^2 and M = slots <= 32 -- at the sizes of
//                       the workflow (1 .. 10 root pairs) most of a 16-row MFMA tile would multiply zeros, the kernel is
//                       bound by the stream of one_rdm, and an MFMA blocks its SIMD's vector issue.
//   prop_ao_kernel<TM>  one workgroup of 16 x 16 threads per slot: X_g and D_s = the chunks added in ascending order (the
//                       second, fixed-order summing step) go to LDS at the odd pitch N | 1 (two 96 x 97 matrices and the
//                       reduction words are 149 824 of the 163 840 bytes of a CU, so every N takes this one form); thread
//                       (ty, tx) owns the elements (ty + 16 m, tx + 16 q), m, q < TM, of M = X D (which replaces D in LDS)
//                       and then of P = M X^T (which replaces X); then tr(P r_x), the Mulliken row sums (P S)_mu,mu and the
//                       atom sums over aoslices, every sum in a fixed order (wave_sum / block_sum, ascending loops).
//   prop_sdip_kernel    one thread per contracted pair i >= j of a geometry, primitive pairs in ascending order, mirrored:
//                       dip[x,i,j] = sum_ab cn_a cn_b (pi / p)^1.5 Kab (P_x - O_x), P as in sgto.hip.
// Every sum has one order; no library state, no profile stage; nothing but the outputs and the caller's scratch is written.
#include <math.h>
#include <string.h>

#include "pipeline.hpp"

namespace evc {

constexpr int kPropGroup = 32;       // slots that share one pass over one_rdm
constexpr int kPropRowsMin = 256;    // rows of one_rdm per chunk, at least; T^2 beyond it is split over blocks
constexpr int kPropMaxChunks = 64;
constexpr int kPropRowTile = 64;     // rows whose weights are in LDS at a time
constexpr int kPropMaxSlots = 4096;
constexpr int kPropMaxAtoms = 65535;
constexpr int kSdipMaxAtoms = 96;    // the limits of evc_sgto_integrals_batch
constexpr int kSdipMaxPrim = 8;
constexpr int kSdipMaxCount = 65535;

// Every launch of this file: the runtime call, not the chevrons (tests/test_properties_closure.py).
template <typename T>
struct prop_same_type {
    using type = T;
};
template <typename... P>
static void prop_launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st,
                        typename prop_same_type<P>::type... a) {
    void *args[] = {(void *)&a...};
    // the result is read by the EVC_LAUNCH_CHECK (hipGetLastError) that follows the call
    (void)hipLaunchKernel(reinterpret_cast<const void *>(kernel), grid, block, args, lds, st);
}

// rows of one_rdm per chunk: a function of T alone
__host__ __device__ __forceinline__ int prop_rows_per_chunk(int T) {
    const int rows = T * T, per = ((rows + kPropMaxChunks - 1) / kPropMaxChunks + 63) / 64 * 64;
    return per > kPropRowsMin ? per : kPropRowsMin;
}
static int prop_chunks(int T) { return (T * T + prop_rows_per_chunk(T) - 1) / prop_rows_per_chunk(T); }

struct PropD1Args {
    const double *one_rdm;   // (T^2, ld1)
    int64_t ld1;
    const double *coeffs;    // (count, T, T)
    double *part;            // (chunks, nslots, N^2)
    int T, n2, count, nslots, s0, ns, rpc;
    int16_t k[kPropGroup], l[kPropGroup];
};

template <int NS>
__global__ __launch_bounds__(256) void prop_d1_kernel(PropD1Args a) {
    __shared__ double w[kPropRowTile][NS];
    const int tid = threadIdx.x, c = blockIdx.x * 256 + tid, chunk = blockIdx.y, T = a.T, T2 = T * T;
    const int r0 = chunk * a.rpc, r1 = r0 + a.rpc < T2 ? r0 + a.rpc : T2;
    const bool live = c < a.n2;
    double acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0.0;
    for (int rt = r0; rt < r1; rt += kPropRowTile) {
        for (int i = tid; i < kPropRowTile * NS; i += 256) {
            const int rr = i / NS, s = i - rr * NS, r = rt + rr;
            double v = 0.0;
            if (r < r1 && s < a.ns) {
                const int ia = r / T, ib = r - ia * T, kk = a.k[s], ll = a.l[s];
                const double *cb = a.coeffs + (int64_t)((a.s0 + s) % a.count) * T2;
                const double *ck = cb + (int64_t)kk * T, *cl = cb + (int64_t)ll * T;
                v = kk == ll ? ck[ia] * ck[ib] : 0.5 * (ck[ia] * cl[ib] + cl[ia] * ck[ib]);
            }
            w[rr][s] = v;
        }
        __syncthreads();
        if (live) {
            const int nr = r1 - rt < kPropRowTile ? r1 - rt : kPropRowTile;
            const double *A = a.one_rdm + (int64_t)rt * a.ld1 + c;
            for (int rr = 0; rr < nr; ++rr) {
                const double v = A[(int64_t)rr * a.ld1];
#pragma unroll
                for (int s = 0; s < NS; ++s) acc[s] = fma(w[rr][s], v, acc[s]);
            }
        }
        __syncthreads();
    }
    if (!live) return;
#pragma unroll
    for (int s = 0; s < NS; ++s)
        if (s < a.ns) a.part[((int64_t)chunk * a.nslots + a.s0 + s) * a.n2 + c] = acc[s];
}

struct PropAoArgs {
    const double *part;      // (chunks, nslots, N^2)
    const double *X;         // X of geometry 0 in the evaluation workspace; geometry g at X + g * sX
    int64_t sX;
    const double *S, *dip, *charges, *coords;
    const int64_t *aoslices;
    double ox, oy, oz;
    double *d_oao, *d_ao, *dipole, *mulliken, *loewdin;
    int nchunks, nslots, n, natm, count;
    uint32_t diag[kPropMaxSlots / 32];   // bit p: pair p is a diagonal pair (k == l)
};

// [lo, hi) of atom `at`, cut to the orbitals there are
__device__ __forceinline__ void prop_slice(const int64_t *aoslices, int at, int n, int &lo, int &hi) {
    const int64_t b = aoslices[2 * at], e = aoslices[2 * at + 1];
    lo = b < 0 ? 0 : b > n ? n : (int)b;
    hi = e < lo ? lo : e > n ? n : (int)e;
}

__host__ __device__ __forceinline__ size_t prop_ao_lds_bytes(int n) {
    return sizeof(double) * ((size_t)2 * n * (n | 1) + n + 8);
}

template <int TM>
__global__ __launch_bounds__(256) void prop_ao_kernel(PropAoArgs a) {
    extern __shared__ double prop_lds[];
    const int n = a.n, ldp = n | 1, n2 = n * n, s = blockIdx.x, g = s % a.count, p = s / a.count, natm = a.natm;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    double *sX = prop_lds, *sD = sX + n * ldp, *sq = sD + n * ldp, *red = sq + n;
    const double *Xg = a.X + (int64_t)g * a.sX;
    for (int e = tid; e < n2; e += 256) {
        const int i = e / n, j = e - i * n;
        sX[i * ldp + j] = Xg[e];
        double d = 0.0;
        for (int c = 0; c < a.nchunks; ++c) d += a.part[((int64_t)c * a.nslots + s) * n2 + e];
        sD[i * ldp + j] = d;
        if (a.d_oao) a.d_oao[(int64_t)s * n2 + e] = d;
    }
    __syncthreads();
    if (a.loewdin)   // the OAO basis is the Loewdin basis: the diagonal of D
        for (int at = tid; at < natm; at += 256) {
            int lo, hi;
            prop_slice(a.aoslices, at, n, lo, hi);
            double q = 0.0;
            for (int mu = lo; mu < hi; ++mu) q += sD[mu * ldp + mu];
            a.loewdin[(int64_t)s * natm + at] = q;
        }
    if (!a.d_ao && !a.dipole && !a.mulliken) return;
    int ri[TM], cj[TM];
#pragma unroll
    for (int m = 0; m < TM; ++m) {
        ri[m] = ty + 16 * m < n ? ty + 16 * m : n - 1;
        cj[m] = tx + 16 * m < n ? tx + 16 * m : n - 1;
    }
    double acc[TM][TM];
    // M = X D
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int q = 0; q < TM; ++q) acc[m][q] = 0.0;
    for (int k = 0; k < n; ++k) {
        double xv[TM], dv[TM];
#pragma unroll
        for (int m = 0; m < TM; ++m) {
            xv[m] = sX[ri[m] * ldp + k];
            dv[m] = sD[k * ldp + cj[m]];
        }
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
            for (int q = 0; q < TM; ++q) acc[m][q] = fma(xv[m], dv[q], acc[m][q]);
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int q = 0; q < TM; ++q) {
            const int i = ty + 16 * m, j = tx + 16 * q;
            if (i < n && j < n) sD[i * ldp + j] = acc[m][q];
            acc[m][q] = 0.0;
        }
    __syncthreads();
    // P = M X^T
    for (int k = 0; k < n; ++k) {
        double mv[TM], xv[TM];
#pragma unroll
        for (int m = 0; m < TM; ++m) {
            mv[m] = sD[ri[m] * ldp + k];
            xv[m] = sX[cj[m] * ldp + k];
        }
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
            for (int q = 0; q < TM; ++q) acc[m][q] = fma(mv[m], xv[q], acc[m][q]);
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int q = 0; q < TM; ++q) {
            const int i = ty + 16 * m, j = tx + 16 * q;
            if (i < n && j < n) {
                sX[i * ldp + j] = acc[m][q];
                if (a.d_ao) a.d_ao[(int64_t)s * n2 + i * n + j] = acc[m][q];
            }
        }
    __syncthreads();
    if (a.dipole) {   // tr(P r_x) = sum_ij r_x[i,j] P[j,i]
        const double *r = a.dip + (int64_t)g * 3 * n2;
        double d0 = 0.0, d1 = 0.0, d2 = 0.0;
        for (int e = tid; e < n2; e += 256) {
            const int i = e / n, j = e - i * n;
            const double pt = sX[j * ldp + i];
            d0 = fma(r[e], pt, d0);
            d1 = fma(r[n2 + e], pt, d1);
            d2 = fma(r[2 * n2 + e], pt, d2);
        }
        const double t0 = block_sum<4>(d0, red), t1 = block_sum<4>(d1, red), t2 = block_sum<4>(d2, red);
        if (tid == 0) {
            double nx = 0.0, ny = 0.0, nz = 0.0;
            if (a.diag[p >> 5] >> (p & 31) & 1u) {   // a state's own dipole: the nuclei
                const double *R = a.coords + (int64_t)g * natm * 3;
                for (int at = 0; at < natm; ++at) {
                    const double z = a.charges[at];
                    nx = fma(z, R[at * 3] - a.ox, nx);
                    ny = fma(z, R[at * 3 + 1] - a.oy, ny);
                    nz = fma(z, R[at * 3 + 2] - a.oz, nz);
                }
            }
            double *o = a.dipole + (int64_t)s * 3;
            o[0] = nx - t0;
            o[1] = ny - t1;
            o[2] = nz - t2;
        }
    }
    if (a.mulliken) {   // (P S)_mu,mu = sum_nu P[mu,nu] S[nu,mu]
        const double *Sg = a.S + (int64_t)g * n2;
        for (int mu = tid; mu < n; mu += 256) {
            double q = 0.0;
            for (int nu = 0; nu < n; ++nu) q = fma(sX[mu * ldp + nu], Sg[nu * n + mu], q);
            sq[mu] = q;
        }
        __syncthreads();
        for (int at = tid; at < natm; at += 256) {
            int lo, hi;
            prop_slice(a.aoslices, at, n, lo, hi);
            double q = 0.0;
            for (int mu = lo; mu < hi; ++mu) q += sq[mu];
            a.mulliken[(int64_t)s * natm + at] = q;
        }
    }
}

struct SdipBasis {
    double ex[kSdipMaxPrim];   // exponents
    double cn[kSdipMaxPrim];   // coefficient x norm of the primitive
};

// thread idx = i N + j of geometry blockIdx.y; i >= j computes and mirrors
__global__ __launch_bounds__(256) void prop_sdip_kernel(SdipBasis bs, const double *__restrict__ coords, int N, int K,
                                                         double ox, double oy, double oz, double *__restrict__ dip) {
#pragma clang fp contract(off)
    constexpr double kPi = 3.141592653589793;
    const int idx = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y, n2 = N * N;
    if (idx >= n2) return;
    const int i = idx / N, j = idx - i * N;
    if (i < j) return;
    const double *Ri = coords + ((int64_t)g * N + i) * 3, *Rj = coords + ((int64_t)g * N + j) * 3;
    const double ax = Ri[0], ay = Ri[1], az = Ri[2], bx = Rj[0], by = Rj[1], bz = Rj[2];
    const double dx = ax - bx, dy = ay - by, dz = az - bz, r2 = dx * dx + dy * dy + dz * dz;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int ia = 0; ia < K; ++ia)
        for (int ib = 0; ib < K; ++ib) {
            const double ea = bs.ex[ia], eb = bs.ex[ib], pp = ea + eb, mu = ea * eb / pp, pip = kPi / pp;
            const double sp = pip * sqrt(pip) * exp(-mu * r2) * (bs.cn[ia] * bs.cn[ib]);
            // on coincident coordinates P is the centre exactly (hchain.s_gaussian_mol)
            const double px = ax == bx ? ax : (ea * ax + eb * bx) / pp, py = ay == by ? ay : (ea * ay + eb * by) / pp;
            const double pz = az == bz ? az : (ea * az + eb * bz) / pp;
            sx = fma(px - ox, sp, sx);
            sy = fma(py - oy, sp, sy);
            sz = fma(pz - oz, sp, sz);
        }
    double *d = dip + (int64_t)g * 3 * n2;
    const int ij = i * N + j, ji = j * N + i;
    d[ij] = sx;
    d[ji] = sx;
    d[n2 + ij] = sy;
    d[n2 + ji] = sy;
    d[2 * n2 + ij] = sz;
    d[2 * n2 + ji] = sz;
}

static LdsAttr g_prop_ao_lds[3];

template <int NS>
static void prop_d1_go(dim3 grid, hipStream_t st, const PropD1Args &a) {
    prop_launch(prop_d1_kernel<NS>, grid, dim3(256), 0, st, a);
}

static int prop_shape(const char *who, int n, int ntrain, int natm, int count, int npairs) {
    EVC_REQUIRE(n >= 1 && n <= kMaxOrbitals, "%s: n=%d, supported 1 ... %d", who, n, kMaxOrbitals);
    EVC_REQUIRE(ntrain >= 1 && ntrain <= kSubspaceMaxT, "%s: ntrain=%d, supported 1 ... %d", who, ntrain, kSubspaceMaxT);
    EVC_REQUIRE(natm >= 1 && natm <= kPropMaxAtoms, "%s: natm=%d, supported 1 ... %d", who, natm, kPropMaxAtoms);
    EVC_REQUIRE(count >= 1 && npairs >= 1 && (int64_t)count * npairs <= kPropMaxSlots,
                "%s: count=%d, npairs=%d (need count >= 1, npairs >= 1, count * npairs <= %d)", who, count, npairs,
                kPropMaxSlots);
    return 0;
}

static size_t prop_scratch_bytes(int n, int ntrain, int count, int npairs) {
    return align_up((size_t)prop_chunks(ntrain) * count * npairs * n * n * sizeof(double), 256);
}

static int sdip_shape(const char *who, int natm, int nprim, int count) {
    EVC_REQUIRE(natm >= 1 && natm <= kSdipMaxAtoms, "%s: natm=%d, supported 1 ... %d", who, natm, kSdipMaxAtoms);
    EVC_REQUIRE(nprim >= 1 && nprim <= kSdipMaxPrim, "%s: nprim=%d, supported 1 ... %d", who, nprim, kSdipMaxPrim);
    EVC_REQUIRE(count >= 1 && count <= kSdipMaxCount, "%s: count=%d, supported 1 ... %d", who, count, kSdipMaxCount);
    return 0;
}

static bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace evc

using namespace evc;

extern "C" size_t evc_properties_workspace_bytes(int n, int ntrain, int natm, int count, int npairs) {
    if (prop_shape("evc_properties_workspace_bytes", n, ntrain, natm, count, npairs)) return 0;
    return prop_scratch_bytes(n, ntrain, count, npairs);
}

extern "C" int evc_properties_roots_batch(const evc_trdm_set *t, const evc_property_inputs *in, const double *coeffs,
                                          int nvec, const int32_t *pairs, int npairs, const evc_property_outputs *out,
                                          const void *ws, size_t ws_bytes, void *scratch, size_t scratch_bytes,
                                          void *stream) {
    const char *who = "evc_properties_roots_batch";
    EVC_REQUIRE(t && in && coeffs && pairs && out && ws && scratch, "%s: null pointer among t, in, coeffs, pairs, out, ws, "
                "scratch", who);
    if (int rc = prop_shape(who, t->n, t->ntrain, in->natm, in->count, npairs)) return rc;
    if (check_set(t)) {
        char msg[400];
        snprintf(msg, sizeof(msg), "%s", evc_last_error());
        set_error("%s: %s", who, msg);
        return -1;
    }
    const int n = t->n, T = t->ntrain, natm = in->natm, count = in->count, nslots = count * npairs;
    EVC_REQUIRE(nvec >= 1 && nvec <= T, "%s: nvec=%d out of range 1..%d (T)", who, nvec, T);
    PropAoArgs pa;
    memset(&pa, 0, sizeof(pa));
    for (int p = 0; p < npairs; ++p) {
        const int k = pairs[2 * p], l = pairs[2 * p + 1];
        EVC_REQUIRE(0 <= k && k <= l && l < nvec, "%s: pair %d = (%d, %d) outside 0 <= k <= l < nvec=%d", who, p, k, l,
                    nvec);
        if (k == l) pa.diag[p >> 5] |= 1u << (p & 31);
    }
    EVC_REQUIRE(!out->dipole || (in->dip && in->charges && in->coords), "%s: null pointer among dip, charges, coords "
                "(needed for dipole)", who);
    EVC_REQUIRE(!out->mulliken || in->S, "%s: null pointer S (needed for mulliken)", who);
    EVC_REQUIRE(!(out->mulliken || out->loewdin) || in->aoslices, "%s: null pointer aoslices (needed for mulliken / "
                "loewdin)", who);
    EVC_REQUIRE(aligned16(ws) && aligned16(scratch), "%s: ws / scratch misaligned (16 bytes)", who);
    EVC_REQUIRE(aligned8(coeffs) && aligned8(in->S) && aligned8(in->dip) && aligned8(in->charges) &&
                aligned8(in->coords) && aligned8(in->aoslices) && aligned8(out->d_oao) && aligned8(out->d_ao) &&
                aligned8(out->dipole) && aligned8(out->mulliken) && aligned8(out->loewdin),
                "%s: misaligned pointer (8 bytes) among coeffs, the inputs and the outputs", who);
    const size_t need = prop_scratch_bytes(n, T, count, npairs);
    EVC_REQUIRE(scratch_bytes >= need, "%s: scratch of %zu bytes, %zu needed", who, scratch_bytes, need);
    const Ws w = carve(t, natm, const_cast<char *>(static_cast<const char *>(ws)));
    EVC_REQUIRE(ws_bytes >= w.bytes * (size_t)count, "%s: ws of %zu bytes holds no %d geometries of %zu bytes", who,
                ws_bytes, count, w.bytes);
    hipStream_t st = as_stream(stream);
    const int n2 = n * n, nchunks = prop_chunks(T);
    // (1) the chunks of D of every slot, one launch per group of slots
    PropD1Args da;
    memset(&da, 0, sizeof(da));
    da.one_rdm = t->one_rdm;
    da.ld1 = t->ld1;
    da.coeffs = coeffs;
    da.part = static_cast<double *>(scratch);
    da.T = T;
    da.n2 = n2;
    da.count = count;
    da.nslots = nslots;
    da.rpc = prop_rows_per_chunk(T);
    const dim3 grid1((unsigned)ceil_div(n2, 256), (unsigned)nchunks);
    for (int s0 = 0; s0 < nslots; s0 += kPropGroup) {
        const int ns = nslots - s0 < kPropGroup ? nslots - s0 : kPropGroup;
        da.s0 = s0;
        da.ns = ns;
        for (int s = 0; s < ns; ++s) {
            da.k[s] = (int16_t)pairs[2 * ((s0 + s) / count)];
            da.l[s] = (int16_t)pairs[2 * ((s0 + s) / count) + 1];
        }
        if (ns == 1) prop_d1_go<1>(grid1, st, da);
        else if (ns == 2) prop_d1_go<2>(grid1, st, da);
        else if (ns <= 4) prop_d1_go<4>(grid1, st, da);
        else if (ns <= 8) prop_d1_go<8>(grid1, st, da);
        else if (ns <= 16) prop_d1_go<16>(grid1, st, da);
        else prop_d1_go<32>(grid1, st, da);
        EVC_LAUNCH_CHECK("prop_d1_kernel");
    }
    // (2) everything else, one workgroup per slot
    pa.part = da.part;
    pa.X = w.X;
    pa.sX = w.stride;
    pa.S = in->S;
    pa.dip = in->dip;
    pa.charges = in->charges;
    pa.coords = in->coords;
    pa.aoslices = in->aoslices;
    pa.ox = in->origin[0];
    pa.oy = in->origin[1];
    pa.oz = in->origin[2];
    pa.d_oao = out->d_oao;
    pa.d_ao = out->d_ao;
    pa.dipole = out->dipole;
    pa.mulliken = out->mulliken;
    pa.loewdin = out->loewdin;
    pa.nchunks = nchunks;
    pa.nslots = nslots;
    pa.n = n;
    pa.natm = natm;
    pa.count = count;
    if (!pa.d_oao && !pa.d_ao && !pa.dipole && !pa.mulliken && !pa.loewdin) return 0;
    const size_t lds = prop_ao_lds_bytes(n);
    const dim3 grid2((unsigned)nslots);
    if (n <= 32) {
        EVC_TRY(allow_dynamic_lds(prop_ao_kernel<2>, g_prop_ao_lds[0], (int)prop_ao_lds_bytes(32), "prop_ao_kernel<2>"));
        prop_launch(prop_ao_kernel<2>, grid2, dim3(256), lds, st, pa);
    } else if (n <= 64) {
        EVC_TRY(allow_dynamic_lds(prop_ao_kernel<4>, g_prop_ao_lds[1], (int)prop_ao_lds_bytes(64), "prop_ao_kernel<4>"));
        prop_launch(prop_ao_kernel<4>, grid2, dim3(256), lds, st, pa);
    } else {
        EVC_TRY(allow_dynamic_lds(prop_ao_kernel<6>, g_prop_ao_lds[2], (int)prop_ao_lds_bytes(96), "prop_ao_kernel<6>"));
        prop_launch(prop_ao_kernel<6>, grid2, dim3(256), lds, st, pa);
    }
    EVC_LAUNCH_CHECK("prop_ao_kernel");
    return 0;
}

extern "C" int evc_sgto_dipole_batch(int natm, int nprim, int count, const double *coords, const double *ex,
                                     const double *co, const double origin[3], double *dip, void *stream) {
    const char *who = "evc_sgto_dipole_batch";
    if (int rc = sdip_shape(who, natm, nprim, count)) return rc;
    EVC_REQUIRE(coords && ex && co && origin && dip, "%s: null pointer", who);
    EVC_REQUIRE(aligned8(coords) && aligned8(dip), "%s: misaligned pointer (8 bytes)", who);
    SdipBasis bs;
    for (int k = 0; k < kSdipMaxPrim; ++k) {
        bs.ex[k] = 1.0;
        bs.cn[k] = 0.0;
    }
    for (int k = 0; k < nprim; ++k) {
        EVC_REQUIRE(ex[k] > 0.0 && isfinite(ex[k]), "%s: exponent %d is %g, must be positive", who, k, ex[k]);
        bs.ex[k] = ex[k];
        bs.cn[k] = co[k] * pow(2.0 * ex[k] / 3.141592653589793, 0.75);
    }
    prop_launch(prop_sdip_kernel, dim3((unsigned)ceil_div((int64_t)natm * natm, 256), (unsigned)count), dim3(256), 0,
                as_stream(stream), bs, coords, natm, nprim, origin[0], origin[1], origin[2], dip);
    EVC_LAUNCH_CHECK("prop_sdip_kernel");
    return 0;
}
