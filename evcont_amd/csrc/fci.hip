// Full-CI training states on the device (fci_small.py: SmallFCI._excite_all, .trans_rdm12, .contract):
//   excite      D[pq](Ia,Ib) = sa c(Ja,Ib) + sb c(Ia,Jb)      signed gather through the string tables
//   t-RDM       M = D~_bra . D_ket^T  (N^2 x dim x N^2)       split-K FP64 MFMA, partial tiles summed in a fixed order
//   sigma       G = h2 . D            (N^2 x N^2 x dim)       FP64 MFMA over determinant tiles, then the signed gather of
//               sigma = sum_pq E_pq (G[pq]/2 + h'_pq c)       G back through the tables
//   rows        evc_fci_trdm_rows: the dense t-RDMs of one bra against K kets; evc_fci_trdm_rows_packed: the same product
//               (one function, fci_trdm_rows_run) with each ket's two-body block packed on the device into a row of the
//               evaluator's matrix (fci_pack.hip); evc_fci_trdm_rows_block: up to kTrdmBras bras against shared kets, the
//               ket-side D of a determinant chunk formed once for every bra that sees the ket
// D is materialised in HBM in chunks (the caller's workspace), so that the MFMA kernels issue nothing but operand
// loads and MFMAs and the gather work runs in launches of its own (FP64 MFMA blocks its SIMD's vector issue).
//
// String tables (fci_tables.py): tab[I * npad + pq] = +-(J + 1) with <I| a_p^+ a_q |J> = +-1, 0 where E_pq annihilates
// every string into I; npad = N^2 rounded up to 16, the pad columns are 0.  One table per spin.
//
// Both matrix kernels contract operands stored [k][m] (m contiguous), so every MFMA fragment load is 16 consecutive
// doubles: the t-RDM reads D determinant-major ([k][pq]), sigma reads h2^T [rs][pq] and D orbital-major ([rs][k]).
#include "common.hpp"
#include "kernels.hpp"

namespace evc {

static int fci_npad(int norb) { return (norb * norb + 15) / 16 * 16; }
// sigma: row tiles per wave for nt = npad / 16 tiles
static int fci_rt(int nt) { return (int)ceil_div(nt, ceil_div(nt, 4)); }

// ---- excite ----------------------------------------------------------------------
__device__ __forceinline__ double fci_excite_one(const int32_t *__restrict__ tab_a, const int32_t *__restrict__ tab_b,
                                                 const double *__restrict__ c, int64_t nb, int npad, int64_t ia,
                                                 int64_t ib, int pq) {
    const int32_t ta = tab_a[ia * npad + pq], tb = tab_b[ib * npad + pq];
    double v = 0.0;
    if (ta != 0) {
        const double x = c[(int64_t)(abs(ta) - 1) * nb + ib];
        v = ta > 0 ? x : -x;
    }
    if (tb != 0) {
        const double x = c[ia * nb + (abs(tb) - 1)];
        v += tb > 0 ? x : -x;
    }
    return v;
}

// LAYOUT 0: D[kk * npad + pq]; 1: D[kk * npad + qp] (the bra side of the t-RDM product); rows kk with k0 + kk >= dim
// and the pad columns are written as zeros.
template <int LAYOUT>
__global__ __launch_bounds__(256) void fci_excite_det_kernel(const int32_t *__restrict__ tab_a,
                                                             const int32_t *__restrict__ tab_b,
                                                             const double *__restrict__ c, int norb, int64_t nb,
                                                             int64_t dim, int64_t k0, int64_t nk, int npad,
                                                             double *__restrict__ D) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nk * npad) return;
    const int64_t kk = idx / npad, k = k0 + kk;
    const int pq = (int)(idx - kk * npad);
    double v = 0.0;
    if (k < dim) v = fci_excite_one(tab_a, tab_b, c, nb, npad, k / nb, k % nb, pq);
    int col = pq;
    if (LAYOUT == 1 && pq < norb * norb) col = (pq % norb) * norb + pq / norb;
    D[kk * npad + col] = v;
}

// D[pq * ld + kk], pq < npad, kk < nk (nk <= ld)
__global__ __launch_bounds__(256) void fci_excite_orb_kernel(const int32_t *__restrict__ tab_a,
                                                             const int32_t *__restrict__ tab_b,
                                                             const double *__restrict__ c, int64_t nb, int64_t dim,
                                                             int64_t k0, int64_t nk, int npad, double *__restrict__ D,
                                                             int64_t ld) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nk * npad) return;
    const int pq = (int)(idx / nk);
    const int64_t kk = idx - (int64_t)pq * nk, k = k0 + kk;
    double v = 0.0;
    if (k < dim) v = fci_excite_one(tab_a, tab_b, c, nb, npad, k / nb, k % nb, pq);
    D[(int64_t)pq * ld + kk] = v;
}

static int launch_excite(int layout, int norb, int64_t nb, int64_t dim, const int32_t *tab_a, const int32_t *tab_b,
                         const double *c, int64_t k0, int64_t nk, double *D, int64_t ld, hipStream_t st) {
    const int npad = fci_npad(norb);
    const unsigned grid = (unsigned)ceil_div(nk * npad, 256);
    if (layout == EVC_FCI_ORB_MAJOR) {
        fci_excite_orb_kernel<<<grid, 256, 0, st>>>(tab_a, tab_b, c, nb, dim, k0, nk, npad, D, ld);
        note_kernel(EVC_PROF_FCI_EXCITE, "fci_excite_orb_kernel");
    } else if (layout == EVC_FCI_DET_MAJOR_T) {
        fci_excite_det_kernel<1><<<grid, 256, 0, st>>>(tab_a, tab_b, c, norb, nb, dim, k0, nk, npad, D);
        note_kernel(EVC_PROF_FCI_EXCITE, "fci_excite_det_kernel<1>");
    } else {
        fci_excite_det_kernel<0><<<grid, 256, 0, st>>>(tab_a, tab_b, c, norb, nb, dim, k0, nk, npad, D);
        note_kernel(EVC_PROF_FCI_EXCITE, "fci_excite_det_kernel<0>");
    }
    EVC_LAUNCH_CHECK("fci_excite");
    return 0;
}

// ---- t-RDM product ---------------------------------------------------------------
// One workgroup per block of `rows` determinants: NBW x NBW waves, each with RT x RT tiles of the (npad, npad) product
// A^T B over the block's rows, A = D~_bra rows, B = D_ket rows (RT * RT * 8 accumulator registers a lane: 72 at twelve
// orbitals, where 3 x 3 waves hold 3 x 3 tiles each).  The waves of the first wave row also carry g1[rs] = sum_k bra[k] B[k][rs] on the B fragments they hold anyway (RT FP64 FMAs per RT*RT MFMAs), wave 0 the overlap.
// Partials: Pm[blk][npad][npad], Pg[blk][npad], Po[blk].
// blockIdx.z picks the bra r = r0 + z of a block call (evc_fci_trdm_rows_block): its D~ rows and its vector reach the
// kernel by value, its partials lie r * nblk blocks into Pm / Pg / Po, and B is shared.  What one (bra, ket, block)
// computes does not depend on the other bras of the launch.
constexpr int kTrdmBras = 16;
struct TrdmBras {
    const double *A[kTrdmBras];     // D~ of bra r: all its blocks (a_resident) or the blocks of this launch
    const double *c[kTrdmBras];     // the bra vectors
    int64_t row[kTrdmBras];         // first output row of bra r
};
template <int RT, int NBW>
__global__ __launch_bounds__(64 * NBW * NBW) void fci_trdm_kernel(
    TrdmBras bras, int r0, const double *__restrict__ B, const double *__restrict__ ket, int npad, int nq, int64_t rows,
    int64_t blk0, int64_t nblk, int64_t dim, int a_resident, double *__restrict__ Pm, double *__restrict__ Pg,
    double *__restrict__ Po) {
    const int br = r0 + (int)blockIdx.z;
    const double *__restrict__ A = bras.A[br];
    const double *__restrict__ bra = bras.c[br];
    Pm += (int64_t)br * nblk * npad * npad;
    Pg += (int64_t)br * nblk * npad;
    Po += (int64_t)br * nblk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int nt = npad / 16;
    // beyond RT * NBW tiles per edge the product is made in nq x nq quadrants, one per blockIdx.y
    const int wr = (int)(blockIdx.y / nq) * NBW + wave / NBW, wc = (int)(blockIdx.y % nq) * NBW + wave % NBW;
    const bool first = blockIdx.y == 0 && wave == 0;
    const int64_t blk = blk0 + blockIdx.x;
    A += (a_resident ? blk : (int64_t)blockIdx.x) * rows * npad;
    B += (int64_t)blockIdx.x * rows * npad;
    const int64_t kg0 = blk * rows;
    bool rok[RT], cok[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        rok[t] = wr * RT + t < nt;
        cok[t] = wc * RT + t < nt;
    }
    d4 acc[RT][RT];
    double g1[RT];
    double ov = 0.0;
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        g1[r] = 0.0;
#pragma unroll
        for (int c = 0; c < RT; ++c) acc[r][c] = (d4){0.0, 0.0, 0.0, 0.0};
    }
    const double *__restrict__ ap = A + (int64_t)l4 * npad + wr * RT * 16 + l15;
    const double *__restrict__ bp = B + (int64_t)l4 * npad + wc * RT * 16 + l15;
    const int64_t ksteps = rows / 4;
    for (int64_t ks = 0; ks < ksteps; ++ks) {
        double af[RT], bf[RT];
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            af[t] = rok[t] ? ap[ks * 4 * npad + t * 16] : 0.0;
            bf[t] = cok[t] ? bp[ks * 4 * npad + t * 16] : 0.0;
        }
        if (wr == 0) {
            const int64_t kg = kg0 + ks * 4 + l4;
            const double cb = kg < dim ? bra[kg] : 0.0;
#pragma unroll
            for (int t = 0; t < RT; ++t) g1[t] = fma(cb, bf[t], g1[t]);
            if (first) ov = fma(cb, kg < dim ? ket[kg] : 0.0, ov);
        }
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int c = 0; c < RT; ++c) acc[r][c] = mfma_f64(af[r], bf[c], acc[r][c]);
    }
    double *__restrict__ pm = Pm + blk * npad * npad;
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < RT; ++c)
            if (rok[r] && cok[c]) {
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    pm[(int64_t)((wr * RT + r) * 16 + l4 + 4 * v) * npad + (wc * RT + c) * 16 + l15] = acc[r][c][v];
            }
    if (wr == 0) {
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            double v = g1[t];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (cok[t] && l4 == 0) Pg[blk * npad + (wc * RT + t) * 16 + l15] = v;
        }
        if (first) {
            double v = ov;
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (lane == 0) Po[blk] = v;
        }
    }
}

// g1[pq] = sum over the blocks in order; dm1[q][p] = g1[p][q]; thread n2: the overlap.  blockIdx.y: bra r0 + y, whose
// results go to output row bras.row[r] + i (ket i).
__global__ __launch_bounds__(256) void fci_trdm_reduce1_kernel(TrdmBras bras, int r0, int64_t i,
                                                               const double *__restrict__ Pg,
                                                               const double *__restrict__ Po, int norb, int npad,
                                                               int64_t nblk, double *__restrict__ g1,
                                                               double *__restrict__ dm1, double *__restrict__ ovlp) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int n2 = norb * norb;
    if (t > n2) return;
    const int br = r0 + (int)blockIdx.y;
    const int64_t row = bras.row[br] + i;
    Pg += (int64_t)br * nblk * npad;
    Po += (int64_t)br * nblk;
    g1 += (int64_t)br * npad;
    dm1 += row * n2;
    ovlp += row;
    double s = 0.0;
    if (t == n2) {
        for (int64_t b = 0; b < nblk; ++b) s += Po[b];
        *ovlp = s;
        return;
    }
    for (int64_t b = 0; b < nblk; ++b) s += Pg[b * npad + t];
    g1[t] = s;
    dm1[(t % norb) * norb + t / norb] = s;
}

// dm2[p,q,r,s] = sum_blocks M[pq,rs] - delta_qr g1[p,s]; blockIdx.y: bra r0 + y.  dense: dm2 is the (rows, norb^4)
// output and the bra writes its row bras.row[r] + i; otherwise dm2 is one scratch block (the packed call, one bra).
__global__ __launch_bounds__(256) void fci_trdm_reduce2_kernel(TrdmBras bras, int r0, int64_t i, int dense,
                                                               const double *__restrict__ Pm,
                                                               const double *__restrict__ g1, int norb, int npad,
                                                               int64_t nblk, double *__restrict__ dm2) {
    const int n2 = norb * norb;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n2 * n2) return;
    const int br = r0 + (int)blockIdx.y;
    Pm += (int64_t)br * nblk * npad * npad;
    g1 += (int64_t)br * npad;
    if (dense) dm2 += (bras.row[br] + i) * ((int64_t)n2 * n2);
    const int pq = idx / n2, rs = idx - pq * n2;
    const double *__restrict__ src = Pm + (int64_t)pq * npad + rs;
    double m = 0.0;
    for (int64_t b = 0; b < nblk; ++b) m += src[b * npad * npad];
    const int p = pq / norb, q = pq % norb, r = rs / norb, s = rs % norb;
    dm2[idx] = q == r ? m - g1[p * norb + s] : m;
}

struct TrdmLaunch {
    const TrdmBras *bras;
    int r0, nz;                 // bras r0 ... r0 + nz - 1 (the grid's z)
    const double *B, *ket;
    int npad, nq;
    int64_t rows, blk0, nblocks, nblk, dim;
    int a_resident;
    double *Pm, *Pg, *Po;
};
template <int RT, int NBW>
static void launch_trdm_t(const TrdmLaunch &a, hipStream_t st) {
    fci_trdm_kernel<RT, NBW><<<dim3((unsigned)a.nblocks, a.nq * a.nq, a.nz), 64 * NBW * NBW, 0, st>>>(
        *a.bras, a.r0, a.B, a.ket, a.npad, a.nq, a.rows, a.blk0, a.nblk, a.dim, a.a_resident, a.Pm, a.Pg, a.Po);
}
// tiles per wave edge, waves per workgroup edge, quadrants per edge for nt tiles per edge
static void fci_trdm_config(int nt, int &rt, int &nbw, int &nq) {
    nq = 1;
    if (nt <= 4) rt = nt, nbw = 1;
    else if (nt <= 6) rt = 3, nbw = 2;
    else if (nt <= 8) rt = 4, nbw = 2;
    else if (nt == 9) rt = 3, nbw = 3;
    else if (nt <= 12) rt = 3, nbw = 2, nq = 2;
    else rt = 4, nbw = 2, nq = 2;
}
static void launch_trdm(int rt, int nbw, const TrdmLaunch &a, hipStream_t st) {
    switch (rt * 10 + nbw) {
        case 11: launch_trdm_t<1, 1>(a, st); break;
        case 21: launch_trdm_t<2, 1>(a, st); break;
        case 31: launch_trdm_t<3, 1>(a, st); break;
        case 41: launch_trdm_t<4, 1>(a, st); break;
        case 32: launch_trdm_t<3, 2>(a, st); break;
        case 42: launch_trdm_t<4, 2>(a, st); break;
        default: launch_trdm_t<3, 3>(a, st); break;
    }
}

// ---- sigma -----------------------------------------------------------------------
// hp[pq] = h1[pq] - 1/2 sum_r (pr|rq); h2T[rs * npad + pq] = h2[pq][rs], zero padded
__global__ __launch_bounds__(256) void fci_sigma_prep_kernel(const double *__restrict__ h1,
                                                             const double *__restrict__ h2, int norb, int npad,
                                                             double *__restrict__ hp, double *__restrict__ h2T) {
    const int n2 = norb * norb;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= npad * npad) return;
    const int rs = idx / npad, pq = idx - rs * npad;
    h2T[idx] = (rs < n2 && pq < n2) ? h2[(int64_t)pq * n2 + rs] : 0.0;
    if (rs == 0) {
        double v = 0.0;
        if (pq < n2) {
            const int p = pq / norb, q = pq % norb;
            double s = 0.0;
            for (int r = 0; r < norb; ++r) s += h2[(((int64_t)p * norb + r) * norb + r) * norb + q];
            v = h1[pq] - 0.5 * s;
        }
        hp[pq] = v;
    }
}

// G[pq][k0 + k] = sum_rs h2T[rs][pq] D[rs][k]: a wave owns RT row tiles x 4 determinant tiles; consecutive waves share
// the determinant tiles (their D fragments meet in the cache).
template <int RT>
__global__ __launch_bounds__(256) void fci_sigma_gemm_kernel(const double *__restrict__ h2T,
                                                             const double *__restrict__ D, int64_t ldd, int npad,
                                                             int nbw, int64_t njb, double *__restrict__ G, int64_t ldg) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int nt = npad / 16;
    const int64_t gw = (int64_t)blockIdx.x * 4 + wave;
    const int rb = (int)(gw % nbw);
    const int64_t jb = gw / nbw;
    if (jb >= njb) return;
    bool rok[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) rok[t] = rb * RT + t < nt;
    d4 acc[RT][4];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = (d4){0.0, 0.0, 0.0, 0.0};
    const double *__restrict__ ap = h2T + (int64_t)l4 * npad + rb * RT * 16 + l15;
    const double *__restrict__ bp = D + (int64_t)l4 * ldd + jb * 64 + l15;
    for (int ks = 0; ks < npad / 4; ++ks) {
        double af[RT], bf[4];
#pragma unroll
        for (int t = 0; t < RT; ++t) af[t] = rok[t] ? ap[(int64_t)ks * 4 * npad + t * 16] : 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) bf[t] = bp[(int64_t)ks * 4 * ldd + t * 16];
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = mfma_f64(af[r], bf[c], acc[r][c]);
    }
#pragma unroll
    for (int r = 0; r < RT; ++r)
        if (rok[r]) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    G[(int64_t)((rb * RT + r) * 16 + l4 + 4 * v) * ldg + jb * 64 + c * 16 + l15] = acc[r][c][v];
        }
}

template <int RT>
static void launch_sigma_gemm_t(const double *h2T, const double *D, int64_t ldd, int npad, int nbw, int64_t njb,
                                double *G, int64_t ldg, hipStream_t st) {
    fci_sigma_gemm_kernel<RT><<<(unsigned)ceil_div(njb * nbw, 4), 256, 0, st>>>(h2T, D, ldd, npad, nbw, njb, G, ldg);
}

// sigma(I) = sum_pq [ sa X_pq(Ja,Ib) + sb X_pq(Ia,Jb) ],  X_pq = G[pq]/2 + h'_pq c; one thread per determinant, pq in
// order
__global__ __launch_bounds__(256) void fci_sigma_gather_kernel(const int32_t *__restrict__ tab_a,
                                                               const int32_t *__restrict__ tab_b,
                                                               const double *__restrict__ c,
                                                               const double *__restrict__ G, int64_t ldg,
                                                               const double *__restrict__ hp, int norb, int npad,
                                                               int64_t nb, int64_t dim, double *__restrict__ sigma) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= dim) return;
    const int64_t ia = k / nb, ib = k % nb;
    const int n2 = norb * norb;
    double s = 0.0;
    for (int pq = 0; pq < n2; ++pq) {
        const int32_t ta = tab_a[ia * npad + pq], tb = tab_b[ib * npad + pq];
        const double h = hp[pq];
        if (ta != 0) {
            const int64_t j = (int64_t)(abs(ta) - 1) * nb + ib;
            const double x = 0.5 * G[(int64_t)pq * ldg + j] + h * c[j];
            s += ta > 0 ? x : -x;
        }
        if (tb != 0) {
            const int64_t j = ia * nb + (abs(tb) - 1);
            const double x = 0.5 * G[(int64_t)pq * ldg + j] + h * c[j];
            s += tb > 0 ? x : -x;
        }
    }
    sigma[k] = s;
}

// ---- workspace layouts ------------------------------------------------------------
struct FciShape {
    int norb, npad, nt, rt, nbw;
    int64_t na, nb, dim, rows, nblk, ldg;
    size_t trdm_fixed, trdm_block, sigma_fixed, sigma_col;   // bytes
};
static int fci_shape(const char *who, int norb, int64_t na, int64_t nb, FciShape &s) {
    EVC_REQUIRE(norb >= 1 && norb <= kFciMaxOrb, "%s: norb=%d, supported 1 ... %d", who, norb, kFciMaxOrb);
    EVC_REQUIRE(na >= 1 && nb >= 1 && na <= 12870 && nb <= 12870, "%s: na=%lld nb=%lld strings (1 ... 12870 each)", who,
                (long long)na, (long long)nb);
    s.norb = norb;
    s.npad = fci_npad(norb);
    s.nt = s.npad / 16;
    s.rt = fci_rt(s.nt);
    s.nbw = (int)ceil_div(s.nt, s.rt);
    s.na = na;
    s.nb = nb;
    s.dim = na * nb;
    s.rows = fci_rows_per_block(s.dim);
    s.nblk = ceil_div(s.dim, s.rows);
    s.ldg = (int64_t)align_up((size_t)s.dim, 64);
    // t-RDM: Pm, Pg, Po, g1 | D~_bra blocks | D_ket blocks
    s.trdm_fixed = align_up(((size_t)s.nblk * ((size_t)s.npad * s.npad + s.npad + 1) + s.npad) * 8, 256);
    s.trdm_block = (size_t)s.rows * s.npad * 8;
    // sigma: h2T, hp | G (npad, ldg) | D chunk (npad, columns)
    s.sigma_fixed = align_up(((size_t)s.npad * s.npad + s.npad) * 8, 256) + (size_t)s.npad * s.ldg * 8;
    s.sigma_col = (size_t)s.npad * 8;
    return 0;
}
// the partials and g1 of nbras bras: Pm[r][blk], Pg[r][blk], Po[r][blk], g1[r]; one bra: trdm_fixed
static size_t fci_trdm_fixed_bytes(const FciShape &s, int nbras) {
    return align_up((size_t)nbras * ((size_t)s.nblk * ((size_t)s.npad * s.npad + s.npad + 1) + s.npad) * 8, 256);
}
// the least t-RDM workspace of nbras bras: one block of D~ per bra and one of D_ket
static size_t fci_trdm_need_bytes(const FciShape &s, int nbras) {
    return fci_trdm_fixed_bytes(s, nbras) + (size_t)(nbras + 1) * s.trdm_block;
}

}  // namespace evc

using namespace evc;

extern "C" size_t evc_fci_rows_block_workspace_bytes(int norb, int64_t na, int64_t nb, int nbras, int minimal) {
    FciShape s;
    if (nbras < 1 || nbras > kTrdmBras) return 0;
    if (fci_shape("evc_fci_rows_block_workspace_bytes", norb, na, nb, s)) return 0;
    const size_t t = minimal ? fci_trdm_need_bytes(s, nbras)
                             : fci_trdm_fixed_bytes(s, nbras) + s.trdm_block * (size_t)((nbras + 1) * s.nblk);
    const size_t g = s.sigma_fixed + s.sigma_col * (size_t)(minimal ? 64 : s.ldg);
    return t > g ? t : g;
}

extern "C" size_t evc_fci_workspace_bytes(int norb, int64_t na, int64_t nb, int minimal) {
    FciShape s;
    if (fci_shape("evc_fci_workspace_bytes", norb, na, nb, s)) return 0;
    const size_t t = s.trdm_fixed + s.trdm_block * (size_t)(minimal ? 2 : 2 * s.nblk);
    const size_t g = s.sigma_fixed + s.sigma_col * (size_t)(minimal ? 64 : s.ldg);
    return t > g ? t : g;
}

extern "C" int evc_fci_excite(int norb, int64_t na, int64_t nb, const int32_t *tab_a, const int32_t *tab_b,
                              const double *c, int64_t k0, int64_t nk, int layout, double *D, int64_t ld,
                              void *stream) {
    FciShape s;
    if (int rc = fci_shape("evc_fci_excite", norb, na, nb, s)) return rc;
    EVC_REQUIRE(tab_a && tab_b && c && D, "evc_fci_excite: null pointer");
    EVC_REQUIRE(layout == EVC_FCI_DET_MAJOR || layout == EVC_FCI_DET_MAJOR_T || layout == EVC_FCI_ORB_MAJOR,
                "evc_fci_excite: layout=%d", layout);
    EVC_REQUIRE(k0 >= 0 && nk >= 1 && nk * s.npad < ((int64_t)1 << 38), "evc_fci_excite: k0=%lld nk=%lld", (long long)k0,
                (long long)nk);
    EVC_REQUIRE(layout == EVC_FCI_ORB_MAJOR ? ld >= nk : ld == s.npad, "evc_fci_excite: ld=%lld (layout %d, nk=%lld)",
                (long long)ld, layout, (long long)nk);
    return launch_excite(layout, norb, nb, s.dim, tab_a, tab_b, c, k0, nk, D, ld, as_stream(stream));
}

// The row call behind evc_fci_trdm_rows, evc_fci_trdm_rows_packed (one bra) and evc_fci_trdm_rows_block: bra r against
// kets[0 .. nkets_of[r] - 1] (counts non-decreasing, so the bras that see ket i are r0(i) ... nbras - 1), the determinant
// blocks in order, then the two reductions per ket.  The ket-side D of a chunk is formed once and read by every bra of
// the launch (the grid's z); what a (bra, ket) pair computes is what it computes alone.  Results go to the consecutive
// ragged rows off_r + i.  `dm2` (rows, norb^4): the dense two-body results; NULL (one bra): fci_trdm_reduce2_kernel writes
// each ket's dense block into `slot` (norb^4 doubles) and fci_row_pack_kernel (fci_pack.hip) packs it into row i of
// `rows` (pitch ld) in `layout`.  ws / ws_bytes: the t-RDM workspace alone (at least fci_trdm_need_bytes(s, nbras)).
// note_bras: 0, or nbras for the block call's record.
static int fci_trdm_rows_run(const FciShape &s, const int32_t *tab_a, const int32_t *tab_b, const double *const *bras,
                             int nbras, const double *const *kets, const int *nkets_of, int note_bras, double *ovlp,
                             double *dm1, double *dm2, double *slot, int layout, double *rows, int64_t ld, void *ws,
                             size_t ws_bytes, hipStream_t st) {
    const int norb = s.norb;
    const int64_t nb = s.nb;
    const int64_t nfit = (int64_t)((ws_bytes - fci_trdm_fixed_bytes(s, nbras)) / s.trdm_block);
    const bool resident = nfit >= nbras * s.nblk + 1;   // D~ of every bra whole: formed once for all the kets
    const int64_t cb = resident ? (nfit - nbras * s.nblk < s.nblk ? nfit - nbras * s.nblk : s.nblk) : nfit / (nbras + 1);
    const int64_t bra_blocks = resident ? s.nblk : cb;  // blocks of D~ each bra holds
    double *Pm = static_cast<double *>(ws);
    double *Pg = Pm + nbras * s.nblk * s.npad * s.npad;
    double *Po = Pg + nbras * s.nblk * s.npad;
    double *g1 = Po + nbras * s.nblk;
    double *Dbra = reinterpret_cast<double *>(static_cast<char *>(ws) + fci_trdm_fixed_bytes(s, nbras));
    double *Dket = Dbra + nbras * bra_blocks * s.rows * s.npad;
    const int n2 = norb * norb;
    int trt, tnbw, nq;
    fci_trdm_config(s.nt, trt, tnbw, nq);
    TrdmBras tb = {};
    for (int r = 0; r < nbras; ++r) {
        tb.A[r] = Dbra + r * bra_blocks * s.rows * s.npad;
        tb.c[r] = bras[r];
        tb.row[r] = r ? tb.row[r - 1] + nkets_of[r - 1] : 0;
    }
    if (resident)
        for (int r = 0; r < nbras; ++r)
            if (int rc = launch_excite(EVC_FCI_DET_MAJOR_T, norb, nb, s.dim, tab_a, tab_b, bras[r], 0, s.nblk * s.rows,
                                       const_cast<double *>(tb.A[r]), s.npad, st))
                return rc;
    int r0 = 0;
    for (int i = 0; i < nkets_of[nbras - 1]; ++i) {
        while (nkets_of[r0] <= i) ++r0;
        const int nz = nbras - r0;
        for (int64_t b0 = 0; b0 < s.nblk; b0 += cb) {
            const int64_t nbk = s.nblk - b0 < cb ? s.nblk - b0 : cb;
            if (!resident)
                for (int r = r0; r < nbras; ++r)
                    if (int rc = launch_excite(EVC_FCI_DET_MAJOR_T, norb, nb, s.dim, tab_a, tab_b, bras[r], b0 * s.rows,
                                               nbk * s.rows, const_cast<double *>(tb.A[r]), s.npad, st))
                        return rc;
            if (int rc = launch_excite(EVC_FCI_DET_MAJOR, norb, nb, s.dim, tab_a, tab_b, kets[i], b0 * s.rows,
                                       nbk * s.rows, Dket, s.npad, st))
                return rc;
            const TrdmLaunch a = {&tb, r0, nz, Dket, kets[i], s.npad, nq, s.rows, b0, nbk, s.nblk, s.dim, resident ? 1 : 0,
                                  Pm, Pg, Po};
            launch_trdm(trt, tnbw, a, st);
            EVC_LAUNCH_CHECK("fci_trdm_kernel");
        }
        fci_trdm_reduce1_kernel<<<dim3((unsigned)ceil_div(n2 + 1, 256), nz), 256, 0, st>>>(
            tb, r0, i, Pg, Po, norb, s.npad, s.nblk, g1, dm1, ovlp);
        EVC_LAUNCH_CHECK("fci_trdm_reduce1_kernel");
        fci_trdm_reduce2_kernel<<<dim3((unsigned)ceil_div((int64_t)n2 * n2, 256), nz), 256, 0, st>>>(
            tb, r0, i, dm2 ? 1 : 0, Pm, g1, norb, s.npad, s.nblk, dm2 ? dm2 : slot);
        EVC_LAUNCH_CHECK("fci_trdm_reduce2_kernel");
        if (!dm2)
            if (int rc = launch_fci_row_pack(layout, norb, slot, rows + (int64_t)i * ld, ld, st)) return rc;
    }
    if (note_bras)
        note_kernel(EVC_PROF_FCI_TRDM,
                    "fci_trdm_kernel<%d,%d> quadrants=%d blocks=%lld bra_resident=%d ket_blocks=%lld bras=%d", trt, tnbw,
                    nq * nq, (long long)s.nblk, resident ? 1 : 0, (long long)cb, note_bras);
    else
        note_kernel(EVC_PROF_FCI_TRDM, "fci_trdm_kernel<%d,%d> quadrants=%d blocks=%lld bra_resident=%d ket_blocks=%lld",
                    trt, tnbw, nq * nq, (long long)s.nblk, resident ? 1 : 0, (long long)cb);
    return 0;
}

extern "C" int evc_fci_trdm_rows(int norb, int64_t na, int64_t nb, const int32_t *tab_a, const int32_t *tab_b,
                                 const double *bra, const double *const *kets, int nkets, double *ovlp, double *dm1,
                                 double *dm2, void *ws, size_t ws_bytes, void *stream) {
    FciShape s;
    if (int rc = fci_shape("evc_fci_trdm_rows", norb, na, nb, s)) return rc;
    EVC_REQUIRE(tab_a && tab_b && bra && kets && ovlp && dm1 && dm2 && ws, "evc_fci_trdm_rows: null pointer");
    EVC_REQUIRE(nkets >= 1 && nkets <= 4096, "evc_fci_trdm_rows: nkets=%d (1 ... 4096)", nkets);
    for (int i = 0; i < nkets; ++i) EVC_REQUIRE(kets[i], "evc_fci_trdm_rows: kets[%d] is null", i);
    EVC_REQUIRE(aligned16(ws), "evc_fci_trdm_rows: workspace not 16-byte aligned");
    const size_t need = s.trdm_fixed + 2 * s.trdm_block;
    EVC_REQUIRE(ws_bytes >= need, "evc_fci_trdm_rows: workspace of %zu bytes, at least %zu needed for %lld determinants",
                ws_bytes, need, (long long)s.dim);
    clear_fci_kernels(EVC_PROF_FCI_TRDM);
    return fci_trdm_rows_run(s, tab_a, tab_b, &bra, 1, kets, &nkets, 0, ovlp, dm1, dm2, nullptr, 0, nullptr, 0, ws,
                             ws_bytes, as_stream(stream));
}

// [a, a + na) and [b, b + nb) share a byte
static bool fci_overlaps(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

extern "C" int evc_fci_trdm_rows_block(int norb, int64_t na, int64_t nb, const int32_t *tab_a, const int32_t *tab_b,
                                       const double *const *bras, int nbras, const double *const *kets,
                                       const int *nkets_of, double *ovlp, double *dm1, double *dm2, void *ws,
                                       size_t ws_bytes, void *stream) {
    FciShape s;
    if (int rc = fci_shape("evc_fci_trdm_rows_block", norb, na, nb, s)) return rc;
    EVC_REQUIRE(tab_a && tab_b && bras && kets && nkets_of && ovlp && dm1 && dm2 && ws,
                "evc_fci_trdm_rows_block: null pointer");
    EVC_REQUIRE(nbras >= 1 && nbras <= kTrdmBras, "evc_fci_trdm_rows_block: nbras=%d (1 ... %d)", nbras, kTrdmBras);
    int64_t total = 0;
    for (int r = 0; r < nbras; ++r) {
        EVC_REQUIRE(bras[r], "evc_fci_trdm_rows_block: bras[%d] is null", r);
        EVC_REQUIRE(nkets_of[r] >= 1 && nkets_of[r] <= 4096, "evc_fci_trdm_rows_block: nkets_of[%d]=%d (1 ... 4096)", r,
                    nkets_of[r]);
        EVC_REQUIRE(r == 0 || nkets_of[r] >= nkets_of[r - 1],
                    "evc_fci_trdm_rows_block: nkets_of[%d]=%d below nkets_of[%d]=%d (counts must not decrease)", r,
                    nkets_of[r], r - 1, nkets_of[r - 1]);
        total += nkets_of[r];
    }
    const int nkets = nkets_of[nbras - 1];
    for (int i = 0; i < nkets; ++i) EVC_REQUIRE(kets[i], "evc_fci_trdm_rows_block: kets[%d] is null", i);
    EVC_REQUIRE(aligned16(ws), "evc_fci_trdm_rows_block: workspace not 16-byte aligned");
    const size_t need = fci_trdm_need_bytes(s, nbras);
    EVC_REQUIRE(ws_bytes >= need,
                "evc_fci_trdm_rows_block: workspace of %zu bytes, at least %zu needed for %lld determinants and %d bras",
                ws_bytes, need, (long long)s.dim, nbras);
    const size_t n2 = (size_t)norb * norb, vec = (size_t)s.dim * 8;
    const struct { const void *p; size_t n; const char *name; } outs[3] = {
        {ovlp, (size_t)total * 8, "ovlp"}, {dm1, (size_t)total * n2 * 8, "dm1"}, {dm2, (size_t)total * n2 * n2 * 8, "dm2"}};
    for (const auto &o : outs) {
        for (int r = 0; r < nbras; ++r)
            EVC_REQUIRE(!fci_overlaps(o.p, o.n, bras[r], vec), "evc_fci_trdm_rows_block: %s overlaps bras[%d]", o.name, r);
        for (int i = 0; i < nkets; ++i)
            EVC_REQUIRE(!fci_overlaps(o.p, o.n, kets[i], vec), "evc_fci_trdm_rows_block: %s overlaps kets[%d]", o.name, i);
    }
    clear_fci_kernels(EVC_PROF_FCI_TRDM);
    return fci_trdm_rows_run(s, tab_a, tab_b, bras, nbras, kets, nkets_of, nbras, ovlp, dm1, dm2, nullptr, 0, nullptr, 0,
                             ws, ws_bytes, as_stream(stream));
}

// the scratch slot of the packed row call: one dense dm2 block, in front of the t-RDM workspace
static size_t fci_pack_slot_bytes(int norb) { return align_up((size_t)norb * norb * norb * norb * 8, 256); }

extern "C" size_t evc_fci_rows_packed_workspace_bytes(int norb, int64_t na, int64_t nb, int minimal) {
    const size_t base = evc_fci_workspace_bytes(norb, na, nb, minimal);
    return base ? base + fci_pack_slot_bytes(norb) : 0;
}

extern "C" int evc_fci_trdm_rows_packed(int norb, int64_t na, int64_t nb, const int32_t *tab_a, const int32_t *tab_b,
                                        const double *bra, const double *const *kets, int nkets, double *ovlp,
                                        double *dm1, int layout, double *rows, int64_t ld, void *ws, size_t ws_bytes,
                                        void *stream) {
    FciShape s;
    if (int rc = fci_shape("evc_fci_trdm_rows_packed", norb, na, nb, s)) return rc;
    EVC_REQUIRE(tab_a && tab_b && bra && kets && ovlp && dm1 && rows && ws, "evc_fci_trdm_rows_packed: null pointer");
    EVC_REQUIRE(nkets >= 1 && nkets <= 4096, "evc_fci_trdm_rows_packed: nkets=%d (1 ... 4096)", nkets);
    for (int i = 0; i < nkets; ++i) EVC_REQUIRE(kets[i], "evc_fci_trdm_rows_packed: kets[%d] is null", i);
    EVC_REQUIRE(layout == EVC_LAYOUT_PACK2 || layout == EVC_LAYOUT_SYM8,
                "evc_fci_trdm_rows_packed: layout=%d (EVC_LAYOUT_PACK2 or EVC_LAYOUT_SYM8)", layout);
    const int64_t cols = fci_row_pack_cols(layout, norb);
    EVC_REQUIRE(ld >= (cols + 15) / 16 * 16 && ld % 16 == 0 && ld < ((int64_t)1 << 31),
                "evc_fci_trdm_rows_packed: ld=%lld (a multiple of 16, at least %lld columns rounded up to 16, below 2^31)",
                (long long)ld, (long long)cols);
    EVC_REQUIRE(aligned16(ws) && aligned16(rows), "evc_fci_trdm_rows_packed: workspace or rows not 16-byte aligned");
    const size_t slot = fci_pack_slot_bytes(norb), need = slot + s.trdm_fixed + 2 * s.trdm_block;
    EVC_REQUIRE(ws_bytes >= need,
                "evc_fci_trdm_rows_packed: workspace of %zu bytes, at least %zu needed for %lld determinants", ws_bytes,
                need, (long long)s.dim);
    clear_fci_kernels(EVC_PROF_FCI_TRDM);
    clear_fci_kernels(EVC_PROF_FCI_PACK);
    if (int rc = fci_trdm_rows_run(s, tab_a, tab_b, &bra, 1, kets, &nkets, 0, ovlp, dm1, nullptr,
                                   static_cast<double *>(ws), layout, rows, ld, static_cast<char *>(ws) + slot,
                                   ws_bytes - slot, as_stream(stream)))
        return rc;
    note_fci_row_pack(layout, norb, nkets, ld);
    return 0;
}

extern "C" int evc_fci_sigma(int norb, int64_t na, int64_t nb, const int32_t *tab_a, const int32_t *tab_b,
                             const double *h1, const double *h2, const double *c, double *sigma, void *ws,
                             size_t ws_bytes, void *stream) {
    FciShape s;
    if (int rc = fci_shape("evc_fci_sigma", norb, na, nb, s)) return rc;
    EVC_REQUIRE(tab_a && tab_b && h1 && h2 && c && sigma && ws, "evc_fci_sigma: null pointer");
    EVC_REQUIRE(c != sigma, "evc_fci_sigma: sigma must not alias c");
    EVC_REQUIRE(aligned16(ws), "evc_fci_sigma: workspace not 16-byte aligned");
    const size_t need = s.sigma_fixed + 64 * s.sigma_col;
    EVC_REQUIRE(ws_bytes >= need, "evc_fci_sigma: workspace of %zu bytes, at least %zu needed for %lld determinants",
                ws_bytes, need, (long long)s.dim);
    hipStream_t st = as_stream(stream);
    clear_fci_kernels(EVC_PROF_FCI_SIGMA);
    int64_t cols = (int64_t)((ws_bytes - s.sigma_fixed) / s.sigma_col) / 64 * 64;
    if (cols > s.ldg) cols = s.ldg;
    double *h2T = static_cast<double *>(ws);
    double *hp = h2T + (int64_t)s.npad * s.npad;
    double *G = reinterpret_cast<double *>(static_cast<char *>(ws) + align_up(((size_t)s.npad * s.npad + s.npad) * 8, 256));
    double *D = G + (int64_t)s.npad * s.ldg;
    fci_sigma_prep_kernel<<<(unsigned)ceil_div(s.npad * s.npad, 256), 256, 0, st>>>(h1, h2, norb, s.npad, hp, h2T);
    EVC_LAUNCH_CHECK("fci_sigma_prep_kernel");
    for (int64_t k0 = 0; k0 < s.ldg; k0 += cols) {
        const int64_t nk = s.ldg - k0 < cols ? s.ldg - k0 : cols;   // a multiple of 64
        if (int rc = launch_excite(EVC_FCI_ORB_MAJOR, norb, nb, s.dim, tab_a, tab_b, c, k0, nk, D, cols, st)) return rc;
        switch (s.rt) {
            case 1: launch_sigma_gemm_t<1>(h2T, D, cols, s.npad, s.nbw, nk / 64, G + k0, s.ldg, st); break;
            case 2: launch_sigma_gemm_t<2>(h2T, D, cols, s.npad, s.nbw, nk / 64, G + k0, s.ldg, st); break;
            case 3: launch_sigma_gemm_t<3>(h2T, D, cols, s.npad, s.nbw, nk / 64, G + k0, s.ldg, st); break;
            default: launch_sigma_gemm_t<4>(h2T, D, cols, s.npad, s.nbw, nk / 64, G + k0, s.ldg, st); break;
        }
        EVC_LAUNCH_CHECK("fci_sigma_gemm_kernel");
    }
    fci_sigma_gather_kernel<<<(unsigned)ceil_div(s.dim, 256), 256, 0, st>>>(tab_a, tab_b, c, G, s.ldg, hp, norb, s.npad,
                                                                            nb, s.dim, sigma);
    EVC_LAUNCH_CHECK("fci_sigma_gather_kernel");
    note_kernel(EVC_PROF_FCI_SIGMA, "fci_sigma_gemm_kernel<%d> chunk=%lld + fci_sigma_gather_kernel", s.rt,
                (long long)cols);
    return 0;
}
