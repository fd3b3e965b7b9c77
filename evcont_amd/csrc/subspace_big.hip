// K6 for LARGE training sets (T > 32): the subspace generalised eigenproblem H c = E S c of
// ab_initio_eigenvector_continuation.py:73-88 / :157-173 with LAPACK dsygvd semantics (lower triangles,
// Cholesky of S, c^T S c = 1) and the row weights of ab_initio_gradients_loewdin.py:343-356, for training sets the
// register / 32 x 32-tile kernel of subspace_small.hip cannot hold.  The reference puts no bound on T (its Zundel
// learning curve evaluates 80 and 100 training states, scripts/MD/Zundel_thermodynamics/continuation/
// 05_Zundel_test_potential_energy.py:182-210; converge_EVCont_MD grows T without bound, MD_utils.py:128-502).
//
// One workgroup of 1024 threads (16 waves) per problem.  ONE T x T matrix lives in LDS at a time (128 KB at T = 128):
//   (a) [only when the cached factor does not match] L = chol(S) right-looking in LDS, inverted in place, B = L^-1
//       written to global memory (the per-workspace cache: S_train does not depend on the geometry);
//   (b) H assembled from the span partials in LDS, symmetrised from its lower triangle;
//   (c) W = B Hs and C = W B^T as "row . row" products on the FP64 matrix cores (16 x 16 tiles dealt to the 16 waves,
//       operands read with 16-byte loads from L2-resident global scratch / LDS);
//   (d) nroots <= 4 (the energy + force path asks for ONE root): Householder tridiagonalisation in LDS, Sturm multisection,
//       twisted factorisation, back-transformation through the reflectors, and a residual / orthogonality check in the
//       original matrix (big_few_roots.hpp); otherwise, or when that check fails: eigen-decomposition of C + sigma I (sigma:
//       Gershgorin bound, makes it positive definite) by one-sided (Hestenes) Jacobi on its columns in LDS: 16 lanes per
//       column pair, 16-byte conflict-free LDS rows, the three dot products reduced over a DPP row, one barrier per
//       round-robin step; at convergence column j is (lambda_j + sigma) v_j, so no eigenvector matrix is carried through
//       the rotations (big_jacobi, big_block.hpp);
//   (e) ascending order, back-transformation c = B^T y, weights.
// With EVC_FLAG_WARM_START the Jacobi sweeps start from G0 = (C + sigma I) V_prev (V_prev checked for orthonormality).
// The same code runs with the matrix in global memory (template parameter) for T beyond what LDS holds (Jacobi route).
// (The Loewdin orthogonalisation beyond 32 orbitals runs on the same Jacobi: loewdin_big.hip.)
#include <stdlib.h>

#include "big_block.hpp"
#include "big_few_roots.hpp"
#include "common.hpp"
#include "kernels.hpp"

namespace evc {

// In-place Cholesky factor of the lower triangle in M (pitch Tp) followed by its in-place inverse: on return the lower
// triangle of M holds B = L^-1.  A matrix that is not positive definite yields NaNs.  dinv, tmp: T doubles each.
__device__ __forceinline__ void big_chol_inverse(double *M, int T, int Tp, double *dinv, double *tmp) {
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    for (int j = 0; j < T; ++j) {
        const double d = M[(size_t)j * Tp + j];
        double rs = __builtin_amdgcn_rsq(d);
        rs = rs * fma(-0.5 * d * rs, rs, 1.5);
        rs = rs * fma(-0.5 * d * rs, rs, 1.5);
        if (tid == 0) dinv[j] = rs;   // 1 / L_jj (the diagonal itself is fixed up below)
        for (int i = j + 1 + tid; i < T; i += kBT) M[(size_t)i * Tp + j] *= rs;
        __syncthreads();
        for (int i = j + 1 + ty; i < T; i += 32) {
            const double lij = M[(size_t)i * Tp + j];
            for (int k = j + 1 + tx; k <= i; k += 32) M[(size_t)i * Tp + k] = fma(-lij, M[(size_t)k * Tp + j], M[(size_t)i * Tp + k]);
        }
        __syncthreads();
    }
    // inverse, column by column from the last: new column j below the diagonal = -(L22^-1 c) / L_jj
    const int l8 = tid & 7, r8 = tid >> 3;
    for (int j = T - 1; j >= 0; --j) {
        for (int i = j + 1 + r8; i < T; i += kBT / 8) {   // (the eight lanes of a group share i)
            double t = 0.0;
            for (int k = j + 1 + l8; k <= i; k += 8) t = fma(M[(size_t)i * Tp + k], M[(size_t)k * Tp + j], t);
            t = sum8(t);
            if (l8 == 0) tmp[i] = t;
        }
        __syncthreads();
        const double ajj = dinv[j];
        for (int i = j + 1 + tid; i < T; i += kBT) M[(size_t)i * Tp + j] = -tmp[i] * ajj;
        if (tid == 0) M[(size_t)j * Tp + j] = ajj;
        __syncthreads();
    }
}

template <bool kLds>
__global__ __launch_bounds__(kBT) void subspace_big_kernel(SolveArgs a) {
    extern __shared__ __align__(16) double sm[];
    {
        const int64_t g = blockIdx.x;
        a.h1part += g * a.sh1;
        if (a.h2part) a.h2part += g * a.sh2;
        a.S += g * a.sS;
        a.evals += g * a.sev;
        a.evecs += g * a.svec;
        if (a.Hout) a.Hout += g * a.sH;
        if (a.w1) a.w1 += g * a.sw;
        if (a.w2) a.w2 += g * a.sw;
        if (a.w2t) a.w2t += (g - g % kMaxBatchG) * a.sw;
        if (a.w1t) a.w1t += (g - g % kMaxBatchG) * a.sw;
        if (a.vstd) a.vstd += g * a.sw;
        if (a.bcache) a.bcache += g * a.sw;
        a.scratch += g * a.sscratch;
        if (a.e_shift_dev) a.e_shift = a.e_shift_dev[g];
    }
    const int T = a.T, m = (T + 1) & ~1, Tp = (T + 15) & ~15, Pj = (m + 31) & ~31;
    const size_t Tp2 = (size_t)Tp * Tp;
    const size_t msz = (size_t)m * Pj > Tp2 ? (size_t)m * Pj : Tp2;
    // global scratch: [B (when there is no cache) | W | C | the matrix itself when it does not fit LDS]
    double *Bg = a.bcache ? a.bcache + Tp2 : a.scratch;
    double *Wg = a.scratch + Tp2, *Cg = a.scratch + 2 * Tp2;
    double *M = kLds ? sm : a.scratch + 3 * Tp2;
    double *aux = kLds ? sm + msz : sm;
    double *ev = aux, *tmp = ev + Tp, *c0 = tmp + Tp, *dinv = c0 + Tp, *red = dinv + Tp;
    int *order = reinterpret_cast<int *>(red + 2 * kBW);
    BigFew fw;   // (the Householder work vectors share the buffers of the phases that are over / not yet reached)
    fw.d = ev;
    fw.vv = tmp;
    fw.pv = dinv;
    fw.ww = c0;
    fw.e = reinterpret_cast<double *>(order + Tp + (Tp & 1));
    fw.tau = fw.e + Tp;
    fw.dp = fw.tau + Tp;
    fw.dm = fw.dp + (size_t)kFewRoots * Tp;
    fw.Y = fw.dm + (size_t)kFewRoots * Tp;
    fw.iv = fw.Y + (size_t)kFewRoots * Tp;
    fw.lam = fw.iv + 2 * kFewRoots + 4;
    fw.cnt = reinterpret_cast<unsigned short *>(fw.lam + kFewRoots);
    const int tid = threadIdx.x;
    const int64_t P = (int64_t)T * (T + 1) / 2;
    const bool pairs = (a.layout == EVC_LAYOUT_PAIR5 || a.layout == EVC_LAYOUT_PACK2 || a.layout == EVC_LAYOUT_SYM8);
    const int64_t rows2 = pairs ? P : (int64_t)T * T;

    EVC_BSTAMP(0);
    // (a) B = L^-1: from the cache when the overlap matrix it was computed from is bit-identical to this call's
    bool hit = false;
    if (a.bcache) {
        bool diff = false;
        for (int idx = tid; idx < T * T; idx += kBT) {
            const int i = idx / T, j = idx - i * T;
            if (i >= j) diff = diff || !(a.bcache[idx] == a.S[idx]);
        }
        hit = !big_block_any(diff, red);
    }
    if (!hit) {   // uniform
        for (size_t idx = tid; idx < Tp2; idx += kBT) {
            const int i = (int)(idx / Tp), j = (int)(idx - (size_t)i * Tp);
            M[idx] = (i < T && j <= i) ? a.S[(size_t)i * T + j] : 0.0;
        }
        __syncthreads();
        big_chol_inverse(M, T, Tp, dinv, tmp);
        for (size_t idx = tid; idx < Tp2; idx += kBT) {
            const int i = (int)(idx / Tp), j = (int)(idx - (size_t)i * Tp);
            Bg[idx] = (i < T && j <= i) ? M[idx] : 0.0;
        }
        if (a.bcache)
            for (int idx = tid; idx < T * T; idx += kBT) a.bcache[idx] = a.S[idx];
        __syncthreads();
    }
    EVC_BSTAMP(1);
    // (b) H from the span partials (stored [span][row]), placed as the reference does (evcont.py:41-68)
    for (size_t idx = tid; idx < Tp2; idx += kBT) M[idx] = 0.0;
    __syncthreads();
    for (int r = tid; r < T * T; r += kBT) {
        double s = 0.0;
        for (int k = 0; k < a.nsp1; ++k) s += a.h1part[(int64_t)k * T * T + r];
        const int i = r / T;
        M[(size_t)i * Tp + (r - i * T)] = a.alpha1 * s;
    }
    __syncthreads();
    for (int64_t r = tid; r < rows2; r += kBT) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int k = 0;
        for (; k + 4 <= a.nsp2; k += 4) {
            s0 += a.h2part[(int64_t)(k + 0) * rows2 + r];
            s1 += a.h2part[(int64_t)(k + 1) * rows2 + r];
            s2 += a.h2part[(int64_t)(k + 2) * rows2 + r];
            s3 += a.h2part[(int64_t)(k + 3) * rows2 + r];
        }
        for (; k < a.nsp2; ++k) s0 += a.h2part[(int64_t)k * rows2 + r];
        const double s = (s0 + s1) + (s2 + s3);
        int ia, ib;
        if (pairs) {
            ia = (int)tri_row(r);
            ib = (int)(r - (int64_t)ia * (ia + 1) / 2);
        } else {
            ia = (int)(r / T);
            ib = (int)(r - (int64_t)ia * T);
        }
        M[(size_t)ia * Tp + ib] += a.alpha2 * s;
    }
    __syncthreads();
    if (a.Hout)
        for (int idx = tid; idx < T * T; idx += kBT) {
            const int i = idx / T;
            a.Hout[idx] = M[(size_t)i * Tp + (idx - i * T)];
        }
    __syncthreads();
    for (int idx = tid; idx < T * T; idx += kBT) {   // Hs from the LOWER triangle (dsygst)
        const int i = idx / T, j = idx - i * T;
        if (j > i) M[(size_t)i * Tp + j] = M[(size_t)j * Tp + i];
    }
    __syncthreads();
    EVC_BSTAMP(2);
    // (c) W = B Hs (W[i][k] = sum_l B[i][l] Hs[k][l]);  C = W B^T (C[i][j] = sum_k W[i][k] B[j][k])
    big_mm_rr(Tp, Bg, Tp, M, Tp, [&](int i, int k, double v) { Wg[(size_t)i * Tp + k] = v; });
    __syncthreads();
    big_mm_rr(Tp, Wg, Tp, Bg, Tp, [&](int i, int j, double v) { Cg[(size_t)i * Tp + j] = v; });
    __syncthreads();
    EVC_BSTAMP(3);
    // exact symmetry (as the rotations assume) and the Gershgorin bound of the shift
    for (size_t idx = tid; idx < Tp2; idx += kBT) {
        const int i = (int)(idx / Tp), j = (int)(idx - (size_t)i * Tp);
        if (j < i) {
            const double v = 0.5 * (Cg[idx] + Cg[(size_t)j * Tp + i]);
            Cg[idx] = v;
            Cg[(size_t)j * Tp + i] = v;
        }
    }
    __syncthreads();
    double rmax = 0.0;
    for (int i = tid; i < T; i += kBT) {
        double rs = 0.0;
        for (int j = 0; j < T; ++j) rs += fabs(Cg[(size_t)i * Tp + j]);
        rmax = big_nanmax(rmax, rs);
    }
    rmax = big_block_max(rmax, red);
    const double shift = 2.0 * rmax + 1.0e-300;   // eigenvalues of the shifted matrix within [1, 3] x the bound
    EVC_BSTAMP(4);
    // (d') a few roots: tridiagonal route, verified; anything else (or a failed check): all eigenpairs by Jacobi
    bool few = false;
    if (kLds && a.few && a.nroots <= kFewRoots && T <= 128) {   // uniform
        for (size_t idx = tid; idx < Tp2; idx += kBT) M[idx] = Cg[idx];
        __syncthreads();
        few = big_few_roots(M, Cg, T, Tp, a.nroots, rmax + 1.0e-300, fw, red);
        EVC_BVAL(1, few ? 1.0 : 0.0);
        __syncthreads();
    }
    EVC_BSTAMP(5);
    if (!few) {
    // (d) G0, column-major with pitch Pj
    bool warm = false;
    if (a.warm && a.vstd) {   // uniform: the previous eigenvectors (rows of vstd, pitch Tp) must be orthonormal
        double dev = 0.0;
        big_mm_rr(Tp, a.vstd, Tp, a.vstd, Tp, [&](int i, int j, double v) {
            const double e = v - ((i == j && i < T) ? 1.0 : 0.0);
            dev = fma(e, e, dev);
        });
        dev = big_block_sum(dev, red);
        warm = dev < 1.0e-16;   // (NaN: false)
    }
    for (size_t idx = tid; idx < (size_t)m * Pj; idx += kBT) {
        const int j = (int)(idx / Pj), i = (int)(idx - (size_t)j * Pj);
        double v = 0.0;
        if (!warm && i < T && j < T) v = Cg[(size_t)i * Tp + j] + (i == j ? shift : 0.0);
        M[idx] = v;
    }
    __syncthreads();
    if (warm) {   // G[j][i] = sum_k Vt[j][k] C[i][k] + shift Vt[j][i]
        big_mm_rr(Tp, a.vstd, Tp, Cg, Tp, [&](int j, int i, double v) {
            if (j < T && i < T) M[(size_t)j * Pj + i] = v + shift * a.vstd[(size_t)j * Tp + i];
        });
        __syncthreads();
    }
    big_jacobi(M, m, Pj, red);
    // column norms = eigenvalues + shift; normalised columns = eigenvectors
    for (int j = tid >> 4; j < m; j += kBT / 16) {
        const int s = tid & 15;
        double nn = 0.0;
        for (int i = 2 * s; i < Pj; i += 32) {
            const double2 x = *reinterpret_cast<const double2 *>(M + (size_t)j * Pj + i);
            nn = fma(x.x, x.x, fma(x.y, x.y, nn));
        }
        nn = sum16(nn);
        const double l = sqrt(nn);
        const double inv = l > 1.0e-300 ? 1.0 / l : 0.0;   // (the decoupled dummy column of an odd problem stays zero)
        for (int i = 2 * s; i < Pj; i += 32) {
            double2 x = *reinterpret_cast<const double2 *>(M + (size_t)j * Pj + i);
            x.x *= inv;
            x.y *= inv;
            *reinterpret_cast<double2 *>(M + (size_t)j * Pj + i) = x;
        }
        if (s == 0 && j < Tp) ev[j] = l - shift;
    }
    __syncthreads();
    if (a.vstd)
        for (size_t idx = tid; idx < Tp2; idx += kBT) {
            const int j = (int)(idx / Tp), i = (int)(idx - (size_t)j * Tp);
            a.vstd[idx] = (j < T && i < T) ? M[(size_t)j * Pj + i] : 0.0;
        }
    // (e) ascending order
    for (int j = tid; j < T; j += kBT) {
        int rank = 0;
        const double v = ev[j];
        for (int k = 0; k < T; ++k) rank += (ev[k] < v || (ev[k] == v && k < j)) ? 1 : 0;
        order[rank] = j;
    }
    __syncthreads();
    }   // !few
    EVC_BSTAMP(6);
    // back-transformation c_i = sum_{k >= i} B[k][i] y_k for the requested roots
    for (int idx = tid; idx < a.nroots * T; idx += kBT) {
        const int root = idx / T, i = idx - root * T;
        const double *y = few ? fw.Y + (size_t)root * Tp : M + (size_t)order[root] * Pj;
        double c = 0.0;
        for (int k = i; k < T; ++k) c = fma(Bg[(size_t)k * Tp + i], y[k], c);
        a.evecs[idx] = c;
        if (root == 0) tmp[i] = c;   // (c0 may still hold Householder work: staged in tmp, copied below)
    }
    for (int r = tid; r < a.nroots; r += kBT) a.evals[r] = (few ? fw.lam[r] : ev[order[r]]) + a.e_shift;
    __syncthreads();
    for (int i = tid; i < T; i += kBT) c0[i] = tmp[i];
    __syncthreads();
    // weights of root 0 for the predicted RDMs (gradients_loewdin.py:343-356)
    if (a.w1)
        for (int idx = tid; idx < T * T; idx += kBT) {
            const int ia = idx / T;
            const double w = c0[ia] * c0[idx - ia * T];
            a.w1[idx] = w;
            // transposed copy for the batched K8: [row][slot] in the workspace of the group's first geometry
            if (a.w1t) a.w1t[(int64_t)idx * kMaxBatchG + (int)(blockIdx.x % kMaxBatchG)] = w;
        }
    if (a.w2) {
        for (int64_t r = tid; r < a.w2_count; r += kBT) {
            const int64_t g = r + a.w2_offset;
            double w;
            if (pairs) {
                const int ia = (int)tri_row(g), ib = (int)(g - (int64_t)ia * (ia + 1) / 2);
                w = (ia == ib) ? c0[ia] * c0[ia] : 2.0 * c0[ia] * c0[ib];
            } else {
                const int ia = (int)(g / T);
                w = c0[ia] * c0[g - (int64_t)ia * T];
            }
            a.w2[r] = w;
            if (a.w2t) a.w2t[r * kMaxBatchG + (int)(blockIdx.x % kMaxBatchG)] = w;
        }
    }
    EVC_BSTAMP(7);
}

static size_t big_aux_bytes(int T) {
    const int Tp = (T + 15) & ~15;
    return sizeof(double) * ((size_t)4 * Tp + 2 * kBW) + sizeof(int) * (size_t)(Tp + 2) +
           sizeof(double) * ((size_t)(2 + 3 * kFewRoots) * Tp + 3 * kFewRoots + 8) + sizeof(unsigned short) * kBT + 64;
}
static size_t big_matrix_doubles(int T) {
    const size_t m = (T + 1) & ~1, Tp = (T + 15) & ~15, Pj = (m + 31) & ~(size_t)31;
    return m * Pj > Tp * Tp ? m * Pj : Tp * Tp;
}
static bool big_fits_lds(int T) { return sizeof(double) * big_matrix_doubles(T) + big_aux_bytes(T) <= 160 * 1024; }

size_t subspace_big_scratch_doubles(int T) {
    const size_t Tp = (T + 15) & ~15;
    return 3 * Tp * Tp + (big_fits_lds(T) ? 0 : big_matrix_doubles(T));
}

int launch_subspace_big(const SolveArgs &a_in, int count, hipStream_t st) {
    SolveArgs a = a_in;
    a.few = subspace_few_enabled();
    if (!a.scratch) {
        set_error("subspace solve: T=%d needs a scratch buffer (evc_subspace_solve_ws_bytes)", a.T);
        return -1;
    }
    if (big_fits_lds(a.T)) {
        const size_t lds = sizeof(double) * big_matrix_doubles(a.T) + big_aux_bytes(a.T);
        static LdsAttr attr;
        if (int rc = allow_dynamic_lds(subspace_big_kernel<true>, attr, 160 * 1024, "subspace_big")) return rc;
        hipLaunchKernelGGL(subspace_big_kernel<true>, dim3(count), dim3(kBT), lds, st, a);
    } else {
        hipLaunchKernelGGL(subspace_big_kernel<false>, dim3(count), dim3(kBT), big_aux_bytes(a.T), st, a);
    }
    EVC_LAUNCH_CHECK("subspace_big");
    // (few: the tridiagonal route is tried -- the LDS-resident kernel only)
    note_kernel(EVC_PROF_SUBSPACE, "subspace_big_kernel<%d> few=%d", big_fits_lds(a.T) ? 1 : 0,
                big_fits_lds(a.T) && a.few && a.nroots <= kFewRoots && a.T <= 128 ? 1 : 0);
    return 0;
}

}  // namespace evc

#ifdef EVC_DEBUG_STAMPS
extern "C" int evc_debug_read_big(long long *stamps, double *vals, int n) {
    if (n > 16) n = 16;
    hipError_t e = hipMemcpyFromSymbol(stamps, HIP_SYMBOL(evc::g_big_stamp), sizeof(long long) * n);
    if (e == hipSuccess) e = hipMemcpyFromSymbol(vals, HIP_SYMBOL(evc::g_big_val), sizeof(double) * n);
    return (int)e;
}
#endif
