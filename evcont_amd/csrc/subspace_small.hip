// K6  subspace generalised eigenproblem for T <= 32, LAPACK dsygvd semantics (evcont.py:38-90,157-173), with the
// weights of root 0 (gradients_loewdin.py:343-353): one workgroup per geometry, matrices in LDS.  Larger training
// sets: subspace_big.hip.  subspace_loewdin_kernel carries the eigendecomposition half of the Loewdin step
// (loewdin.hpp) in the same launch.
#include <stdlib.h>
#include <string.h>

#include "common.hpp"
#include "kernels.hpp"
#include "loewdin.hpp"

namespace evc {
#include "few_roots.hpp"   // (inside namespace evc, behind the phase-stamp macros of eigh_small.hpp)

// Cholesky factor of the symmetric positive definite T x T matrix S (lower triangle of Ssrc, pitch T) and its
// inverse B = L^-1, on ONE wave with everything in registers: lane i holds row i of L; the pivot and the column
// entries a step needs from other lanes travel through v_readlane (uniform operands), so the 2 T dependent steps
// carry no LDS round trip and no barrier.  Writes B (lower triangular) to Bi at pitch kRp; a matrix that is not
// positive definite yields NaNs.  T <= 32.  Called by wave 0 only.
__device__ __forceinline__ void chol_inverse_wave(const double *Ssrc, int T, double *Bi) {
    const int i = threadIdx.x & 31;
    double a[32], rinv[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        a[k] = (i < T && k < T) ? (k <= i ? Ssrc[i * T + k] : 0.0) : (k == i ? 1.0 : 0.0);
        rinv[k] = 1.0;
    }
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        if (j < T) {   // uniform
            const double d = readlane_f64(a[j], j);
            double rs = __builtin_amdgcn_rsq(d);
            rs = rs * fma(-0.5 * d * rs, rs, 1.5);
            rs = rs * fma(-0.5 * d * rs, rs, 1.5);
            const double lij = a[j] * rs;   // lane j: sqrt(d)
            a[j] = lij;
            rinv[j] = rs;                   // 1 / L_jj (uniform)
#pragma unroll
            for (int k = j + 1; k < 32; ++k)
                if (k < T) a[k] = fma(-lij, readlane_f64(lij, k), a[k]);
        }
    }
    double b[32];
#pragma unroll
    for (int r = 0; r < 32; ++r) {
        b[r] = 0.0;
        if (r < T) {   // uniform
            double acc = (r == i) ? 1.0 : 0.0, acc2 = 0.0;
#pragma unroll
            for (int k = 0; k + 1 < r; k += 2) {
                acc = fma(-readlane_f64(a[k], r), b[k], acc);
                acc2 = fma(-readlane_f64(a[k + 1], r), b[k + 1], acc2);
            }
            if (r & 1) acc = fma(-readlane_f64(a[r - 1], r), b[r - 1], acc);
            b[r] = (acc + acc2) * rinv[r];
        }
    }
    if (threadIdx.x < 32 && i < T) {
#pragma unroll
        for (int r = 0; r < 32; ++r)
            if (r < T) Bi[r * kRp + i] = b[r];
    }
}

// ------------------------------------------------------------------ subspace solve
__device__ __forceinline__ void subspace_body(SolveArgs a, const int64_t gblk) {
    extern __shared__ __align__(16) double sm[];
    {
        const int64_t g = gblk;
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
        if (a.e_shift_dev) a.e_shift = a.e_shift_dev[g];
    }
    EVC_STAMP(30);
    const int T = a.T;
    const int m = (T + 1) & ~1;
    double *H = sm;             // T*T  assembled H; later the coefficient vectors
    double *L = H + m * m;      // T*T  Cholesky factor (lower)
    double *Cm = L + m * m;     // m*m  standard-form matrix
    double *V = Cm + m * m;     // m*m
    double *red = V + m * m + m;   // 8 (behind m unused doubles: the carve jacobi_aux_bytes sizes, as loewdin_body's)
    double *ev = red + 8;       // m
    int *order = reinterpret_cast<int *>(ev + m);                              // m
    // kJwMax x kJwPitch doubles for the single-wave eigensolver (only carved for m <= kJwMax), 16-byte aligned,
    // followed by the refinement's six matrices
    double *Gc = reinterpret_cast<double *>((reinterpret_cast<uintptr_t>(order + m) + 15) & ~(uintptr_t)15);
    double *R6 = Gc + kJwMax * kJwPitch;
    const int tid = threadIdx.x;
    const int64_t P = (int64_t)T * (T + 1) / 2;
    const bool pairs = layout_pairs(a.layout);
    const int64_t rows2 = pairs ? P : (int64_t)T * T;

    // (1) one-body rows (partials are stored [span][row]: coalesced over rows)
    for (int r = tid; r < T * T; r += kThreads) {
        double s = 0.0;
        for (int k = 0; k < a.nsp1; ++k) s += a.h1part[(int64_t)k * T * T + r];
        H[r] = a.alpha1 * s;
    }
    // S lower triangle -> L
    for (int idx = tid; idx < T * T; idx += kThreads) {
        const int i = idx / T, j = idx - i * T;
        L[idx] = (i >= j) ? a.S[idx] : 0.0;
    }
    __syncthreads();
    // (2) two-body rows, placed as the reference does (evcont.py:41-68)
    for (int64_t r = tid; r < rows2; r += kThreads) {
        // (eight loads in flight per thread: up to 64 spans are summed here instead of in a launch of their own)
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
        int k = 0;
        for (; k + 8 <= a.nsp2; k += 8) {
            s0 += a.h2part[(int64_t)(k + 0) * rows2 + r];
            s1 += a.h2part[(int64_t)(k + 1) * rows2 + r];
            s2 += a.h2part[(int64_t)(k + 2) * rows2 + r];
            s3 += a.h2part[(int64_t)(k + 3) * rows2 + r];
            s4 += a.h2part[(int64_t)(k + 4) * rows2 + r];
            s5 += a.h2part[(int64_t)(k + 5) * rows2 + r];
            s6 += a.h2part[(int64_t)(k + 6) * rows2 + r];
            s7 += a.h2part[(int64_t)(k + 7) * rows2 + r];
        }
        for (; k < a.nsp2; ++k) s0 += a.h2part[(int64_t)k * rows2 + r];
        const double s = ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7));
        int ia, ib;
        if (pairs) {
            ia = (int)tri_row(r);
            ib = (int)(r - (int64_t)ia * (ia + 1) / 2);
        } else {
            ia = (int)(r / T);
            ib = (int)(r - (int64_t)ia * T);
        }
        H[ia * T + ib] += a.alpha2 * s;
    }
    __syncthreads();
    if (a.Hout)
        for (int idx = tid; idx < T * T; idx += kThreads) a.Hout[idx] = H[idx];
    const bool fastbase = a.fast && m <= kJwMax;   // workgroup-parallel factorisation (T <= 32)
    EVC_STAMP(31);
    if (fastbase) {
        // (3') Cholesky S = L L^T and B = L^-1 in the registers of one wave (chol_inverse_wave); (4') C = B Hsym B^T as
        //      two row.row products on the workgroup, matrices at pitch kRp in the refinement's buffers (free until the
        //      eigensolver starts).  The left-looking thread-per-row loops of the general path below are chains of
        //      ~T^2/2 dependent LDS reads each.
        double *Bi = R6 + kRsz, *Hs = R6 + 2 * kRsz, *Wt = R6 + 3 * kRsz;
        // S_train is the same for every geometry: B = L^-1 is cached in the workspace next to the matrix it was computed
        // from and reused when that matrix is bit-identical to this call's (uninitialised or stale memory: a miss)
        double sv[4];   // this thread's elements of the overlap matrix (T*T <= 1024)
        int same = a.bcache ? 1 : 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = tid + u * kThreads;
            sv[u] = idx < T * T ? L[idx] : 0.0;
            if (a.bcache && idx < T * T) same &= (a.bcache[idx] == sv[u]) ? 1 : 0;
        }
        // (block-wide AND through the reduction scratch; __syncthreads_and would add static LDS to a kernel that asks for
        //  all 160 KB dynamically)
        const bool hit = block_max_nan(same ? 0.0 : 1.0, red) == 0.0;
        for (int idx = tid; idx < kRsz; idx += kThreads) {
            const int i = idx / kRp, j = idx - i * kRp;
            const bool in = i < T && j < T;
            Hs[idx] = in ? (i >= j ? H[i * T + j] : H[j * T + i]) : 0.0;
            Bi[idx] = (hit && in) ? a.bcache[T * T + i * T + j] : 0.0;
        }
        __syncthreads();
        if (!hit) {   // workgroup-uniform
            if (tid < 64) chol_inverse_wave(L, T, Bi);
            __syncthreads();
            if (a.bcache) {
                for (int idx = tid; idx < T * T; idx += kThreads) {
                    const int i = idx / T, j = idx - i * T;
                    a.bcache[T * T + idx] = Bi[i * kRp + j];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int idx = tid + u * kThreads;
                    if (idx < T * T) a.bcache[idx] = sv[u];
                }
            }
        }
        EVC_STAMP(33);
        // Wt[j][k] = sum_l B[j][l] Hs[k][l];  C[i][j] = sum_k B[i][k] Wt[j][k]  (rows >= T are zero: decoupled dummy)
        mm_rowrow(m, Bi, Hs, [&](int j, int k, double v) { Wt[j * kRp + k] = v; });
        __syncthreads();
        mm_rowrow(m, Bi, Wt, [&](int i, int j, double v) { V[i * m + j] = v; });
        // keep B = L^-1 (pitch m) where the left-looking path keeps L: the back-transformation is c = B^T y
        for (int idx = tid; idx < m * m; idx += kThreads) {
            const int i = idx / m, j = idx - i * m;
            L[idx] = Bi[i * kRp + j];
        }
        __syncthreads();
    } else {
    // (3) Cholesky of S (lower triangle, as dpotrf('L')), left-looking: thread i owns row i and
        //     recomputes the pivot itself, so the column needs no barrier between pivot and scaling.
        for (int j = 0; j < T; ++j) {
            const int i = tid;
            double v = 0.0, d = 0.0;
            if (i >= j && i < T) {
                v = L[i * T + j];
                d = L[j * T + j];
                for (int k = 0; k < j; ++k) {
                    const double ljk = L[j * T + k];
                    v = fma(-L[i * T + k], ljk, v);
                    d = fma(-ljk, ljk, d);
                }
                d = sqrt(d);
            }
            __syncthreads();
            if (i >= j && i < T) L[i * T + j] = (i == j) ? d : v / d;
            __syncthreads();
        }
        // (4) C = L^-1 Hsym L^-T, Hsym from the LOWER triangle of H (dsygst).
        //     thread j solves L z = Hsym[:,j]; result in Cm[:,j]
        if (tid < T) {
            const int j = tid;
            for (int i = 0; i < T; ++i) {
                double v = (i >= j) ? H[i * T + j] : H[j * T + i];
                for (int k = 0; k < i; ++k) v = fma(-L[i * T + k], Cm[k * m + j], v);
                Cm[i * m + j] = v / L[i * T + i];
            }
        }
        __syncthreads();
        //     thread i solves L w = Z[i,:]^T; result is row i of C, kept in V[i,:]
        if (tid < T) {
            const int i = tid;
            for (int j = 0; j < T; ++j) {
                double v = Cm[i * m + j];
                for (int k = 0; k < j; ++k) v = fma(-L[j * T + k], V[i * m + k], v);
                V[i * m + j] = v / L[j * T + j];
            }
        }
        __syncthreads();
    }
    for (int idx = tid; idx < m * m; idx += kThreads) {
        const int i = idx / m, j = idx - i * m;
        double v = 0.0;
        if (i < T && j < T) v = 0.5 * (V[i * m + j] + V[j * m + i]);
        Cm[idx] = v;  // the dummy dimension (odd T) stays decoupled and is skipped below
    }
    __syncthreads();
    EVC_STAMP(34);
    // A few lowest roots (the energy+force path asks for one): double-precision tridiagonal route on ONE wave, verified
    // against the matrix (few_roots.hpp); anything it does not like falls through to the full eigensolver below.
    bool few_ok = false;
    // (a warm-started call skips it: the refinement from the previous call's eigenvectors below is faster still -- H30,
    //  one geometry per step: 4 420 -> 4 900 steps/s; the call after a cold one finds no such vectors, runs the full
    //  eigensolver once and leaves them)
    if (a.few && !(a.warm && a.vstd) && fastbase && a.nroots <= few::kMaxRoots && T >= 2) {
        if (tid < 64) {
            const int why = T <= 8    ? few::few_roots_wave<8>(Cm, m, T, a.nroots, ev, V, T, R6, red + 2)
                            : T <= 16 ? few::few_roots_wave<16>(Cm, m, T, a.nroots, ev, V, T, R6, red + 2)
                            : T <= 24 ? few::few_roots_wave<24>(Cm, m, T, a.nroots, ev, V, T, R6, red + 2)
                                      : few::few_roots_wave<32>(Cm, m, T, a.nroots, ev, V, T, R6, red + 2);
            if (tid == 0) red[0] = why == 0 ? 1.0 : 0.0;
            EVC_DBGVAL(40, why);
            EVC_DBGVAL(41, red[2]);
            EVC_DBGVAL(42, red[3]);
            EVC_DBGVAL(43, red[4]);
            EVC_DBGVAL(44, red[5]);
        }
        __syncthreads();
        few_ok = red[0] != 0.0;
        __syncthreads();
        EVC_STAMP(37);
    }
    // warm start from the standard-form eigenvectors of the previous call (H is free as scratch here)
    if (few_ok) {
        // (ev[r], V[r * T + i]: root r ascending; c = B^T y below)
    } else {   // (T <= kSubspaceSmallT = kJwMax is guaranteed by the launchers: the wave solvers serve every call)
        // the standard-form matrix is indefinite: shift it by a Gershgorin bound (the eigenvectors do not change)
        if (tid < m) {
            double rs = 0.0;
            for (int j = 0; j < m; ++j) rs += fabs(Cm[tid * m + j]);
            ev[tid] = rs;
        }
        __syncthreads();
        double shift = 0.0;
        for (int j = 0; j < m; ++j) shift = fmax(shift, ev[j]);
        shift = 2.0 * shift + 1.0e-300;   // eigenvalues of the shifted matrix within [1, 3] x the bound
        __syncthreads();
        if (a.fast) {
            const bool warm = a.warm && a.vstd;
            if (warm) {   // refinement straight from the previous eigenvectors (garbage makes it fall back)
                for (int idx = tid; idx < m * m; idx += kThreads) V[idx] = a.vstd[idx];
                __syncthreads();
            }
            eigh_small(Cm, V, m, T, shift, warm, a.fast, R6, Gc, ev, red);
        } else {
            const bool warm = a.warm && a.vstd && warm_start_rotate(Cm, V, H, T, m, a.vstd, m, red);
            jacobi_eigh_wave(Cm, V, m, shift, !warm, Gc, ev);
        }
    }
    if (a.vstd && !few_ok)
        for (int idx = tid; idx < m * m; idx += kThreads) a.vstd[idx] = V[idx];
    EVC_STAMP(35);
    // (5) ascending order
    if (!few_ok) {
        if (tid < T) ev[tid] = Cm[tid * m + tid];
        __syncthreads();
        if (tid < T) {
            int rank = 0;
            const double v = ev[tid];
            for (int j = 0; j < T; ++j) rank += (ev[j] < v || (ev[j] == v && j < tid)) ? 1 : 0;
            order[rank] = tid;
        }
        __syncthreads();
    }
    // (6) back-transform c = L^-T y for the requested roots; store into H region
    if (few_ok) {
        // c_i = sum_{k >= i} B[k][i] y_k, y = row `root` of V (pitch T)
        for (int idx = tid; idx < a.nroots * T; idx += kThreads) {
            const int root = idx / T, i = idx - root * T;
            double c = 0.0;
            for (int k = i; k < T; ++k) c = fma(L[k * m + i], V[root * T + k], c);
            H[idx] = c;
        }
        if (tid < a.nroots) a.evals[tid] = ev[tid] + a.e_shift;
    } else if (fastbase) {
        // c_i = sum_{k >= i} B[k][i] y_k with B = L^-1 kept in `L` (pitch m): one thread per (root, i)
        for (int idx = tid; idx < a.nroots * T; idx += kThreads) {
            const int root = idx / T, i = idx - root * T, col = order[root];
            double c = 0.0;
            for (int k = i; k < T; ++k) c = fma(L[k * m + i], V[k * m + col], c);
            H[idx] = c;
        }
        if (tid < a.nroots) a.evals[tid] = ev[order[tid]] + a.e_shift;
    } else if (tid < a.nroots) {
        const int col = order[tid];
        double *c = H + tid * T;
        for (int i = T - 1; i >= 0; --i) {
            double v = V[i * m + col];
            for (int k = i + 1; k < T; ++k) v = fma(-L[k * T + i], c[k], v);
            c[i] = v / L[i * T + i];
        }
        a.evals[tid] = ev[col] + a.e_shift;
    }
    __syncthreads();
    for (int idx = tid; idx < a.nroots * T; idx += kThreads) a.evecs[idx] = H[idx];
    EVC_STAMP(36);
    // (7) weights of root 0 for the predicted RDMs
    const double *c0 = H;
    if (a.w1)
        for (int idx = tid; idx < T * T; idx += kThreads) {
            const int ia = idx / T;
            const double w = c0[ia] * c0[idx - ia * T];
            a.w1[idx] = w;
            // transposed copy for the batched K8: [row][slot] in the workspace of the group's first geometry
            if (a.w1t) a.w1t[(int64_t)idx * kMaxBatchG + (int)(gblk % kMaxBatchG)] = w;
        }
    if (a.w2) {
        for (int64_t r = tid; r < a.w2_count; r += kThreads) {
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
            // transposed copy for the batched K8: [row][slot] in the workspace of the group's first geometry
            if (a.w2t) a.w2t[r * kMaxBatchG + (int)(gblk % kMaxBatchG)] = w;
        }
    }
}

__global__ __launch_bounds__(kThreads) void subspace_kernel(SolveArgs a) { subspace_body(a, blockIdx.x); }

// The subspace solve and the eigendecomposition half of the Loewdin step (part 2: U and s, which the gradient's last
// kernel alone reads) in ONE launch: `count` workgroups each, both one workgroup per geometry and latency-bound, neither
// depending on the other -- the eigensolver (~75 us) then runs beside the subspace solve (~54 us) instead of in front of
// the whole energy phase, with no second stream (batches of 12 and more geometries; smaller calls send it to the side
// stream, side_stream.hip).
__global__ __launch_bounds__(kThreads) void subspace_loewdin_kernel(SolveArgs sa, LoewdinArgs la, int count) {
    if ((int)blockIdx.x < count) subspace_body(sa, blockIdx.x);
    else loewdin_body(la, (int64_t)blockIdx.x - count);
}

// The host's view of the few-roots condition of subspace_body: whether the kernel tries the tridiagonal route (it still
// falls through to the full eigensolver when the route's own check fails on the device).
static bool subspace_few_tried(const SolveArgs &a) {
    return a.few && !(a.warm && a.vstd) && a.fast && a.nroots <= few::kMaxRoots && a.T >= 2;
}

int launch_subspace_loewdin(const SolveArgs &s_in, const LoewdinArgs &l_in, int count, hipStream_t st) {
    SolveArgs a = s_in;
    LoewdinArgs l = l_in;
    a.fast = l.fast = eigh_fast_enabled();
    dbg_upload_max_sweeps();
    a.few = subspace_few_enabled();
    l.part = 2;
    if (a.T > kSubspaceSmallT || l.n > kJwMax || !l.fast) {
        set_error("subspace + Loewdin in one launch: T=%d, n=%d outside the small-kernel range", a.T, l.n);
        return -1;
    }
    const int m = (a.T + 1) & ~1, ml = (l.n + 1) & ~1;
    const size_t lds_s = sizeof(double) * (size_t)4 * m * m + sizeof(int) * m + jacobi_aux_bytes(m);
    const size_t lds_l = sizeof(double) * (size_t)3 * ml * ml + jacobi_aux_bytes(ml);
    static LdsAttr attr;
    if (int rc = allow_dynamic_lds(subspace_loewdin_kernel, attr, 160 * 1024, "subspace_loewdin")) return rc;
    hipLaunchKernelGGL(subspace_loewdin_kernel, dim3(2 * count), dim3(kThreads), lds_s > lds_l ? lds_s : lds_l, st, a, l,
                       count);
    EVC_LAUNCH_CHECK("subspace_loewdin");
    note_kernel(EVC_PROF_SUBSPACE, "subspace_loewdin_kernel few=%d", subspace_few_tried(a) ? 1 : 0);
    return 0;
}

int launch_subspace_solve(const SolveArgs &a_in, int count, hipStream_t st) {
    // (measured: 0.26 / 0.42 / 0.61 ms at T = 33 / 48 / 64 against 0.62 / 1.14 / 1.89 ms for the two-sided LDS Jacobi
    //  this file used up to T = 64 in round 2)
    if (a_in.T > kSubspaceSmallT) return launch_subspace_big(a_in, count, st);
    SolveArgs a = a_in;
    a.fast = eigh_fast_enabled();
    dbg_upload_max_sweeps();
    a.few = subspace_few_enabled();
    const int m = (a.T + 1) & ~1;
    const size_t lds = sizeof(double) * (size_t)4 * m * m + sizeof(int) * m + jacobi_aux_bytes(m);
    static LdsAttr attr;
    if (int rc = allow_dynamic_lds(subspace_kernel, attr, 160 * 1024, "subspace_solve")) return rc;
    hipLaunchKernelGGL(subspace_kernel, dim3(count), dim3(kThreads), lds, st, a);
    EVC_LAUNCH_CHECK("subspace_solve");
    note_kernel(EVC_PROF_SUBSPACE, "subspace_kernel few=%d", subspace_few_tried(a) ? 1 : 0);
    return 0;
}

}  // namespace evc

#ifdef EVC_DEBUG_STAMPS
extern "C" int evc_debug_read_subspace(long long *stamps, double *vals, int n) { return evc::dbg_read(stamps, vals, n); }
#endif
