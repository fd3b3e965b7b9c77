// K1/K2  Loewdin orthogonalisation on ONE workgroup, n <= 32 on the fast paths, up to 80 in LDS alone:
//   X = S^-1/2, h1 = X^T h X  (electron_integral_utils.py:6-18,135; gradients_loewdin.py:336-338)
// loewdin_body is the kernel body of loewdin.hip's loewdin_kernel and the ride-along half of subspace_small.hip's
// subspace_loewdin_kernel.
#pragma once
#include "common.hpp"
#include "kernels.hpp"
#include "eigh_small.hpp"

namespace evc {

// ------------------------------------------------------------------ Loewdin: S^-1/2 without the eigensolver
// X = S^-1/2 and h1 = X h X are all the ENERGY phase needs from the Loewdin step (the eigenvectors and eigenvalues of S
// only enter the response term at the very end of the gradient, launch_grad_final).  The coupled Newton-Schulz iteration
//     Y_0 = S / c,  Z_0 = I,  T_k = (3 I - Z_k Y_k) / 2,  Y_k+1 = Y_k T_k,  Z_k+1 = Z_k T_k      (c = ||S||_inf >= lambda_max)
// (Higham, Functions of Matrices, eq. 6.35: Y -> (S/c)^1/2, Z -> (S/c)^-1/2, quadratically; all iterates are polynomials
// in S, hence symmetric and commuting) is three 32^3 products per step on the FP64 matrix cores, one 16 x 16 output tile
// per wave: ~0.8 us per step, 10-14 steps for cond(S) ~ 10^2-10^3, against ~65 us for the full eigendecomposition.
// One more step of the uncoupled form X <- X (3 I - X S X) / 2 on the ORIGINAL S removes what the coupled iterates have
// drifted and yields the residual max |I - X S X| the result is accepted on; anything else (S not positive definite,
// cond(S) beyond ~10^8, NaNs) returns false and the caller takes the eigensolver.
//
// LDS: 32 x 32 matrices at pitch 48 doubles -- the four rows a fragment read touches (k = lane >> 4) are 16 doubles
// apart modulo 32, i.e. on disjoint halves of the 64 banks; a symmetric A operand is read along the rows of A^T = A
// (lane & 15 -> consecutive addresses), so no operand is ever read with a stride.
constexpr int kNsP = 48;
constexpr int kNsSz = 32 * kNsP;
constexpr int kNsMaxIter = 64;
constexpr int kNsDoubles = 6 * kNsSz + 8;

// (kmax = 4 for n <= 16: K = 16 covers the matrix, and only the tile (0, 0) is active then)
__device__ __forceinline__ d4 ns_tile(const double *A, const double *B, int ao, int bo, int kmax) {
    d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 8; ++kk)
        if (kk < kmax)   // uniform
            acc = mfma_f64(A[kk * 4 * kNsP + ao], B[kk * 4 * kNsP + bo], acc);
    return acc;
}

__device__ bool loewdin_ns(const double *__restrict__ S, const double *__restrict__ h, double *__restrict__ X,
                           double *__restrict__ h1, int n, double *sm) {
    double *S0 = sm, *Yc = S0 + kNsSz, *Zc = Yc + kNsSz, *Yn = Zc + kNsSz, *Zn = Yn + kNsSz, *Tm = Zn + kNsSz;
    double *red = Tm + kNsSz;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int ti = wave >> 1, tj = wave & 1;
    const int ao = l4 * kNsP + 16 * ti + l15, bo = l4 * kNsP + 16 * tj + l15;
    const int oi = 16 * ti + l4, oj = 16 * tj + l15;   // output element of register r: (oi + 4 r, oj)
    // n <= 16: one tile holds the matrix -- the other three waves idle (their padding tiles are never read: K = 16)
    const bool act = 16 * ti < n && 16 * tj < n;
    const int kmax = n <= 16 ? 4 : 8;
    double hreg[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int idx = tid + u * kThreads, i = idx >> 5, j = idx & 31;
        const bool in = i < n && j < n;
        // (LAPACK's eigh reads the lower triangle: so does this)
        S0[i * kNsP + j] = in ? S[i >= j ? i * n + j : j * n + i] : (i == j ? 1.0 : 0.0);
        hreg[u] = (in && h) ? h[i * n + j] : 0.0;
    }
    __syncthreads();
    if (wave == 0) {
        double cs = 0.0;
        if (lane < 32)
            for (int i = 0; i < 32; ++i) cs += fabs(S0[i * kNsP + lane]);
        cs = wave_max_nan(cs);
        if (lane == 0) red[4] = cs;
    }
    __syncthreads();
    const double c = red[4];
    if (!(c > 0.0) || !(c < 1.0e300)) return false;   // (uniform: zero matrix, NaN, Inf)
    const double rc = 1.0 / c;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int idx = tid + u * kThreads, i = idx >> 5, j = idx & 31;
        const bool in = i < n && j < n;
        Yc[i * kNsP + j] = in ? S0[i * kNsP + j] * rc : (i == j ? 1.0 : 0.0);
        Zc[i * kNsP + j] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    bool ok = false;
    double eprev = 2.0;
    int it = 0;
#pragma unroll 1
    for (; it < kNsMaxIter; ++it) {
        double e = 0.0;
        if (act) {
            const d4 p = ns_tile(Zc, Yc, ao, bo, kmax);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double dlt = (oi + 4 * r == oj) ? 1.0 : 0.0;
                e = nanmax(e, fabs(dlt - p[r]));
                Tm[(oi + 4 * r) * kNsP + oj] = 1.5 * dlt - 0.5 * p[r];
            }
            e = wave_max_nan(e);
        }
        if (lane == 0) red[wave] = e;
        __syncthreads();
        e = nanmax(nanmax(red[0], red[1]), nanmax(red[2], red[3]));
        if (act) {
            d4 yn = {0.0, 0.0, 0.0, 0.0}, zn = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 8; ++kk)
                if (kk < kmax) {
                    const double b = Tm[kk * 4 * kNsP + bo];
                    yn = mfma_f64(Yc[kk * 4 * kNsP + ao], b, yn);
                    zn = mfma_f64(Zc[kk * 4 * kNsP + ao], b, zn);
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Yn[(oi + 4 * r) * kNsP + oj] = yn[r];
                Zn[(oi + 4 * r) * kNsP + oj] = zn[r];
            }
        }
        __syncthreads();
        double *t0 = Yc;
        Yc = Yn;
        Yn = t0;
        t0 = Zc;
        Zc = Zn;
        Zn = t0;
        if (e != e) break;
        // e = max |I - Z Y| BEFORE this step; the step squares it (3/4 e^2).  Below 1e-3 a step that does not even halve
        // it has reached the rounding floor of an ill-conditioned S: the residual test below decides.
        if (e < 1.0e-8 || (e < 1.0e-3 && e > 0.5 * eprev)) {
            ok = true;
            ++it;
            break;
        }
        eprev = e;
    }
    EVC_DBGVAL(50, it);
    if (!ok) return false;
    // X = Z / sqrt(c), then one step on the original S:  W = S X,  P = X W,  X <- X (3 I - P) / 2
    const double rsq = sqrt(rc);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int idx = tid + u * kThreads, i = idx >> 5, j = idx & 31;
        if (i < n && j < n) Zc[i * kNsP + j] *= rsq;
    }
    __syncthreads();
    if (act) {
        const d4 wv = ns_tile(S0, Zc, ao, bo, kmax);
#pragma unroll
        for (int r = 0; r < 4; ++r) Tm[(oi + 4 * r) * kNsP + oj] = wv[r];
    }
    __syncthreads();
    double res;
    {
        double e = 0.0;
        if (act) {
            const d4 p = ns_tile(Zc, Tm, ao, bo, kmax);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double dlt = (oi + 4 * r == oj) ? 1.0 : 0.0;
                e = nanmax(e, fabs(dlt - p[r]));
                Yn[(oi + 4 * r) * kNsP + oj] = 1.5 * dlt - 0.5 * p[r];
            }
            e = wave_max_nan(e);
        }
        if (lane == 0) red[wave] = e;
        __syncthreads();
        res = nanmax(nanmax(red[0], red[1]), nanmax(red[2], red[3]));
    }
    EVC_DBGVAL(51, res);
    if (!(res < 1.0e-7)) return false;   // (after the step: ~res^2)
    if (act) {
        const d4 xv = ns_tile(Zc, Yn, ao, bo, kmax);
#pragma unroll
        for (int r = 0; r < 4; ++r) Zn[(oi + 4 * r) * kNsP + oj] = xv[r];
    }
    __syncthreads();
    // symmetrised X -> Yc and the caller; h^T -> Tm (the A operand is read along rows of its transpose)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int idx = tid + u * kThreads, i = idx >> 5, j = idx & 31;
        const bool in = i < n && j < n;
        const double v = in ? 0.5 * (Zn[i * kNsP + j] + Zn[j * kNsP + i]) : (i == j ? 1.0 : 0.0);
        Yc[i * kNsP + j] = v;
        if (in) X[i * n + j] = v;
        Tm[j * kNsP + i] = hreg[u];
    }
    if (!(h && h1)) return true;
    __syncthreads();
    if (act) {
        const d4 wv = ns_tile(Tm, Yc, ao, bo, kmax);   // W = h X
#pragma unroll
        for (int r = 0; r < 4; ++r) Yn[(oi + 4 * r) * kNsP + oj] = wv[r];
    }
    __syncthreads();
    if (act) {
        const d4 hv = ns_tile(Yc, Yn, ao, bo, kmax);   // h1 = X W
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (oi + 4 * r < n && oj < n) h1[(oi + 4 * r) * n + oj] = hv[r];
    }
    return true;
}

// ------------------------------------------------------------------ Loewdin
__device__ __forceinline__ void loewdin_body(LoewdinArgs a, const int64_t g) {
    const int n = a.n;
    const double *__restrict__ S = a.S + g * a.sS;
    const double *__restrict__ h = a.h ? a.h + g * a.sh : nullptr;
    double *__restrict__ X = a.X + g * a.sws;
    double *__restrict__ U = a.U + g * a.sws;
    double *__restrict__ sv = a.s + g * a.sws;
    double *__restrict__ h1 = a.h1 ? a.h1 + g * a.sws : nullptr;
    extern __shared__ __align__(16) double sm[];
    const int m = (n + 1) & ~1;
    // part = 1: X and h1 only, by Newton-Schulz (the eigensolver below only if that declines, and then without touching
    // U and s, which a part = 2 launch on another stream is writing); part = 2: U and s only; 0: everything
    const bool want_x = a.part != 2, want_u = a.part != 1;
    if (a.part == 1 && m <= kJwMax && a.fast) {
        if (loewdin_ns(S, h, X, h1, n, sm)) return;
        __syncthreads();
    }
    double *A = sm;              // m*m   (later: hcore)
    double *V = A + m * m;       // m*m   (later: T = h X)
    double *Xs = V + m * m;      // m*m   (uses n*n)
    double *rot = Xs + m * m;    // m
    double *red = rot + m;       // 8
    double *f = red + 8;         // m
    double *Gc = f + m;          // kJwMax x kJwPitch (only carved for m <= kJwMax), then the refinement's six matrices
    double *R6 = Gc + kJwMax * kJwPitch;
    const int tid = threadIdx.x, tk = tid & 15, tj = tid >> 4;
    // LAPACK's eigh reads one triangle; numpy.linalg.eigh uses the lower one.
    for (int idx = tid; idx < m * m; idx += kThreads) A[idx] = 0.0;
    __syncthreads();
    for (int idx = tid; idx < n * n; idx += kThreads) {
        const int i = idx / n, j = idx - i * n;
        const double v = S[idx];
        if (i >= j) {
            A[i * m + j] = v;
            A[j * m + i] = v;
        }
    }
    __syncthreads();
    // warm start from the eigenvectors the previous call left in U (same workspace, nearby geometry)
    // (hcore is only needed behind the eigensolver: requested now, its latency is gone by then)
    double hpre[(kRsz + kThreads - 1) / kThreads];
    if (m <= kJwMax && a.fast) {
#pragma unroll
        for (int u = 0; u < (kRsz + kThreads - 1) / kThreads; ++u) {
            const int idx = tid + u * kThreads, i = idx / kRp, j = idx - i * kRp;
            hpre[u] = (idx < kRsz && i < n && j < n && h) ? h[i * n + j] : 0.0;
        }
    }
    if (m <= kJwMax && a.fast) {
        if (a.warm) {   // refinement straight from U (a stale or never-written buffer makes it fall back)
            for (int idx = tid; idx < m * m; idx += kThreads) {
                const int i = idx / m, j = idx - i * m;
                V[idx] = (i < n && j < n) ? U[i * n + j] : (i == j ? 1.0 : 0.0);
            }
            __syncthreads();
        }
        eigh_small(A, V, m, n, 0.0, a.warm != 0, a.fast, R6, Gc, f, red);
    } else {
        const bool warm = a.warm && warm_start_rotate(A, V, Xs, n, m, U, n, red);
        if (m <= kJwMax) jacobi_eigh_wave(A, V, m, 0.0, !warm, Gc, f);
        else jacobi_eigh_lds(A, V, m, rot, red, !warm);
    }
    if (tid < m) {
        const double s = A[tid * m + tid];
        f[tid] = (tid < n && s > 1.0e-15) ? 1.0 / sqrt(s) : 0.0;
        if (tid < n && want_u) sv[tid] = s;
    }
    __syncthreads();
    if (m <= kJwMax && a.fast) {
        // X = V diag(f) V^T and h1 = X^T h X as row.row products at pitch kRp (the refinement's buffers are free)
        double *Vf = R6, *Vp = R6 + kRsz, *Xp = R6 + 2 * kRsz, *hp = R6 + 3 * kRsz, *Tt = R6 + 4 * kRsz;
#pragma unroll
        for (int u = 0; u < (kRsz + kThreads - 1) / kThreads; ++u) {
            const int idx = tid + u * kThreads;
            if (idx < kRsz) {
                const int i = idx / kRp, j = idx - i * kRp;
                const bool in = i < n && j < n;
                const double v = in ? V[i * m + j] : 0.0;
                Vp[idx] = v;
                Vf[idx] = in ? v * f[j] : 0.0;
                hp[idx] = hpre[u];
                Xp[idx] = 0.0;
                Tt[idx] = 0.0;
                if (in && want_u) U[i * n + j] = v;
            }
        }
        if (!want_x) return;
        __syncthreads();
        mm_rowrow(m, Vf, Vp, [&](int i, int j, double v) {
            if (i < n && j < n) {
                Xp[i * kRp + j] = v;
                X[i * n + j] = v;
            }
        });
        if (h && h1) {
            __syncthreads();
            // Tt[j][i] = (h X)[i][j] = sum_k X[j][k] h[i][k]  (X symmetric);  h1[i][j] = sum_k X[i][k] Tt[j][k]
            mm_rowrow(m, Xp, hp, [&](int j, int i, double v) { Tt[j * kRp + i] = v; });
            __syncthreads();
            mm_rowrow(m, Xp, Tt, [&](int i, int j, double v) {
                if (i < n && j < n) h1[i * n + j] = v;
            });
        }
        return;
    }
    // X = V diag(f) V^T  (a dummy column, if any, has f = 0)
    mm16(n, [&](int i, int k) { return V[i * m + k] * f[k]; }, [&](int k, int j) { return V[j * m + k]; },
         [&](int i, int j, double v) {
             Xs[i * n + j] = v;
             X[i * n + j] = v;
         });
    for (int i = tj; i < n; i += 16)
        for (int j = tk; j < n; j += 16) U[i * n + j] = V[i * m + j];
    if (h && h1) {
        copy_to_lds(A, h, n * n);
        __syncthreads();
        // T = h X (into V), h1 = X^T T
        mm16(n, [&](int i, int k) { return A[i * n + k]; }, [&](int k, int j) { return Xs[k * n + j]; },
             [&](int i, int j, double v) { V[i * n + j] = v; });
        __syncthreads();
        mm16(n, [&](int i, int k) { return Xs[k * n + i]; }, [&](int k, int j) { return V[k * n + j]; },
             [&](int i, int j, double v) { h1[i * n + j] = v; });
    }
}

}  // namespace evc
