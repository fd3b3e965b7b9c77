// Eigensolvers of the single-workgroup dense kernels (symmetric matrices of up to 32 x 32 on one wave or one workgroup,
// beyond that the two-sided Jacobi in LDS), their DPP / reduction helpers, the warm start and the phase stamps of the
// timing experiments.  eigh_small is the entry point for m <= 32; the LDS these routines need beyond the caller's
// matrices is jacobi_aux_bytes(m).
#pragma once
#include <stdlib.h>

#include "common.hpp"
#include "small_mm.hpp"

namespace evc {

// ------------------------------------------------------------------ Jacobi eigensolver (LDS)
// A (m x m, m even, symmetric, both triangles kept) is diagonalised in place; V accumulates the
// rotations (columns = eigenvectors).  Pairs follow the round-robin tournament, computed
// arithmetically: at step s pair k is (k ? (s+k) mod (m-1) : m-1, (s+m-1-k) mod (m-1)), so the m/2
// rotations of a step are disjoint.  A step is: (i) m/2 lanes compute (c,s); barrier; (ii) every 2x2
// block (pair k) x (pair k2), k<=k2, gets its row AND column rotation in registers and is mirrored;
// V gets the column rotation; barrier.  The kernel is a chain of ~7(m-1) such latency-bound steps,
// so the rotation uses the hardware rcp/rsq seeds with explicit Newton steps: the angle needs
// only ~1e-8 (it merely has to make a_pq small), while c is refined to full precision so that
// c^2+s^2 = 1 to rounding and V stays orthogonal.
__device__ __forceinline__ void pair_of(int step, int k, int m, int &p, int &q) {
    const int w = m - 1;
    p = step + k;
    if (p >= w) p -= w;
    if (k == 0) p = w;
    q = step + w - k;
    if (q >= w) q -= w;
}

__device__ __forceinline__ void jacobi_rotation(double app, double aqq, double apq, double &c, double &s) {
    c = 1.0;
    s = 0.0;
    if (fabs(apq) > 1.0e-150) {
        // t = sgn(d) b / (|d| + sqrt(d^2 + b^2)), d = aqq - app, b = 2 apq  (the smaller root)
        const double d = aqq - app, b = 2.0 * apq;
        const double h2 = fma(d, d, b * b);
        double y = __builtin_amdgcn_rsq(h2);
        y = y * fma(-0.5 * h2 * y, y, 1.5);
        const double den = fabs(d) + h2 * y;
        double r = __builtin_amdgcn_rcp(den);
        r = r * fma(-den, r, 2.0);
        const double t = copysign(b, d * b) * r;
        const double x = fma(t, t, 1.0);
        double z = __builtin_amdgcn_rsq(x);
        z = z * fma(-0.5 * x * z, z, 1.5);
        z = z * fma(-0.5 * x * z, z, 1.5);
        z = z * fma(-0.5 * x * z, z, 1.5);
        c = z;
        s = t * z;
    }
}

// init_v = false: V already holds an orthogonal matrix and A the matrix in THAT basis (warm start).
__device__ __forceinline__ void jacobi_eigh_lds(double *A, double *V, int m, double *rot, double *red, bool init_v = true) {
    const int tid = threadIdx.x;
    const int tk = tid & 15, tj = tid >> 4;
    const int half = m >> 1;
    if (init_v)
        for (int i = tj; i < m; i += 16)
            for (int j = tk; j < m; j += 16) V[i * m + j] = (i == j) ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, dg = 0.0;
        for (int i = tj; i < m; i += 16)
            for (int j = tk; j < m; j += 16) {
                const double v = A[i * m + j];
                if (i == j) dg = fma(v, v, dg);
                else off = fma(v, v, off);
            }
        off = block_sum<4>(off, red);
        dg = block_sum<4>(dg, red + 4);
        if (!(off > 1.0e-32 * dg)) break;  // converged (or NaN input)
        for (int step = 0; step < m - 1; ++step) {
            if (tid < half) {
                int p, q;
                pair_of(step, tid, m, p, q);
                double c, s;
                jacobi_rotation(A[p * m + p], A[q * m + q], A[p * m + q], c, s);
                rot[2 * tid] = c;
                rot[2 * tid + 1] = s;
            }
            __syncthreads();
            for (int kb = 0; kb < half; kb += 16)
                for (int k2b = kb; k2b < half; k2b += 16) {
                    const int k = kb + tj, k2 = k2b + tk;
                    if (k2 < half && k <= k2) {
                        int p, q, p2, q2;
                        pair_of(step, k, m, p, q);
                        pair_of(step, k2, m, p2, q2);
                        const double c = rot[2 * k], s = rot[2 * k + 1], c2 = rot[2 * k2], s2 = rot[2 * k2 + 1];
                        const double b00 = A[p * m + p2], b01 = A[p * m + q2], b10 = A[q * m + p2],
                                     b11 = A[q * m + q2];
                        const double r00 = c * b00 - s * b10, r01 = c * b01 - s * b11;   // J^T B
                        const double r10 = s * b00 + c * b10, r11 = s * b01 + c * b11;
                        const double n00 = c2 * r00 - s2 * r01, n01 = s2 * r00 + c2 * r01;  // . J2
                        const double n10 = c2 * r10 - s2 * r11, n11 = s2 * r10 + c2 * r11;
                        if (k == k2) {
                            const double o = 0.5 * (n01 + n10);  // ~1e-8 |a_pq|: the angle is approximate
                            A[p * m + p] = n00; A[p * m + q] = o; A[q * m + p] = o; A[q * m + q] = n11;
                        } else {
                            A[p * m + p2] = n00; A[p * m + q2] = n01; A[q * m + p2] = n10; A[q * m + q2] = n11;
                            A[p2 * m + p] = n00; A[q2 * m + p] = n01; A[p2 * m + q] = n10; A[q2 * m + q] = n11;
                        }
                    }
                }
            for (int ib = 0; ib < m; ib += 16)
                for (int kb = 0; kb < half; kb += 16) {
                    const int i = ib + tj, k = kb + tk;
                    if (i < m && k < half) {
                        int p, q;
                        pair_of(step, k, m, p, q);
                        const double c = rot[2 * k], s = rot[2 * k + 1];
                        const double vp = V[i * m + p], vq = V[i * m + q];
                        V[i * m + p] = c * vp - s * vq;
                        V[i * m + q] = s * vp + c * vq;
                    }
                }
            __syncthreads();
        }
    }
    __syncthreads();
}

// ------------------------------------------------------------------ one-sided Jacobi on ONE wave (m <= 32)
// Hestenes' method on the columns of G = A V (V orthogonal, A symmetric positive definite): the plane rotation of a
// column pair (p,q) that makes g_p . g_q = 0 is applied to the two columns; at convergence the columns of G are
// orthogonal, g_j = lambda_j v_j.  Same round-robin pairing as above, but a step needs no workgroup barrier and no
// hand-over of rotation parameters: the four lanes of a pair read their two columns (8 rows each, 16-byte LDS loads),
// reduce the three dot products among themselves with DPP, compute (c,s) redundantly and write the rotated columns
// back; LDS operations of one wave execute in order, so the next step sees them.  ~1/3 of the two-sided step's
// latency.  Columns are stored [col][row] with pitch kJwPitch; rows >= m are zero.  Called by wave 0 only.
// Convergence: |g_p.g_q| <= 1e-9 |g_p||g_q| for every pair BEFORE the rotations of a sweep.
constexpr int kJwPitch = 34;
constexpr int kJwMax = 32;

// Sum over the four lanes of a quad, every lane gets the total (DPP moves, common.hpp).
template <int CTRL, typename T>
__device__ __forceinline__ T dpp_quad(T v) { return dpp_move<CTRL>(v); }
constexpr int kQuadXor1 = 0xB1;   // quad_perm [1,0,3,2]
constexpr int kQuadXor2 = 0x4E;   // quad_perm [2,3,0,1]
template <typename T>
__device__ __forceinline__ T quad_sum(T v) {
    v += dpp_quad<kQuadXor1>(v);
    v += dpp_quad<kQuadXor2>(v);
    return v;
}


// Timing experiments (tools/micro/loewdin_time.py; build with EVC_DEBUG_STAMPS=1): workgroup 0 stamps the phases of
// the eigen-kernels with the 100 MHz wall clock and a cap on the sweeps of the wave solvers can be set.  Compiled out
// of the product library.
// Device code is not relocatable, so every unit that includes this header (loewdin.hip, subspace_small.hip) has its own
// copy of the three symbols; dbg_upload_max_sweeps / dbg_read below act on the including unit's copy.
#ifdef EVC_DEBUG_STAMPS
static __device__ long long g_dbg_stamp[64];
static __device__ double g_dbg_val[64];
static __device__ int g_dbg_max_sweeps = 0;   // > 0: cap on the sweeps of the wave solvers (EVC_DBG_MAX_SWEEPS)
#define EVC_STAMP(i_)                                                                   \
    do {                                                                                \
        if (blockIdx.x == 0 && threadIdx.x == 0) g_dbg_stamp[i_] = wall_clock64();      \
    } while (0)
#define EVC_DBGVAL(i_, v_)                                                              \
    do {                                                                                \
        if (blockIdx.x == 0 && threadIdx.x == 0) g_dbg_val[i_] = (double)(v_);          \
    } while (0)
#else
constexpr int g_dbg_max_sweeps = 0;
#define EVC_STAMP(i_) do { } while (0)
#define EVC_DBGVAL(i_, v_) do { } while (0)
#endif
#define EVC_FEW_STAMP(i_) EVC_STAMP(i_)

#ifdef EVC_DEBUG_STAMPS
static void dbg_upload_max_sweeps() {
    static bool done = false;
    if (done) return;
    done = true;
    if (const char *e = getenv("EVC_DBG_MAX_SWEEPS")) {
        const int v = atoi(e);
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_dbg_max_sweeps), &v, sizeof(int));
    }
}
// stamps / values written by workgroup 0 of this unit's last eigen-kernel
static int dbg_read(long long *stamps, double *vals, int n) {
    if (n > 64) n = 64;
    hipError_t e = hipMemcpyFromSymbol(stamps, HIP_SYMBOL(g_dbg_stamp), sizeof(long long) * n);
    if (e == hipSuccess) e = hipMemcpyFromSymbol(vals, HIP_SYMBOL(g_dbg_val), sizeof(double) * n);
    return (int)e;
}
#else
static inline void dbg_upload_max_sweeps() {}
#endif

__device__ __forceinline__ void jacobi_onesided_wave(double *Gc, int m) {
    const int lane = threadIdx.x & 63;
    const int k = lane >> 2, sub = lane & 3;
    const int half = m >> 1;
    const bool active = k < half;
    const int row0 = sub * 8;
    const int cap = g_dbg_max_sweeps > 0 ? g_dbg_max_sweeps : 40;
    for (int sweep = 0; sweep < cap; ++sweep) {
        bool bad = false;
        for (int step = 0; step < m - 1; ++step) {
            int p = 0, q = 1;
            if (active) pair_of(step, k, m, p, q);
            double *gp = Gc + p * kJwPitch + row0, *gq = Gc + q * kJwPitch + row0;
            double2 xg[4], yg[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                xg[u] = *reinterpret_cast<const double2 *>(gp + 2 * u);
                yg[u] = *reinterpret_cast<const double2 *>(gq + 2 * u);
            }
            double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                al = fma(xg[u].x, xg[u].x, fma(xg[u].y, xg[u].y, al));
                be = fma(yg[u].x, yg[u].x, fma(yg[u].y, yg[u].y, be));
                ga = fma(xg[u].x, yg[u].x, fma(xg[u].y, yg[u].y, ga));
            }
            al = quad_sum(al);
            be = quad_sum(be);
            ga = quad_sum(ga);
            // rotate when the columns are not yet orthogonal to working precision
            const double ab = al * be, g2 = ga * ga;
            const bool rot = active && (g2 > 1.0e-30 * ab);
            bad = bad || (active && g2 > 1.0e-18 * ab);
            if (rot) {
                // t = sgn(d) b / (|d| + sqrt(d^2 + b^2)), d = beta - alpha, b = 2 gamma (the smaller root)
                // (the angle only has to make g_p . g_q small: one Newton step on the seeds; c is refined to full
                // precision so that c^2 + s^2 = 1 to rounding and the columns keep their norms)
                const double d = be - al, b = 2.0 * ga;
                const double h2 = fma(d, d, b * b);
                double y = __builtin_amdgcn_rsq(h2);
                y = y * fma(-0.5 * h2 * y, y, 1.5);
                const double den = fabs(d) + h2 * y;
                double r = __builtin_amdgcn_rcp(den);
                r = r * fma(-den, r, 2.0);
                const double t = copysign(b, d * b == 0.0 ? b : d * b) * r;
                const double x = fma(t, t, 1.0);
                double z = __builtin_amdgcn_rsq(x);
                z = z * fma(-0.5 * x * z, z, 1.5);
                z = z * fma(-0.5 * x * z, z, 1.5);
                z = z * fma(-0.5 * x * z, z, 1.5);
                const double c = z, s = t * z;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    double2 a, b2;
                    a.x = c * xg[u].x - s * yg[u].x;
                    a.y = c * xg[u].y - s * yg[u].y;
                    b2.x = s * xg[u].x + c * yg[u].x;
                    b2.y = s * xg[u].y + c * yg[u].y;
                    *reinterpret_cast<double2 *>(gp + 2 * u) = a;
                    *reinterpret_cast<double2 *>(gq + 2 * u) = b2;
                }
            }
        }
        // every pair of this sweep was orthogonal to 1e-9 BEFORE its rotation: quadratic convergence leaves the
        // columns orthogonal to rounding after it, a confirming sweep is not needed
        if (__ballot(bad) == 0) break;
    }
}

// Eigen-decomposition of the symmetric m x m matrix A (LDS, both triangles) for m <= 32 through the wave kernel
// above: on return diag(A) holds the eigenvalues and V (row-major, V[i*m+j]) the eigenvectors as columns.
// shift: A + shift*I must be positive definite (0 for an overlap matrix): then the converged columns are
// g_j = lambda_j v_j with lambda_j = |g_j| > 0, so V = G diag(1/|g_j|) and no eigenvector matrix has to be carried
// through the rotations (its orthogonality is that of the columns of G, which is the convergence criterion).
// init_v = false: V holds an orthogonal start matrix and A the matrix in THAT basis (warm start), G0 = V (A + shift I).
// Gc: kJwMax x kJwPitch doubles of LDS.
__device__ __forceinline__ void jacobi_eigh_wave(double *A, double *V, int m, double shift, bool init_v, double *Gc, double *lam) {
    const int tid = threadIdx.x;
    for (int idx = tid; idx < kJwMax * kJwPitch; idx += kThreads) {
        const int j = idx / kJwPitch, i = idx - j * kJwPitch;
        double g = 0.0;
        if (i < m && j < m) {
            if (init_v) {
                g = A[i * m + j] + ((i == j) ? shift : 0.0);
            } else {
                double acc = shift * V[i * m + j];
                for (int kk = 0; kk < m; ++kk) acc = fma(V[i * m + kk], A[kk * m + j], acc);
                g = acc;
            }
        }
        Gc[idx] = g;
    }
    __syncthreads();
    if (tid < 64) jacobi_onesided_wave(Gc, m);
    __syncthreads();
    if (tid < m) {
        double nn = 0.0;
        for (int i = 0; i < m; ++i) nn = fma(Gc[tid * kJwPitch + i], Gc[tid * kJwPitch + i], nn);
        lam[tid] = sqrt(nn);
    }
    __syncthreads();
    for (int idx = tid; idx < m * m; idx += kThreads) {
        const int i = idx / m, j = idx - i * m;
        const double l = lam[j];
        // a zero column (the decoupled dummy dimension of an odd problem) keeps its unit vector
        V[idx] = l > 1.0e-300 ? Gc[j * kJwPitch + i] / l : (i == j ? 1.0 : 0.0);
        if (i == j) A[idx] = l - shift;
    }
    __syncthreads();
}

// ------------------------------------------------------------------ FP32 Jacobi + FP64 refinement (m <= 32)
// The FP64 wave Jacobi above is a chain of ~8 sweeps x (m-1) steps of ~1200 cycles each (f64 rsq/rcp seeds with
// Newton steps, twice the LDS bytes), and its last sweeps only square an error that is already tiny.  Two stages
// instead:
//  (1) the same one-sided Jacobi in FP32 (hardware v_sqrt/v_rcp/v_rsq_f32 without refinement, half the LDS traffic,
//      ~2.5x shorter steps), run until every column pair is orthogonal to 1e-5 before its rotation: eigenvectors to
//      ~1e-6;
//  (2) Ogita-Aishima refinement in FP64 (Japan J. Indust. Appl. Math. 35 (2018) 1007): with R = I - Z^T Z,
//      S = Z^T A Z, l_i = S_ii / (1 - R_ii),  E_ij = (S_ij + l_j R_ij) / (l_j - l_i)  (R_ij / 2 on the diagonal and
//      inside a cluster |l_i - l_j| <= delta),  Z <- Z + Z E  squares the error per pass: four small products on the
//      whole workgroup, one or two passes.
// Everything downstream (X = V f(s) V^T, the divided-difference response, the generalised eigenvectors) is a smooth
// function of invariant subspaces, so the arbitrary basis the cluster rule leaves inside a degenerate eigenspace is
// harmless -- as it is for LAPACK.  Returns false (A untouched) when the refinement does not contract: the caller
// falls back to the FP64 Jacobi.
constexpr int kJfPitch = 36;   // floats per column (16-byte aligned columns)

__device__ __forceinline__ void jacobi_onesided_wave_f32(float *Gf, int m) {
    const int lane = threadIdx.x & 63;
    const int k = lane >> 2, sub = lane & 3;
    const int half = m >> 1;
    const bool active = k < half;
    const int row0 = sub * 8;
    const int cap = g_dbg_max_sweeps > 0 ? g_dbg_max_sweeps : 30;
    for (int sweep = 0; sweep < cap; ++sweep) {
        bool bad = false;
        for (int step = 0; step < m - 1; ++step) {
            int p = 0, q = 1;
            if (active) pair_of(step, k, m, p, q);
            float *gp = Gf + p * kJfPitch + row0, *gq = Gf + q * kJfPitch + row0;
            float4 x0 = *reinterpret_cast<const float4 *>(gp), x1 = *reinterpret_cast<const float4 *>(gp + 4);
            float4 y0 = *reinterpret_cast<const float4 *>(gq), y1 = *reinterpret_cast<const float4 *>(gq + 4);
            float al = x0.x * x0.x, be = y0.x * y0.x, ga = x0.x * y0.x;
#define EVC_ACC(X_, Y_)          \
    al = fmaf(X_, X_, al);      \
    be = fmaf(Y_, Y_, be);      \
    ga = fmaf(X_, Y_, ga);
            EVC_ACC(x0.y, y0.y) EVC_ACC(x0.z, y0.z) EVC_ACC(x0.w, y0.w)
            EVC_ACC(x1.x, y1.x) EVC_ACC(x1.y, y1.y) EVC_ACC(x1.z, y1.z) EVC_ACC(x1.w, y1.w)
#undef EVC_ACC
            al = quad_sum(al);
            be = quad_sum(be);
            ga = quad_sum(ga);
            const float ab = al * be, g2 = ga * ga;
            const bool rot = active && (g2 > 1.0e-14f * ab);
            bad = bad || (active && g2 > 1.0e-10f * ab);
            if (rot) {
                const float d = be - al, b = 2.0f * ga;
                const float den = fabsf(d) + __builtin_sqrtf(fmaf(d, d, b * b));
                const float t = copysignf(b, d * b == 0.0f ? b : d * b) * __builtin_amdgcn_rcpf(den);
                const float c = __builtin_amdgcn_rsqf(fmaf(t, t, 1.0f)), s = t * c;
                float4 a0, a1, b0, b1;
#define EVC_ROT(F_)                         \
    a0.F_ = c * x0.F_ - s * y0.F_;          \
    b0.F_ = s * x0.F_ + c * y0.F_;          \
    a1.F_ = c * x1.F_ - s * y1.F_;          \
    b1.F_ = s * x1.F_ + c * y1.F_;
                EVC_ROT(x) EVC_ROT(y) EVC_ROT(z) EVC_ROT(w)
#undef EVC_ROT
                *reinterpret_cast<float4 *>(gp) = a0;
                *reinterpret_cast<float4 *>(gp + 4) = a1;
                *reinterpret_cast<float4 *>(gq) = b0;
                *reinterpret_cast<float4 *>(gq + 4) = b1;
            }
        }
        if (lane == 0) EVC_DBGVAL(20, sweep + 1);
        if (__ballot(bad) == 0) break;
    }
}

// max over the workgroup (NaN-propagating: a NaN input yields a NaN result); red: 4 doubles of LDS.
// Wave stage on DPP moves (quad xor 1, xor 2, row_half_mirror, row_mirror) + four readlanes, no LDS round trips.
__device__ __forceinline__ double nanmax(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double wave_max_nan(double v) {
    v = nanmax(v, dpp_quad<kQuadXor1>(v));
    v = nanmax(v, dpp_quad<kQuadXor2>(v));
    v = nanmax(v, dpp_quad<0x141>(v));   // row_half_mirror
    v = nanmax(v, dpp_quad<0x140>(v));   // row_mirror: every lane holds the maximum of its row of 16
    return nanmax(nanmax(readlane_f64(v, 0), readlane_f64(v, 16)), nanmax(readlane_f64(v, 32), readlane_f64(v, 48)));
}
__device__ __forceinline__ double block_max_nan(double v, double *red) {
    v = wave_max_nan(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    const double t = nanmax(nanmax(red[0], red[1]), nanmax(red[2], red[3]));
    __syncthreads();
    return t;
}
// two maxima with one pair of barriers (red: 8 doubles)
__device__ __forceinline__ void block_max_nan2(double &a, double &b, double *red) {
    a = wave_max_nan(a);
    b = wave_max_nan(b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[wave] = a;
        red[4 + wave] = b;
    }
    __syncthreads();
    a = nanmax(nanmax(red[0], red[1]), nanmax(red[2], red[3]));
    b = nanmax(nanmax(red[4], red[5]), nanmax(red[6], red[7]));
    __syncthreads();
}

}  // namespace evc
#include "tridiag_f32.hpp"   // (behind the DPP helpers it uses)
namespace evc {

// Ogita-Aishima refinement of approximate eigenvectors of the symmetric matrix Ap (pitch kRp).  On entry Z holds the
// start vectors as columns and Zt = Z^T (both pitch kRp, padding zero); B1, B2, B3: scratch matrices.  On success
// (the error contracted to rounding) returns true with Z / Zt pointing at the refined pair (two of the five buffers)
// and lam = eigenvalues; false when a pass does not contract (garbage, NaN or an unresolved cluster structure).
// Rows / columns nreal..m-1 are the decoupled dummy dimension.
__device__ __forceinline__ bool oa_refine(int m, int nreal, const double *Ap, double *&Z, double *&Zt, double *B1,
                                          double *B2, double *B3, double *lam, double *red, int max_pass) {
    const int tid = threadIdx.x;
    bool ok = false;
    double prev = 1.0e300;
    for (int pass = 0; pass < max_pass; ++pass) {
        // Wt = Zt A  (A symmetric: Wt[j][i] = sum_k Zt[j][k] A[i][k])
        if (pass == 0) EVC_STAMP(14);
        mm_rowrow(m, Zt, Ap, [&](int j, int i, double v) { B1[j * kRp + i] = v; });
        __syncthreads();
        if (pass == 0) EVC_STAMP(15);
        // S = Z^T W -> B2,  R = I - Z^T Z -> B3, in one pass over the rows of Zt
#ifdef EVC_SMALL_MM_MFMA
        {
            const int lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
            const int ti = wave >> 1, tj = wave & 1;
            if (16 * ti < m && 16 * tj < m) {   // wave-uniform
                const int i = 16 * ti + l15, j = 16 * tj + l15;
                const double *pr = Zt + (i < m ? i : 0) * kRp;
                const double *zr = Zt + (j < m ? j : 0) * kRp, *wr = B1 + (j < m ? j : 0) * kRp;
                d4 sa = {0.0, 0.0, 0.0, 0.0}, ra = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int kk = 0; kk < 8; ++kk)
                    if (4 * kk < m) {
                        const int k = 4 * kk + l4;
                        const bool kv = k < m;
                        const int kc = kv ? k : 0;
                        const double av = kv ? pr[kc] : 0.0;
                        sa = mfma_f64(av, kv ? wr[kc] : 0.0, sa);
                        ra = mfma_f64(av, kv ? zr[kc] : 0.0, ra);
                    }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ii = 16 * ti + l4 + 4 * r;
                    if (ii < m && j < m) {
                        B2[ii * kRp + j] = sa[r];
                        B3[ii * kRp + j] = (ii == j ? 1.0 : 0.0) - ra[r];
                    }
                }
            }
        }
#else
        {
            const int tk = tid & 15, tj = tid >> 4;
            const int ia = tj, ib = tj + 16, ja = tk, jb = tk + 16;
            const double *pa = Zt + (ia < m ? ia : 0) * kRp, *pb = Zt + (ib < m ? ib : 0) * kRp;
            const double *za = Zt + (ja < m ? ja : 0) * kRp, *zb = Zt + (jb < m ? jb : 0) * kRp;
            const double *wa = B1 + (ja < m ? ja : 0) * kRp, *wb = B1 + (jb < m ? jb : 0) * kRp;
            double s00 = 0, s01 = 0, s10 = 0, s11 = 0, r00 = 0, r01 = 0, r10 = 0, r11 = 0;
            const int m2 = (m + 1) & ~1;
#pragma unroll 2
            for (int k = 0; k < m2; k += 2) {
                const double2 a0 = *reinterpret_cast<const double2 *>(pa + k), a1 = *reinterpret_cast<const double2 *>(pb + k);
                const double2 y0 = *reinterpret_cast<const double2 *>(za + k), y1 = *reinterpret_cast<const double2 *>(zb + k);
                const double2 w0 = *reinterpret_cast<const double2 *>(wa + k), w1 = *reinterpret_cast<const double2 *>(wb + k);
                s00 = fma(a0.x, w0.x, s00); s00 = fma(a0.y, w0.y, s00);
                s01 = fma(a0.x, w1.x, s01); s01 = fma(a0.y, w1.y, s01);
                s10 = fma(a1.x, w0.x, s10); s10 = fma(a1.y, w0.y, s10);
                s11 = fma(a1.x, w1.x, s11); s11 = fma(a1.y, w1.y, s11);
                r00 = fma(a0.x, y0.x, r00); r00 = fma(a0.y, y0.y, r00);
                r01 = fma(a0.x, y1.x, r01); r01 = fma(a0.y, y1.y, r01);
                r10 = fma(a1.x, y0.x, r10); r10 = fma(a1.y, y0.y, r10);
                r11 = fma(a1.x, y1.x, r11); r11 = fma(a1.y, y1.y, r11);
            }
            if (ia < m && ja < m) { B2[ia * kRp + ja] = s00; B3[ia * kRp + ja] = (ia == ja ? 1.0 : 0.0) - r00; }
            if (ia < m && jb < m) { B2[ia * kRp + jb] = s01; B3[ia * kRp + jb] = -r01; }
            if (ib < m && ja < m) { B2[ib * kRp + ja] = s10; B3[ib * kRp + ja] = -r10; }
            if (ib < m && jb < m) { B2[ib * kRp + jb] = s11; B3[ib * kRp + jb] = (ib == jb ? 1.0 : 0.0) - r11; }
        }
#endif
        __syncthreads();
        if (pass == 0) EVC_STAMP(16);
        const double *S = B2, *R = B3;
        // (every wave evaluates the m Rayleigh quotients itself: its maximum needs no exchange, one barrier publishes lam)
        double lm = 0.0;
        {
            const int ln = tid & 63;
            if (ln < m) {
                lm = S[ln * kRp + ln] / (1.0 - R[ln * kRp + ln]);
                if (tid < m) lam[tid] = lm;
                lm = fabs(lm);
            }
        }
        const double lmax = wave_max_nan(lm);
        __syncthreads();
        if (pass == 0) EVC_STAMP(17);
        // E^T -> B1 (Wt is consumed).  E = R/2 + a, a antisymmetric: a_ij = sh / (l_j - l_i) to first order with
        // sh = S_ij + (l_i + l_j)/2 R_ij; evaluated as the tangent of the Jacobi angle of the 2 x 2 problem
        // [[l_i, sh], [sh, l_j]], which is the same number for well separated pairs and stays bounded (|a| <= 1) for
        // close ones -- no cluster threshold.  Elements below the rounding floor are not rotated (an exactly
        // degenerate eigenspace keeps whatever orthonormal basis it has).  Convergence measure: the rotation, but
        // never more than |sh| relative to 1e-8 max|l| (a large rotation inside a numerically degenerate pair moves
        // nothing that any smooth function of A can see), and the symmetric part.
        // rounding leaves ~m eps max|l| in every element of S: below `conv_floor` an element says nothing about
        // convergence, and if the rotation it asks for is large (a numerically degenerate pair: any orthonormal basis of
        // its span is as good as any other) it is not applied at all; small rotations are applied down to `rot_floor`,
        // which is what resolves eigenvectors of tiny eigenvalues as far as the arithmetic allows.  A large rotation
        // of a significant element (a close pair found badly mixed) is limited to 0.3 per pass: the update is first
        // order, and the symmetric part repairs the t^2 loss of orthogonality in the next pass.
        const double rot_floor = 1.8e-15 * lmax, conv_floor = 1.5e-14 * (double)m * lmax;
        double emax = 0.0, rmax = 0.0;
        for (int idx = tid; idx < m * 32; idx += kThreads) {
            const int i = idx >> 5, j = idx & 31;
            if (j < m) {
                const double rv = R[i * kRp + j];
                double e = 0.5 * rv, meas = fabs(e);
                rmax = nanmax(rmax, meas);
                // (the decoupled dummy dimension of an odd problem has S_ij = R_ij = 0 exactly: no rotation -- its
                //  "eigenvalue" 0 may sit arbitrarily close to a real one)
                if (i != j && i < nreal && j < nreal) {
                    const int lo = i < j ? i : j, hi = i < j ? j : i;
                    const double d = lam[hi] - lam[lo];
                    const double sh = S[i * kRp + j] + 0.5 * (lam[i] + lam[j]) * rv;
                    double t = 0.0;
                    if (fabs(sh) > rot_floor || sh != sh) {
                        const double hd = 0.5 * d, rt = sqrt(fma(hd, hd, sh * sh));
                        t = sh / (hd + (hd < 0.0 ? -rt : rt));
                        if (fabs(sh) > conv_floor || sh != sh) {
                            meas = nanmax(meas, fabs(t));
                            t = t > 0.3 ? 0.3 : (t < -0.3 ? -0.3 : t);
                        } else if (fabs(t) > 1.0e-3) {
                            t = 0.0;
                        }
                    }
                    e += (i < j) ? t : -t;
                }
                B1[j * kRp + i] = e;
                emax = nanmax(emax, meas);
            }
        }
        if (pass == 0) EVC_STAMP(18);
        block_max_nan2(emax, rmax, red);
        EVC_STAMP(3 + pass);
        EVC_DBGVAL(pass, emax);
        // give up on NaNs, on vectors that are far from orthonormal (the first-order update cannot repair that) and
        // when the passes stop contracting; large ROTATIONS alone are fine: inside an eigenspace that is degenerate
        // to working precision they are arbitrary and harmless, elsewhere they proceed 0.3 rad per pass
        if (!(rmax < 0.5) || emax != emax || (pass >= 3 && !(emax < prev))) break;
        // Zt' = Zt + E^T Z^T: Zt'[j][i] = Zt[j][i] + sum_k Et[j][k] Z[i][k]; stored both ways (S and R are consumed)
        mm_rowrow(m, B1, Z, [&](int j, int i, double v) {
            const double z = Zt[j * kRp + i] + v;
            B2[j * kRp + i] = z;
            B3[i * kRp + j] = z;
        });
        __syncthreads();
        double *t = Zt;
        Zt = B2;
        B2 = t;
        t = Z;
        Z = B3;
        B3 = t;
        prev = emax;
        if (emax < 3.0e-8) {   // the pass just applied leaves an error of ~emax^2
            ok = true;
            // ... in the eigenvector directions; the rotations applied below the convergence floor (tiny eigenvalue
            // gaps: t = noise-level element / gap can reach 1e-3) still cost t^2 of orthogonality, which one
            // symmetric-only step Z <- Z (I + R / 2) repairs
            {
                mm_rowrow(m, Zt, Zt, [&](int i, int j, double v) { B1[j * kRp + i] = 0.5 * ((i == j ? 1.0 : 0.0) - v); });
                __syncthreads();
                mm_rowrow(m, B1, Z, [&](int j, int i, double v) {
                    const double z = Zt[j * kRp + i] + v;
                    B2[j * kRp + i] = z;
                    B3[i * kRp + j] = z;
                });
                __syncthreads();
                double *t2 = Zt;
                Zt = B2;
                B2 = t2;
                t2 = Z;
                Z = B3;
                B3 = t2;
            }
            break;
        }
    }
    return ok;
}

// Eigen-decomposition of the symmetric m x m matrix A (LDS, pitch m, both triangles; m <= 32, m even, a trailing
// decoupled dummy dimension allowed): on return diag(A) = eigenvalues, V (pitch m) = eigenvectors as columns.
//   warm: V holds the eigenvectors of a nearby problem (any garbage is detected): refinement starts from them;
//   otherwise, or when that does not contract: FP32 tridiagonal start, then FP32 Jacobi start, then FP64 Jacobi.
//   nreal: rows/columns nreal..m-1 are the decoupled dummy dimension of an odd problem.
// A + shift I must be positive definite.  Scratch R6: six matrices of kRsz doubles; Gc: kJwMax x kJwPitch doubles
// (also serves as the FP32 column buffer); lam: m; red: 8 doubles.
__device__ __forceinline__ void eigh_small(double *A, double *V, int m, int nreal, double shift, bool warm, int fast,
                                           double *R6, double *Gc, double *lam, double *red) {
    const int tid = threadIdx.x;
    bool ok = false;
    const bool tri = fast > 1;   // fast: 0 FP64 Jacobi, 1 FP32 Jacobi + refinement, 2 FP32 tridiagonal start first
    if (fast) {
        double *Ap = R6, *Z = R6 + kRsz, *Zt = R6 + 2 * kRsz, *B1 = R6 + 3 * kRsz, *B2 = R6 + 4 * kRsz, *B3 = R6 + 5 * kRsz;
        float *Gf = reinterpret_cast<float *>(Gc);
        EVC_STAMP(0);
        for (int idx = tid; idx < kRsz; idx += kThreads) {
            const int i = idx / kRp, j = idx - i * kRp;
            Ap[idx] = (i < m && j < m) ? A[i * m + j] : 0.0;
        }
        // ONE refinement call site, fed by up to three kinds of start vectors in turn (a loop that is not unrolled: every
        // inlined copy of the refinement is ~15 KB of code, and the instruction cache of a CU pair holds 64 KB):
        //   stage 0  the previous call's eigenvectors (warm start);
        //   stage 1  FP32 tridiagonalisation + multisection + twisted factorisation (tridiag_eig_wg_f32);
        //   stage 2  FP32 one-sided Jacobi on G0 = (A + shift I) / max|.|.
        double amax = 0.0;
        bool sane = true, have_amax = false;
#pragma unroll 1
        for (int stage = warm ? 0 : 1; stage < 3 && !ok && sane; ++stage) {
            if (stage == 1 && !tri) continue;
            if (stage >= 1 && !have_amax) {
                for (int idx = tid; idx < m * m; idx += kThreads) {
                    const int i = idx / m, j = idx - i * m;
                    amax = nanmax(amax, fabs(A[idx] + (i == j ? shift : 0.0)));
                }
                amax = block_max_nan(amax, red);
                have_amax = true;
                sane = amax > 0.0 && amax < 1.0e300;   // (zero, NaN or Inf input: left to the FP64 path)
                if (!sane) break;
            }
            if (stage == 0) {
                for (int idx = tid; idx < kRsz; idx += kThreads) {
                    const int i = idx / kRp, j = idx - i * kRp;
                    const bool in = i < m && j < m;
                    Z[idx] = in ? V[i * m + j] : 0.0;
                    Zt[idx] = in ? V[j * m + i] : 0.0;
                }
                __syncthreads();
            } else if (stage == 1) {
                // FP32 start 1: tridiagonalisation + multisection + twisted factorisation (scratch: the B buffers)
                float *Af = reinterpret_cast<float *>(B1), *scr = Af + 32 * kTp, *zn = scr + 32 * 32 * 5 + 5 * 32;
                float *Zf = Gf;
                const double sc = 1.0 / amax;
                for (int idx = tid; idx < 32 * kTp; idx += kThreads) {
                    const int i = idx / kTp, j = idx - i * kTp;
                    float v = 0.0f;
                    if (i < nreal && j < nreal) v = (float)(A[i * m + j] * sc);
                    else if (i == j && i < m) v = 40.0f;   // decoupled dummy dimension: an eigenvalue outside the spectrum
                    Af[idx] = v;
                }
                __syncthreads();
                EVC_STAMP(1);
                tridiag_eig_wg_f32(Af, m, Zf, zn, scr, reinterpret_cast<int *>(Gf + 34 * 32));
                __syncthreads();
                EVC_STAMP(2);
                for (int idx = tid; idx < kRsz; idx += kThreads) {
                    const int i = idx / kRp, j = idx - i * kRp;   // Zt[i][j] = component j of eigenvector i
                    Zt[idx] = (i < m && j < m) ? (double)Zf[i * kZfp + j] * (double)zn[i] : 0.0;
                }
                __syncthreads();
                for (int idx = tid; idx < kRsz; idx += kThreads) {
                    const int i = idx / kRp, j = idx - i * kRp;
                    Z[idx] = (i < m && j < m) ? Zt[j * kRp + i] : 0.0;
                }
                __syncthreads();
            } else {
                // FP32 start 2: one-sided Jacobi on G0 = (A + shift I) / max|.|, column-major with pitch kJfPitch
                const double sc = 1.0 / amax;
                for (int idx = tid; idx < kJwMax * kJfPitch; idx += kThreads) {
                    const int j = idx / kJfPitch, i = idx - j * kJfPitch;
                    Gf[idx] = (i < m && j < m) ? (float)((A[i * m + j] + (i == j ? shift : 0.0)) * sc) : 0.0f;
                }
                __syncthreads();
                if (tid < 64) jacobi_onesided_wave_f32(Gf, m);
                __syncthreads();
                // Z0 = normalised columns (a zero column = the decoupled dummy dimension keeps its unit vector)
                if (tid < m) {
                    double nn = 0.0;
                    for (int i = 0; i < m; ++i) nn = fma((double)Gf[tid * kJfPitch + i], (double)Gf[tid * kJfPitch + i], nn);
                    lam[tid] = nn > 1.0e-60 ? 1.0 / sqrt(nn) : 0.0;
                }
                __syncthreads();
                for (int idx = tid; idx < kRsz; idx += kThreads) {
                    const int i = idx / kRp, j = idx - i * kRp;   // Zt[i][j] = Z[j][i] = component j of eigenvector i
                    double v = 0.0;
                    if (i < m && j < m) v = lam[i] > 0.0 ? (double)Gf[i * kJfPitch + j] * lam[i] : (i == j ? 1.0 : 0.0);
                    Zt[idx] = v;
                }
                __syncthreads();
                for (int idx = tid; idx < kRsz; idx += kThreads) {
                    const int i = idx / kRp, j = idx - i * kRp;
                    Z[idx] = (i < m && j < m) ? Zt[j * kRp + i] : 0.0;
                }
                __syncthreads();
            }
            ok = oa_refine(m, nreal, Ap, Z, Zt, B1, B2, B3, lam, red, 10);
            EVC_DBGVAL(21, ok ? 1.0 : 0.0);
            if (!ok) {   // the buffers may have been permuted: re-establish the roles
                Z = R6 + kRsz; Zt = R6 + 2 * kRsz; B1 = R6 + 3 * kRsz; B2 = R6 + 4 * kRsz; B3 = R6 + 5 * kRsz;
            }
        }
        EVC_STAMP(10);
        if (ok) {
            for (int idx = tid; idx < m * m; idx += kThreads) {
                const int i = idx / m, j = idx - i * m;
                V[idx] = Z[i * kRp + j];
            }
            if (tid < m) A[tid * m + tid] = lam[tid];
            __syncthreads();
        }
    }
    if (!ok) jacobi_eigh_wave(A, V, m, shift, true, Gc, lam);
}

// Warm start (EVC_FLAG_WARM_START): `prev` holds the eigenvectors of the previous, nearby problem.  If they
// are orthonormal to 1e-8 (a stale or never-written buffer is not), V <- prev (padded with the identity) and
// A <- V^T A V, which is nearly diagonal, so the sweeps that follow are two or three instead of seven or eight.
// Returns whether the rotation was applied (uniform over the workgroup).  Tmp: n*n doubles of LDS.
__device__ __forceinline__ bool warm_start_rotate(double *A, double *V, double *Tmp, int n, int m, const double *__restrict__ prev,
                                  int ldp, double *red) {
    const int tid = threadIdx.x;
    for (int idx = tid; idx < m * m; idx += kThreads) {
        const int i = idx / m, j = idx - i * m;
        V[idx] = (i < n && j < n) ? prev[i * ldp + j] : (i == j ? 1.0 : 0.0);
    }
    __syncthreads();
    mm16(n, [&](int i, int k) { return V[k * m + i]; }, [&](int k, int j) { return V[k * m + j]; },
         [&](int i, int j, double v) { Tmp[i * n + j] = v - (i == j ? 1.0 : 0.0); });
    __syncthreads();
    double dev = 0.0;
    for (int idx = tid; idx < n * n; idx += kThreads) dev = fma(Tmp[idx], Tmp[idx], dev);
    dev = block_sum<4>(dev, red);
    if (!(dev < 1.0e-16)) return false;  // also catches NaN
    mm16(n, [&](int i, int k) { return A[i * m + k]; }, [&](int k, int j) { return V[k * m + j]; },
         [&](int i, int j, double v) { Tmp[i * n + j] = v; });
    __syncthreads();
    mm16(n, [&](int i, int k) { return V[k * m + i]; }, [&](int k, int j) { return Tmp[k * n + j]; },
         [&](int i, int j, double v) { A[i * m + j] = v; });
    __syncthreads();
    for (int idx = tid; idx < n * n; idx += kThreads) {  // exact symmetry, as the rotations assume
        const int i = idx / n, j = idx - i * n;
        if (i > j) {
            const double v = 0.5 * (A[i * m + j] + A[j * m + i]);
            A[i * m + j] = v;
            A[j * m + i] = v;
        }
    }
    __syncthreads();
    return true;
}

static size_t jacobi_aux_bytes(int m) {
    return sizeof(double) * (size_t)(2 * m + 8) + 32 +
           (m <= kJwMax ? sizeof(double) * ((size_t)kJwMax * kJwPitch + (size_t)6 * kRsz) + 16 : 0);
}

}  // namespace evc
