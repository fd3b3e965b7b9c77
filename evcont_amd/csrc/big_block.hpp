// What the 1024-thread kernels share (subspace_big.hip, loewdin_big.hip): block-wide reductions over the 16 waves, the
// "row . row" product on the FP64 matrix cores, and the one-sided (Hestenes) Jacobi on the columns of a matrix.
#pragma once
#include "common.hpp"

namespace evc {

constexpr int kBT = 1024;   // threads of the workgroup
constexpr int kBW = kBT / 64;

// Phase stamps of workgroup 0 (tools/micro/subspace_time.py --stamps; library built with EVC_DEBUG_STAMPS=1).
// Device code is not relocatable, so every unit that includes this header has its own copy of the two symbols (as with
// pt_stamps.hpp); evc_debug_read_big reads subspace_big.hip's copy -- big_jacobi's sweep count of a loewdin_big_kernel
// launch goes to loewdin_big.hip's copy, which has no reader.
#ifdef EVC_DEBUG_STAMPS
[[maybe_unused]] static __device__ long long g_big_stamp[16];
[[maybe_unused]] static __device__ double g_big_val[16];
#define EVC_BSTAMP(i_)                                                                  \
    do {                                                                                \
        if (blockIdx.x == 0 && threadIdx.x == 0) g_big_stamp[i_] = wall_clock64();      \
    } while (0)
#define EVC_BVAL(i_, v_)                                                                \
    do {                                                                                \
        if (blockIdx.x == 0 && threadIdx.x == 0) g_big_val[i_] = (double)(v_);          \
    } while (0)
#else
#define EVC_BSTAMP(i_) do { } while (0)
#define EVC_BVAL(i_, v_) do { } while (0)
#endif

__device__ __forceinline__ double sum8(double v) {    // over the 8 lanes of a half DPP row, every lane gets the total
    v += dpp_move<0xB1>(v);
    v += dpp_move<0x4E>(v);
    v += dpp_move<0x141>(v);
    return v;
}
__device__ __forceinline__ double sum16(double v) {   // over the 16 lanes of a DPP row
    v = sum8(v);
    v += dpp_move<0x140>(v);
    return v;
}

// block-wide reductions over the 16 waves (red: kBW doubles of LDS); all threads get the result
__device__ __forceinline__ double big_block_sum(double v, double *red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kBW; ++w) t += red[w];
    __syncthreads();
    return t;
}
__device__ __forceinline__ double big_nanmax(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double big_block_max(double v, double *red) {   // NaN-propagating
    v = big_nanmax(v, dpp_move<0xB1>(v));
    v = big_nanmax(v, dpp_move<0x4E>(v));
    v = big_nanmax(v, dpp_move<0x141>(v));
    v = big_nanmax(v, dpp_move<0x140>(v));
    v = big_nanmax(big_nanmax(readlane_f64(v, 0), readlane_f64(v, 16)), big_nanmax(readlane_f64(v, 32), readlane_f64(v, 48)));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red[0];
#pragma unroll
    for (int w = 1; w < kBW; ++w) t = big_nanmax(t, red[w]);
    __syncthreads();
    return t;
}
__device__ __forceinline__ bool big_block_any(bool b, double *red) {
    const unsigned long long m = __ballot(b);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m ? 1.0 : 0.0;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kBW; ++w) t += red[w];
    __syncthreads();
    return t != 0.0;
}

// D[i][j] = sum_k P[i][k] Q[j][k], i, j, k < Tp (Tp a multiple of 16; pitches even, rows 16-byte aligned, padding zero).
// v_mfma_f64_16x16x4_f64: A[i][k]: lane l holds i = l & 15, k slot l >> 4; B the same with j; D[i][j]: j = l & 15,
// i = (l >> 4) + 4 reg.  A lane reads the two adjacent columns 8 kk + 2 (l >> 4), +1 of "its" row with one 16-byte load
// and feeds .x / .y to two MFMAs (the K slot of a lane may be any column as long as A and B agree).
template <typename Store>
__device__ __forceinline__ void big_mm_rr(int Tp, const double *__restrict__ P, int ldp, const double *__restrict__ Q,
                                          int ldq, Store store) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int nt = Tp >> 4;
    for (int t = wave; t < nt * nt; t += kBW) {
        const int ti = t / nt, tj = t - ti * nt;
        const double *pr = P + (size_t)(16 * ti + l15) * ldp + 2 * l4;
        const double *qr = Q + (size_t)(16 * tj + l15) * ldq + 2 * l4;
        d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int k = 0; k < Tp; k += 8) {
            const double2 av = *reinterpret_cast<const double2 *>(pr + k);
            const double2 bv = *reinterpret_cast<const double2 *>(qr + k);
            acc = mfma_f64(av.x, bv.x, acc);
            acc = mfma_f64(av.y, bv.y, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) store(16 * ti + l4 + 4 * r, 16 * tj + l15, acc[r]);
    }
}

__device__ __forceinline__ void big_pair_of(int step, int k, int m, int &p, int &q) {   // round-robin tournament
    const int w = m - 1;
    p = step + k;
    if (p >= w) p -= w;
    if (k == 0) p = w;
    q = step + w - k;
    if (q >= w) q -= w;
}

// One-sided Jacobi on the m columns (m even) of G, stored column-major with pitch Pj (a multiple of 32; rows >= the
// matrix size are zero).  Pair k of a step belongs to the 16 lanes [16 k, 16 k + 16): lane s owns rows 2 s, 2 s + 1
// (+ 32 u) -- the 16 lanes of a pair read 256 contiguous bytes.  Convergence: every pair orthogonal to 1e-9 BEFORE its
// rotation in a sweep (the rotations of that sweep then leave ~1e-18).
__device__ __forceinline__ void big_jacobi(double *G, int m, int Pj, double *red) {
    const int tid = threadIdx.x, s = tid & 15;
    const int half = m >> 1, nu = Pj >> 5;
    const int npass = (half + (kBT / 16) - 1) / (kBT / 16);   // 1 for m <= 128
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool bad = false;
        for (int step = 0; step < m - 1; ++step) {
            for (int pass = 0; pass < npass; ++pass) {
                const int k = (tid >> 4) + pass * (kBT / 16);
                if (k < half) {   // uniform over the DPP row
                    int p, q;
                    big_pair_of(step, k, m, p, q);
                    double *gp = G + (size_t)p * Pj + 2 * s, *gq = G + (size_t)q * Pj + 2 * s;
                    double al = 0.0, be = 0.0, ga = 0.0;
                    double2 x[4], y[4];   // the whole share of this lane when Pj <= 128 (the LDS-resident case)
#pragma unroll
                    for (int u = 0; u < 4; ++u) x[u] = y[u] = make_double2(0.0, 0.0);
                    for (int u0 = 0; u0 < nu; u0 += 4) {
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (u0 + u < nu) {
                                x[u] = *reinterpret_cast<const double2 *>(gp + 32 * (u0 + u));
                                y[u] = *reinterpret_cast<const double2 *>(gq + 32 * (u0 + u));
                            }
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (u0 + u < nu) {
                                al = fma(x[u].x, x[u].x, fma(x[u].y, x[u].y, al));
                                be = fma(y[u].x, y[u].x, fma(y[u].y, y[u].y, be));
                                ga = fma(x[u].x, y[u].x, fma(x[u].y, y[u].y, ga));
                            }
                    }
                    al = sum16(al);
                    be = sum16(be);
                    ga = sum16(ga);
                    const double ab = al * be, g2 = ga * ga;
                    const bool rot = g2 > 1.0e-30 * ab;
                    bad = bad || (g2 > 1.0e-18 * ab);
                    if (rot) {   // uniform over the row
                        // t = sgn(d) b / (|d| + sqrt(d^2 + b^2)), d = beta - alpha, b = 2 gamma (the smaller root); the
                        // angle only has to make g_p . g_q small, c is refined to full precision (c^2 + s^2 = 1)
                        const double d = be - al, b = 2.0 * ga;
                        const double h2 = fma(d, d, b * b);
                        double yv = __builtin_amdgcn_rsq(h2);
                        yv = yv * fma(-0.5 * h2 * yv, yv, 1.5);
                        const double den = fabs(d) + h2 * yv;
                        double r = __builtin_amdgcn_rcp(den);
                        r = r * fma(-den, r, 2.0);
                        const double t = copysign(b, d * b == 0.0 ? b : d * b) * r;
                        const double xx = fma(t, t, 1.0);
                        double z = __builtin_amdgcn_rsq(xx);
                        z = z * fma(-0.5 * xx * z, z, 1.5);
                        z = z * fma(-0.5 * xx * z, z, 1.5);
                        z = z * fma(-0.5 * xx * z, z, 1.5);
                        const double c = z, sn = t * z;
                        if (nu <= 4) {   // uniform: rotate the registers
#pragma unroll
                            for (int u = 0; u < 4; ++u)
                                if (u < nu) {
                                    double2 a2, b2;
                                    a2.x = c * x[u].x - sn * y[u].x;
                                    a2.y = c * x[u].y - sn * y[u].y;
                                    b2.x = sn * x[u].x + c * y[u].x;
                                    b2.y = sn * x[u].y + c * y[u].y;
                                    *reinterpret_cast<double2 *>(gp + 32 * u) = a2;
                                    *reinterpret_cast<double2 *>(gq + 32 * u) = b2;
                                }
                        } else {
                            for (int u = 0; u < nu; ++u) {
                                const double2 xv = *reinterpret_cast<const double2 *>(gp + 32 * u);
                                const double2 yw = *reinterpret_cast<const double2 *>(gq + 32 * u);
                                double2 a2, b2;
                                a2.x = c * xv.x - sn * yw.x;
                                a2.y = c * xv.y - sn * yw.y;
                                b2.x = sn * xv.x + c * yw.x;
                                b2.y = sn * xv.y + c * yw.y;
                                *reinterpret_cast<double2 *>(gp + 32 * u) = a2;
                                *reinterpret_cast<double2 *>(gq + 32 * u) = b2;
                            }
                        }
                    }
                }
            }
            __syncthreads();
        }
        EVC_BVAL(0, sweep + 1);
        if (!big_block_any(bad, red)) break;
    }
}

// (Two blocks around big_jacobi stand in both kernels: the orthonormality check of the warm-start vectors and the loop
// "column norm -> eigenvalue, normalise the column".  As helpers here, in every spelling tried, each changed the
// instructions of one of the kernels: tools/isa_diff.py, a branch polarity and the order within a block-wide sum.)

}  // namespace evc
