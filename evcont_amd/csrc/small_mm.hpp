// Small matrix products of the single-workgroup dense kernels (loewdin.hip, subspace_small.hip, grad_tail.hip): matrices
// of up to 96 x 96 in LDS, 256 threads used as four waves (FP64 matrix cores) or as a 16 x 16 grid (tj = row group,
// tk = column group).  Every global operand is staged into LDS with coalesced loads first and inner loops carry no
// integer division.
#pragma once
#include "common.hpp"

namespace evc {

constexpr int kThreads = 256;

// ------------------------------------------------------------------ small LDS matmul
// C[i][j] = sum_k a(i,k) * b(k,j),  i,j < n;  thread (tj,tk) owns i = tj+16*, j = tk+16*.
// Small products on the FP64 matrix cores (n <= 64; up to 32: wave w of the workgroup owns the 16 x 16 output tile
// (w >> 1, w & 1), beyond: sixteen tiles round-robin); operand maps of v_mfma_f64_16x16x4_f64: A[i][k]: lane l holds i = l & 15, k = l >> 4; B[k][j]:
// k = l >> 4, j = l & 15; D[i][j]: j = l & 15, i = (l >> 4) + 4 reg.  One eighth of the LDS traffic of the 2 x 2
// register-blocked vector version (which was LDS-bandwidth bound: ~1 us per 32^3 product against ~0.3 us).
// EVC_SMALL_MM_VALU (build flag): the vector version everywhere.
#ifndef EVC_SMALL_MM_VALU
#define EVC_SMALL_MM_MFMA 1
#endif

// C[i][j] = sum_k a(i,k) b(k,j), i, j, k < n; operands through accessors, result through store(i, j, value).
template <typename FA, typename FB, typename FC>
__device__ __forceinline__ void mm16(int n, FA a, FB b, FC store) {
#ifdef EVC_SMALL_MM_MFMA
    if (n <= 32) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
        const int ti = wave >> 1, tj = wave & 1;
        if (16 * ti < n && 16 * tj < n) {   // wave-uniform
            const int i = 16 * ti + l15, j = 16 * tj + l15;
            const int ic = i < n ? i : 0, jc = j < n ? j : 0;   // (rows / columns beyond n: computed on row 0, never stored)
            d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 8; ++kk)
                if (4 * kk < n) {
                    const int k = 4 * kk + l4;
                    const bool kv = k < n;
                    const int kc = kv ? k : 0;
                    const double av = a(ic, kc), bv = b(kc, jc);
                    acc = mfma_f64(kv ? av : 0.0, kv ? bv : 0.0, acc);
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ii = 16 * ti + l4 + 4 * r;
                if (ii < n && j < n) store(ii, j, acc[r]);
            }
        }
        return;
    }
    if (n <= 64) {   // up to sixteen tiles, dealt round-robin to the four waves, K up to 64
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
        const int nt = (n + 15) >> 4;
        for (int t = wave; t < nt * nt; t += kThreads / 64) {   // wave-uniform
            const int ti = t / nt, tj = t - ti * nt;
            const int i = 16 * ti + l15, j = 16 * tj + l15;
            const int ic = i < n ? i : 0, jc = j < n ? j : 0;
            d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 16; ++kk)
                if (4 * kk < n) {
                    const int k = 4 * kk + l4;
                    const bool kv = k < n;
                    const int kc = kv ? k : 0;
                    const double av = a(ic, kc), bv = b(kc, jc);
                    acc = mfma_f64(kv ? av : 0.0, kv ? bv : 0.0, acc);
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ii = 16 * ti + l4 + 4 * r;
                if (ii < n && j < n) store(ii, j, acc[r]);
            }
        }
        return;
    }
#endif
    const int tk = threadIdx.x & 15, tj = threadIdx.x >> 4;
    for (int i0 = 0; i0 < n; i0 += 32)
        for (int j0 = 0; j0 < n; j0 += 32) {
            const int ia = i0 + tj, ib = i0 + tj + 16, ja = j0 + tk, jb = j0 + tk + 16;
            const bool via = ia < n, vib = ib < n, vja = ja < n, vjb = jb < n;
            const int ia_ = via ? ia : 0, ib_ = vib ? ib : 0, ja_ = vja ? ja : 0, jb_ = vjb ? jb : 0;
            double c00 = 0.0, c01 = 0.0, c10 = 0.0, c11 = 0.0;
            for (int k = 0; k < n; ++k) {
                const double a0 = a(ia_, k), a1 = a(ib_, k);
                const double b0 = b(k, ja_), b1 = b(k, jb_);
                c00 = fma(a0, b0, c00);
                c01 = fma(a0, b1, c01);
                c10 = fma(a1, b0, c10);
                c11 = fma(a1, b1, c11);
            }
            if (via && vja) store(ia, ja, c00);
            if (via && vjb) store(ia, jb, c01);
            if (vib && vja) store(ib, ja, c10);
            if (vib && vjb) store(ib, jb, c11);
        }
}

__device__ __forceinline__ void copy_to_lds(double *dst, const double *__restrict__ src, int count) {
    for (int idx = threadIdx.x; idx < count; idx += kThreads) dst[idx] = src[idx];
}

// ---- refinement on the whole workgroup: matrices of up to 32 x 32 in LDS with row pitch kRp ------------------
// C[i][j] = sum_k P[i][k] Q[j][k] ("row . row": both operands are read along contiguous rows with 16-byte LDS loads;
// 16 consecutive rows at pitch 34 doubles fall on 16 different 4-bank groups).  Thread (tj,tk) of the 16 x 16 grid owns
// i in {tj, tj+16}, j in {tk, tk+16}; rows >= m are read as row 0 and their results dropped by the caller's store.
constexpr int kRp = 34;
constexpr int kRsz = 32 * kRp;   // doubles per matrix

template <typename Store>
__device__ __forceinline__ void mm_rowrow(int m, const double *__restrict__ P, const double *__restrict__ Q, Store store) {
#ifdef EVC_SMALL_MM_MFMA
    // (both fragments are "row l & 15, columns 4 kk + (l >> 4)" reads of a pitch-kRp matrix)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int ti = wave >> 1, tj = wave & 1;
    if (16 * ti >= m || 16 * tj >= m) return;   // wave-uniform
    const int i = 16 * ti + l15, j = 16 * tj + l15;
    const double *pr = P + (i < m ? i : 0) * kRp, *qr = Q + (j < m ? j : 0) * kRp;
    d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 8; ++kk)
        if (4 * kk < m) {
            const int k = 4 * kk + l4;
            const bool kv = k < m;
            const double av = pr[kv ? k : 0], bv = qr[kv ? k : 0];
            acc = mfma_f64(kv ? av : 0.0, kv ? bv : 0.0, acc);
        }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ii = 16 * ti + l4 + 4 * r;
        if (ii < m && j < m) store(ii, j, acc[r]);
    }
#else
    const int tk = threadIdx.x & 15, tj = threadIdx.x >> 4;
    const int ia = tj, ib = tj + 16, ja = tk, jb = tk + 16;
    const double *pa = P + (ia < m ? ia : 0) * kRp, *pb = P + (ib < m ? ib : 0) * kRp;
    const double *qa = Q + (ja < m ? ja : 0) * kRp, *qb = Q + (jb < m ? jb : 0) * kRp;
    double c00 = 0, c01 = 0, c10 = 0, c11 = 0;
    const int m2 = (m + 1) & ~1;   // columns m..m2-1 are zero padding
#pragma unroll 4
    for (int k = 0; k < m2; k += 2) {
        const double2 a0 = *reinterpret_cast<const double2 *>(pa + k), a1 = *reinterpret_cast<const double2 *>(pb + k);
        const double2 b0 = *reinterpret_cast<const double2 *>(qa + k), b1 = *reinterpret_cast<const double2 *>(qb + k);
        c00 = fma(a0.x, b0.x, c00); c00 = fma(a0.y, b0.y, c00);
        c01 = fma(a0.x, b1.x, c01); c01 = fma(a0.y, b1.y, c01);
        c10 = fma(a1.x, b0.x, c10); c10 = fma(a1.y, b0.y, c10);
        c11 = fma(a1.x, b1.x, c11); c11 = fma(a1.y, b1.y, c11);
    }
    if (ia < m && ja < m) store(ia, ja, c00);
    if (ia < m && jb < m) store(ia, jb, c01);
    if (ib < m && ja < m) store(ib, ja, c10);
    if (ib < m && jb < m) store(ib, jb, c11);
#endif
}

}  // namespace evc
