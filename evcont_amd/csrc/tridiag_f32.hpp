// Part of eigh_small.hpp, which includes this file behind the DPP helpers it uses (dpp_quad, kQuadXor1/2): the FP32
// start vectors of the refinement.
#pragma once
#include "common.hpp"

namespace evc {

// ------------------------------------------------------------------ FP32 tridiagonal eigensolver on ONE wave
// Start vectors for the refinement below, as LAPACK's xSYEVX would compute them, in single precision: Householder
// tridiagonalisation, eigenvalues by multisection on the Sturm count, eigenvectors of the tridiagonal matrix by
// twisted factorisation, back-transformation with the reflectors.  ~20 us for m = 30 where the Jacobi sweeps take
// 80.  Nothing here has to be accurate (the refinement squares the error and checks itself; vectors that come out
// parallel -- eigenvalues closer than single precision resolves -- make it give up, and the caller falls back to the
// Jacobi start), so there is no reorthogonalisation inside clusters and no safeguard beyond keeping pivots finite.
// Lane map: j = lane & 31 (row of the matrix, eigenvalue, eigenvector), h = lane >> 5 (column half / direction).
#ifndef EVC_STURM_ROUNDS
#define EVC_STURM_ROUNDS 6
#endif
constexpr int kSturmRounds = EVC_STURM_ROUNDS;   // multisection rounds of 17 sub-intervals each: 17^6 = 2.4e7 ~ 1 / FP32 epsilon
                                                 // (5 rounds: start error 1.5e-3 instead of 1.3e-4 at N = 30, a third refinement pass, +4 us)
constexpr int kTp = 36;    // floats per row of the matrix being reduced (16-byte aligned rows)
constexpr int kZfp = 33;   // floats per eigenvector row of the result (lane-private rows, conflict-free)

__device__ __forceinline__ float half32_sum(float v) {   // sum over the 32 lanes j (both halves hold the same values)
    v += dpp_quad<kQuadXor1>(v);
    v += dpp_quad<kQuadXor2>(v);
    v += dpp_quad<0x141>(v);
    v += dpp_quad<0x140>(v);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
}
__device__ __forceinline__ float readlane_f32(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// Af: m x m matrix (pitch kTp, rows/columns >= m zero), destroyed.  Zf[j*kZfp + i] = component i of eigenvector j
// (unnormalised), zn[j] = 1 / its norm.  scr: 32*32*5 + 5*32 floats; cntbuf: [2][8][32] ints (Sturm counts of a
// multisection round).  Called by the whole workgroup (it
// contains barriers): the reduction and the eigenvectors are chains on wave 0, the multisection runs one abscissa
// per lane on all four waves.
__device__ __forceinline__ void tridiag_eig_wg_f32(float *Af, int m, float *Zf, float *zn, float *scr, int *cntbuf) {
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5, wave = threadIdx.x >> 6;
    float *Vh = scr;                    // [k][r] reflector k
    float *fD = Vh + 32 * 32;           // [i][j][h] pivots of the forward / backward factorisation of lane pair j
    float *fF = fD + 2 * 32 * 32;       // [i][j][h] multipliers
    float *vv = fF + 2 * 32 * 32;       // v of the current step
    float *ww = vv + 32;                // w
    float *dd = ww + 32, *ee = dd + 32, *bb = ee + 32;   // diagonal, off-diagonal, 2 / v^T v
    const int c0 = h * 16;
    // ---- Householder reduction: A <- H_k A H_k, H_k = I - beta v v^T, v zero up to row k; the matrix stays in LDS, the
    //      two half-waves split the columns (a register-resident variant, few_roots.hpp, measured 0.97 us per step in
    //      single precision against 0.69 us for this loop: both are chains of reductions and LDS round trips, and this
    //      one has the shorter sums)
    for (int k = 0; wave == 0 && k + 2 < m; ++k) {
        const float x = (j > k && j < m) ? Af[j * kTp + k] : 0.0f;
        const float sig = half32_sum(x * x);
        const float xk1 = readlane_f32(x, k + 1);
        const float rest = sig - xk1 * xk1;            // what the reflector has to remove
        float alpha = xk1, beta = 0.0f, v = 0.0f;
        if (rest > 1.0e-30f) {
            alpha = -copysignf(__builtin_sqrtf(sig), xk1);
            beta = __builtin_amdgcn_rcpf(sig - xk1 * alpha);
            v = (j == k + 1) ? xk1 - alpha : x;
        }
        if (h == 0) {
            vv[j] = v;
            Vh[k * 32 + j] = v;
            if (j == 0) {
                dd[k] = Af[k * kTp + k];
                ee[k] = alpha;
                bb[k] = beta;
            }
        }
        float a[16], vc[16];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 t = *reinterpret_cast<const float4 *>(Af + j * kTp + c0 + 4 * u);
            const float4 q = *reinterpret_cast<const float4 *>(vv + c0 + 4 * u);
            a[4 * u] = t.x; a[4 * u + 1] = t.y; a[4 * u + 2] = t.z; a[4 * u + 3] = t.w;
            vc[4 * u] = q.x; vc[4 * u + 1] = q.y; vc[4 * u + 2] = q.z; vc[4 * u + 3] = q.w;
        }
        float part = 0.0f;
#pragma unroll
        for (int c = 0; c < 16; ++c) part = fmaf(a[c], vc[c], part);
        float pr = (part + __shfl_xor(part, 32)) * beta;          // p = beta A v
        const float K = 0.5f * beta * half32_sum(pr * v);
        const float w = pr - K * v;                               // (rows <= k: v = 0, and p is not used there)
        if (h == 0) ww[j] = (j > k) ? w : 0.0f;
        const float wr = (j > k) ? w : 0.0f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 q = *reinterpret_cast<const float4 *>(ww + c0 + 4 * u);
            float4 t;
            t.x = a[4 * u] - (v * q.x + wr * vc[4 * u]);
            t.y = a[4 * u + 1] - (v * q.y + wr * vc[4 * u + 1]);
            t.z = a[4 * u + 2] - (v * q.z + wr * vc[4 * u + 2]);
            t.w = a[4 * u + 3] - (v * q.w + wr * vc[4 * u + 3]);
            *reinterpret_cast<float4 *>(Af + j * kTp + c0 + 4 * u) = t;
        }
    }
    EVC_STAMP(11);
    if (threadIdx.x == 0) {
        dd[m - 2] = Af[(m - 2) * kTp + m - 2];
        dd[m - 1] = Af[(m - 1) * kTp + m - 1];
        ee[m - 2] = Af[(m - 1) * kTp + m - 2];
        ee[m - 1] = 0.0f;
    }
    __syncthreads();
    // ---- eigenvalue j by multisection: one abscissa per lane, 8 per eigenvalue (4 waves x 2 halves) -> 9 sub-intervals
    //      per round; the Sturm counts of a round are exchanged through LDS (double-buffered: one barrier per round)
    float dr[32], e2[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        dr[i] = i < m ? dd[i] : 0.0f;
        const float e = (i + 1 < m) ? ee[i] : 0.0f;
        e2[i] = e * e;
    }
    float glo, ghi, emx = 0.0f;
    {
        const float ea = (j > 0 && j < m) ? fabsf(ee[j - 1]) : 0.0f, eb = (j + 1 < m) ? fabsf(ee[j]) : 0.0f;
        const float dj = j < m ? dd[j] : 0.0f;
        float lo = j < m ? dj - ea - eb : 3.0e38f, hi = j < m ? dj + ea + eb : -3.0e38f, em = fmaxf(ea, eb);
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) {
            lo = fminf(lo, __shfl_xor(lo, off));
            hi = fmaxf(hi, __shfl_xor(hi, off));
            em = fmaxf(em, __shfl_xor(em, off));
        }
        const float pad = 1.0e-6f * fmaxf(fabsf(lo), fabsf(hi)) + 1.0e-30f;
        glo = lo - pad;
        ghi = hi + pad;
        emx = em;
    }
    const float pivmin = 1.0e-30f + 1.0e-14f * emx * emx;
    // (the Sturm recurrence runs unguarded: a zero pivot gives q = -inf, which counts as negative and is followed by
    //  q = d - x, as IEEE arithmetic has it; e^2 is kept away from zero so that 0 * inf cannot occur)
#pragma unroll
    for (int i = 0; i < 32; ++i) e2[i] = fmaxf(e2[i], 1.0e-36f);
    float lo = glo, hi = ghi;
    const int slot = 2 * wave + h;   // 0..7; this lane evaluates abscissae 2 slot + 1, 2 slot + 2 of 16
    for (int it = 0; it < kSturmRounds; ++it) {
        const float wd = (hi - lo) * (1.0f / 17.0f);
        const float xa = lo + wd * (float)(2 * slot + 1), xb = lo + wd * (float)(2 * slot + 2);
        float qa = dr[0] - xa, qb = dr[0] - xb;
        int ca = qa < 0.0f ? 1 : 0, cb2 = qb < 0.0f ? 1 : 0;
#pragma unroll
        for (int i = 1; i < 32; ++i) {
            if (i >= m) break;   // uniform: one test per step that is taken, none behind the end
            qa = (dr[i] - xa) - e2[i - 1] * __builtin_amdgcn_rcpf(qa);
            qb = (dr[i] - xb) - e2[i - 1] * __builtin_amdgcn_rcpf(qb);
            ca += qa < 0.0f ? 1 : 0;
            cb2 += qb < 0.0f ? 1 : 0;
        }
        int *cb = cntbuf + (it & 1) * 256;
        // eigenvalue j (ascending, 0-based) is >= x  <=>  count(x) <= j
        cb[slot * 32 + j] = (ca <= j ? 1 : 0) + (cb2 <= j ? 1 : 0);
        __syncthreads();
        int below = 0;
#pragma unroll
        for (int p = 0; p < 8; ++p) below += cb[p * 32 + j];
        lo = lo + wd * (float)below;
        hi = lo + wd;
    }
    if (wave != 0) return;
    const float lam = 0.5f * (lo + hi);
    EVC_STAMP(12);
    // ---- eigenvector of the tridiagonal matrix: twisted factorisation (h = 0: from the top, h = 1: from the bottom)
    {
        auto at = [&](int ii) { return h ? m - 1 - ii : ii; };
        float D = dd[at(0)] - lam;
        for (int ii = 0; ii + 1 < m; ++ii) {
            const int pos = at(ii), nxt = at(ii + 1), ei = pos < nxt ? pos : nxt;
            if (fabsf(D) < pivmin) D = -pivmin;
            const float e = ee[ei], F = e * __builtin_amdgcn_rcpf(D);
            fD[(pos * 32 + j) * 2 + h] = D;
            fF[(ei * 32 + j) * 2 + h] = F;
            D = (dd[nxt] - lam) - F * e;
        }
        fD[(at(m - 1) * 32 + j) * 2 + h] = D;
    }
    int kt = 0;
    {
        float best = 3.0e38f;
        for (int i = 0; i < m; ++i) {
            const float g = fabsf(fD[(i * 32 + j) * 2] + fD[(i * 32 + j) * 2 + 1] - (dd[i] - lam));
            if (g < best) {
                best = g;
                kt = i;
            }
        }
    }
    float nrm = h ? 0.0f : 1.0f;
    {
        // h = 0: z_i = -L_i z_{i+1} downwards from the twist; h = 1: z_{i+1} = -U_i z_i upwards
        float z = 1.0f;
        if (j < m) {
            if (h == 0) {
                Zf[j * kZfp + kt] = 1.0f;
                for (int i = kt - 1; i >= 0; --i) {
                    z = -fF[(i * 32 + j) * 2] * z;
                    Zf[j * kZfp + i] = z;
                    nrm = fmaf(z, z, nrm);
                }
            } else {
                for (int i = kt; i + 1 < m; ++i) {
                    z = -fF[(i * 32 + j) * 2 + 1] * z;
                    Zf[j * kZfp + i + 1] = z;
                    nrm = fmaf(z, z, nrm);
                }
            }
        }
    }
    nrm += __shfl_xor(nrm, 32);
    EVC_STAMP(13);
    if (h == 0 && j < m) zn[j] = __builtin_amdgcn_rsqf(nrm);
    // ---- back-transformation z <- H_0 H_1 ... H_{m-3} z: rows c0 .. c0+15 of eigenvector j in registers
    float z[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) z[c] = (j < m && c0 + c < m) ? Zf[j * kZfp + c0 + c] : 0.0f;
    for (int k = m - 3; k >= 0; --k) {
        float vk[16];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 t = *reinterpret_cast<const float4 *>(Vh + k * 32 + c0 + 4 * u);
            vk[4 * u] = t.x; vk[4 * u + 1] = t.y; vk[4 * u + 2] = t.z; vk[4 * u + 3] = t.w;
        }
        float dot = 0.0f;
#pragma unroll
        for (int c = 0; c < 16; ++c) dot = fmaf(vk[c], z[c], dot);
        dot = (dot + __shfl_xor(dot, 32)) * bb[k];
#pragma unroll
        for (int c = 0; c < 16; ++c) z[c] = fmaf(-dot, vk[c], z[c]);
    }
    if (j < m)
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (c0 + c < m) Zf[j * kZfp + c0 + c] = z[c];
}

}  // namespace evc
