// The gradient's single-workgroup pieces: the row weights of given coefficient vectors (pair_weights_kernel) and
//   K12/K16 one-body gradient intermediates and the adjoint Loewdin response that folds
//          K10/K11 (gradients_loewdin.py:41-134,155-187,300-303) into four N^3 products
// (grad_prep_kernel, unpack8_prep_kernel, grad_final_kernel).
#include <stdlib.h>
#include <string.h>

#include "common.hpp"
#include "kernels.hpp"
#include "small_mm.hpp"
#include "unpack_tiles.hpp"

namespace evc {

// Row weights from coefficient vectors the caller supplies (the non-Hermitian branch: the T x T pencil is solved
// with scipy.linalg.eig on the host, as the reference does, and its eigenvector comes back here), or of the symmetric
// weighting W = (c_k c_l^T + c_l c_k^T) / 2 of a pair of roots (evc_phase_gradient_roots), one slot per blockIdx.y.
// k == l evaluates exactly the single-vector expressions c_a c_b.
__global__ __launch_bounds__(256) void pair_weights_kernel(PairWeightsArgs a) {
    const int slot = (int)blockIdx.y, g = a.slot0 + slot;
    const int T = a.T;
    const double *c = a.c + geo_of(g, a.geo_period) * a.sc;   // (geo_period = 0: one coefficient block)
    const double *ck = c + (int64_t)a.k[slot] * T, *cl = c + (int64_t)a.l[slot] * T;
    const bool diag = a.k[slot] == a.l[slot];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    // transposed copies: [row][slot] in the workspace of the first slot of the group of kMaxBatchG (csrc/kernels.hpp)
    const int64_t gt = (int64_t)(g - g % kMaxBatchG) * a.sw;
    const int col = g % kMaxBatchG;
    if (a.w1 && i < (int64_t)T * T) {
        const int ia = (int)(i / T), ib = (int)(i - (int64_t)ia * T);
        const double w = diag ? ck[ia] * ck[ib] : 0.5 * (ck[ia] * cl[ib] + cl[ia] * ck[ib]);
        a.w1[(int64_t)g * a.sw + i] = w;
        if (a.w1t) a.w1t[gt + i * kMaxBatchG + col] = w;
    }
    if (a.w2 && i < a.w2_count) {
        const int64_t r = i + a.w2_offset;
        double w;
        if (a.pairs) {
            const int ia = (int)tri_row(r), ib = (int)(r - (int64_t)ia * (ia + 1) / 2);
            if (diag) w = (ia == ib) ? ck[ia] * ck[ia] : 2.0 * ck[ia] * ck[ib];
            else w = (ia == ib) ? ck[ia] * cl[ia] : ck[ia] * cl[ib] + cl[ia] * ck[ib];
        } else {
            const int ia = (int)(r / T), ib = (int)(r - (int64_t)ia * T);
            w = diag ? ck[ia] * ck[ib] : 0.5 * (ck[ia] * cl[ib] + cl[ia] * ck[ib]);
        }
        a.w2[(int64_t)g * a.sw + i] = w;
        if (a.w2t) a.w2t[gt + i * kMaxBatchG + col] = w;
    }
}

static int pair_weights_launch(PairWeightsArgs &a, int nslots, hipStream_t st) {
    const int64_t nmax = (int64_t)a.T * a.T > a.w2_count ? (int64_t)a.T * a.T : a.w2_count;
    hipLaunchKernelGGL(pair_weights_kernel, dim3((unsigned)ceil_div(nmax, 256), (unsigned)nslots), dim3(256), 0, st, a);
    EVC_LAUNCH_CHECK("pair_weights");
    return 0;
}

int launch_pair_weights(const double *c, int T, int layout, double *w1, double *w2, int64_t w2_offset,
                        int64_t w2_count, hipStream_t st) {
    PairWeightsArgs a;
    memset(&a, 0, sizeof(a));
    a.c = c;
    a.T = T;
    a.pairs = layout_pairs(layout);
    a.w1 = w1;
    a.w2 = w2;
    a.w2_offset = w2_offset;
    a.w2_count = w2_count;
    return pair_weights_launch(a, 1, st);
}

// Slots s = p * geo_period + g (geo_period > 0; npairs counts the root pairs, the launch covers npairs * geo_period
// slots): pair p of coefficient block g.  geo_period = 0: slot p = pair p of the one block c.
int launch_pair_weights_geo(const double *c, int64_t sc, int geo_period, int T, int layout, const int32_t *pairs,
                            int npairs, double *w1, double *w2, double *w1t, double *w2t, int64_t sw, int64_t w2_offset,
                            int64_t w2_count, hipStream_t st) {
    PairWeightsArgs a;
    memset(&a, 0, sizeof(a));
    a.c = c;
    a.sc = sc;
    a.geo_period = geo_period;
    a.T = T;
    a.pairs = layout_pairs(layout);
    a.w1 = w1;
    a.w2 = w2;
    a.w1t = w1t;
    a.w2t = w2t;
    a.sw = sw;
    a.w2_offset = w2_offset;
    a.w2_count = w2_count;
    const int per = geo_period > 0 ? geo_period : 1, nslots = npairs * per;
    for (int s0 = 0; s0 < nslots; s0 += kPairWeightsSlots) {
        const int ns = nslots - s0 < kPairWeightsSlots ? nslots - s0 : kPairWeightsSlots;
        a.slot0 = s0;
        for (int s = 0; s < ns; ++s) {
            a.k[s] = (int16_t)pairs[2 * ((s0 + s) / per)];
            a.l[s] = (int16_t)pairs[2 * ((s0 + s) / per) + 1];
        }
        if (int rc = pair_weights_launch(a, ns, st)) return rc;
    }
    return 0;
}

// ------------------------------------------------------------------ gradient prep
// Pao = X D X^T ; Y1 = scale1 * hcore X (D + D^T)
__device__ __forceinline__ void grad_prep_body(GradPrepArgs a, int64_t g) {
    extern __shared__ __align__(16) double sm[];
    const int n = a.n;
    {
        a.X += g * a.sws;
        a.hcore += geo_of(g, a.geo_period) * a.sh;
        a.D += g * a.sD;
        a.Pao += g * a.sws;
        a.Y1 += g * a.sws;
    }
    if (n <= 32) {
        // row.row products at pitch kRp (16-byte LDS loads, no bank conflicts): X symmetric, so
        //   T1t[j][i] = (X D)[i][j] = sum_k Dt[j][k] X[i][k],  Pao[i][j] = sum_k T1[i][k] X[j][k]   (T1 = T1t^T stored both ways)
        //   T2t[j][i] = (X (D + D^T))[i][j] = sum_k Dsym[j][k] X[i][k],  Y1[i][j] = scale1 sum_k h[i][k] T2t[j][k]
        double *Xp = sm, *Dt = Xp + kRsz, *Ds2 = Dt + kRsz, *Hp = Ds2 + kRsz, *T1 = Hp + kRsz, *T2t = T1 + kRsz;
        const int m = (n + 1) & ~1;
        for (int idx = threadIdx.x; idx < kRsz; idx += kThreads) {
            const int i = idx / kRp, j = idx - i * kRp;
            const bool in = i < n && j < n;
            const double dij = in ? a.D[i * n + j] : 0.0, dji = in ? a.D[j * n + i] : 0.0;
            Xp[idx] = in ? a.X[i * n + j] : 0.0;
            Dt[idx] = dji;
            Ds2[idx] = dij + dji;
            Hp[idx] = in ? a.hcore[i * n + j] : 0.0;
            T1[idx] = 0.0;
            T2t[idx] = 0.0;
        }
        __syncthreads();
        // T1[i][j] = (X D)[i][j] = sum_k X[i][k] Dt[j][k];  T2t[j][i] = sum_k Dsym[j][k] X[i][k]
        mm_rowrow(m, Xp, Dt, [&](int i, int j, double v) { T1[i * kRp + j] = v; });
        mm_rowrow(m, Ds2, Xp, [&](int j, int i, double v) { T2t[j * kRp + i] = v; });
        __syncthreads();
        mm_rowrow(m, T1, Xp, [&](int i, int j, double v) {
            if (i < n && j < n) a.Pao[i * n + j] = v;
        });
        mm_rowrow(m, Hp, T2t, [&](int i, int j, double v) {
            if (i < n && j < n) a.Y1[i * n + j] = a.scale1 * v;
        });
        return;
    }
    if (n > 64) {
        // four n x n matrices no longer fit LDS: one product buffer, the operands through the caches
        double *Ts = sm;   // n*n
        mm16(n, [&](int i, int k) { return a.X[i * n + k]; }, [&](int k, int j) { return a.D[k * n + j]; },
             [&](int i, int j, double v) { Ts[i * n + j] = v; });
        __syncthreads();
        mm16(n, [&](int i, int k) { return Ts[i * n + k]; }, [&](int k, int j) { return a.X[j * n + k]; },
             [&](int i, int j, double v) { a.Pao[i * n + j] = v; });
        __syncthreads();
        mm16(n, [&](int i, int k) { return a.X[i * n + k]; },
             [&](int k, int j) { return a.D[k * n + j] + a.D[j * n + k]; },
             [&](int i, int j, double v) { Ts[i * n + j] = v; });
        __syncthreads();
        mm16(n, [&](int i, int k) { return a.hcore[i * n + k]; }, [&](int k, int j) { return Ts[k * n + j]; },
             [&](int i, int j, double v) { a.Y1[i * n + j] = a.scale1 * v; });
        return;
    }
    double *Xs = sm;            // n*n
    double *Ds = Xs + n * n;    // n*n
    double *Hs = Ds + n * n;    // n*n
    double *Ts = Hs + n * n;    // n*n
    copy_to_lds(Xs, a.X, n * n);
    copy_to_lds(Ds, a.D, n * n);
    copy_to_lds(Hs, a.hcore, n * n);
    __syncthreads();
    mm16(n, [&](int i, int k) { return Xs[i * n + k]; }, [&](int k, int j) { return Ds[k * n + j]; },
         [&](int i, int j, double v) { Ts[i * n + j] = v; });
    __syncthreads();
    mm16(n, [&](int i, int k) { return Ts[i * n + k]; }, [&](int k, int j) { return Xs[j * n + k]; },
         [&](int i, int j, double v) { a.Pao[i * n + j] = v; });
    __syncthreads();
    mm16(n, [&](int i, int k) { return Xs[i * n + k]; },
         [&](int k, int j) { return Ds[k * n + j] + Ds[j * n + k]; },
         [&](int i, int j, double v) { Ts[i * n + j] = v; });
    __syncthreads();
    mm16(n, [&](int i, int k) { return Hs[i * n + k]; }, [&](int k, int j) { return Ts[k * n + j]; },
         [&](int i, int j, double v) { a.Y1[i * n + j] = a.scale1 * v; });
}

__global__ __launch_bounds__(kThreads) void grad_prep_kernel(GradPrepArgs a) { grad_prep_body(a, blockIdx.x); }

// The same launch ALSO unpacks the packed predicted 2-RDM of the compressed layout into the dense symmetric (pair, pair)
// matrix SB (SB[u][v] = 4 p[tri(max, min)], the mirrored-tile copy of unpack_tiles.hpp, as pack.hip unpack8_pairs_kernel):
// both only need what K8 has just written, so the `count` workgroups of the one and the count * unpack_tile_count(npairs)
// workgroups of the other share a launch instead of following each other (one kernel boundary and the shorter of the
// two durations less on the critical path of a step).  Blocks [0, count): grad_prep; the rest: unpack, one tile each, its
// LDS tile inside the LDS that every block of the launch reserves for grad_prep.
__global__ __launch_bounds__(kThreads) void unpack8_prep_kernel(GradPrepArgs a, const double *__restrict__ p, int64_t sp,
                                                                double *__restrict__ SB, int64_t sws, int count, int ld) {
    if ((int)blockIdx.x < count) {
        grad_prep_body(a, blockIdx.x);
        return;
    }
    extern __shared__ __align__(16) double sm[];
    const int n = a.n, npairs = n * (n + 1) / 2;
    int geom, blk;
    unpack_tile_geom((int64_t)blockIdx.x - count, count, unpack_tile_count(npairs), geom, blk);
    unpack8_tile(p + (int64_t)geom * sp, SB + (int64_t)geom * sws, npairs, ld, blk, sm);
}

static size_t grad_prep_lds(int n) {
    return n <= 32 ? sizeof(double) * (size_t)6 * kRsz : sizeof(double) * (size_t)(n > 64 ? 1 : 4) * n * n;
}

int launch_unpack8_prep(const GradPrepArgs &a, const double *packed, int64_t sp, double *SB, int64_t sws, int count,
                        hipStream_t st) {
    const int npairs = a.n * (a.n + 1) / 2, bpg = unpack_tile_count(npairs);
    const size_t lds = grad_prep_lds(a.n) > kUtLds ? grad_prep_lds(a.n) : kUtLds;   // (grad_prep's, at every n)
    static LdsAttr attr;
    if (int rc = allow_dynamic_lds(unpack8_prep_kernel, attr, 160 * 1024, "unpack8_prep")) return rc;
    hipLaunchKernelGGL(unpack8_prep_kernel, dim3((unsigned)(count + bpg * count)), dim3(kThreads), lds, st, a,
                       packed, sp, SB, sws, count, pair_ld(a.n));
    EVC_LAUNCH_CHECK("unpack8_prep");
    note_kernel(EVC_PROF_UNPACK, "unpack8_prep_kernel");
    return 0;
}

int launch_grad_prep(const GradPrepArgs &a, int count, hipStream_t st) {
    const size_t lds = grad_prep_lds(a.n);
    static LdsAttr attr;
    if (int rc = allow_dynamic_lds(grad_prep_kernel, attr, 160 * 1024, "grad_prep")) return rc;
    hipLaunchKernelGGL(grad_prep_kernel, dim3(count), dim3(kThreads), lds, st, a);
    EVC_LAUNCH_CHECK("grad_prep");
    return 0;
}

// ------------------------------------------------------------------ gradient finalisation
// dE = <dX, Y> + explicit terms, with dX[A,x] = U [ (U^T dS[A,x] U) o F ] U^T (Daleckii-Krein form
// of gradients_loewdin.py:41-134).  Taking the adjoint once,  <dX,Y> = <dS, W>,
// W = U [ F o (U^T Y U) ] U^T, removes the (N,N,A,3) tensor altogether.
template <int NMAX>   // 32: n <= 32 (and n > 64, where nothing is staged); 64: 32 < n <= 64
__global__ __launch_bounds__(kThreads) void grad_final_kernel(GradFinalArgs a) {
    extern __shared__ __align__(16) double sm[];
    const int n = a.n;
    {
        const int64_t g = blockIdx.x;
        a.U += g * a.sws;
        a.s += g * a.sws;
        a.Y1 += g * a.sws;
        a.y2 += g * a.sws;
        a.t2part += g * a.sws;
        a.term3 += g * a.sws;
        a.ipovlp += geo_of(g, a.geo_period) * a.sip;
        if (a.gnuc) a.gnuc += g * a.sgn;
        a.grad += g * a.sgrad;
    }
    // n > 64: four n x n matrices do not fit LDS -- Y and U are then read through the caches (`wide`), Q and W stay
    const bool wide = n > 64;
    double *Y = sm;                          // n*n   (wide: unused, zero-sized)
    double *Q = wide ? sm : Y + n * n;       // n*n
    double *W = Q + n * n;                   // n*n
    double *Us = wide ? W : W + n * n;       // n*n   (wide: unused, zero-sized)
    double *rs = (wide ? W : Us) + n * n;    // n   sqrt(s) (0 where guarded)
    double *fs = rs + n;       // n   f(s)
    double *ss = fs + n;       // n   s
    double *t2 = ss + n;       // 3*n
    double *add = t2 + 3 * n;  // 3*natm: scale1 * (term3 + gnuc)
    int *sl = reinterpret_cast<int *>(add + 3 * a.natm);   // 2*natm: AO slices
    const int tid = threadIdx.x;
    // n <= 64: the 3 n^2 overlap derivatives are fetched into registers now and parked in the three product
    // buffers once those are free, so that the per-atom loop at the end runs out of LDS (it is a chain of
    // dependent global loads otherwise: ~2 us per (atom, x) and wave)
    const bool stage_ip = !wide;          // (n <= 64: the three product buffers exist)
    constexpr int kIpf = (3 * NMAX * NMAX + kThreads - 1) / kThreads;   // 12 values per thread at n = 32, 48 at n = 64
    double ipf[kIpf];
    if (stage_ip) {
#pragma unroll
        for (int u = 0; u < kIpf; ++u)
            if (kThreads * u < 3 * n * n) {   // uniform
                const int idx = tid + kThreads * u;
                ipf[u] = idx < 3 * n * n ? a.ipovlp[idx] : 0.0;
            }
    }
    for (int idx = tid; idx < 2 * a.natm; idx += kThreads) sl[idx] = (int)a.aoslices[idx];
    for (int idx = tid; idx < 3 * a.natm; idx += kThreads) {
        double g = 0.0;
        if (a.scale1 != 0.0) {
            g = a.scale1 * a.term3[idx];
            if (a.gnuc) g += a.scale1 * a.gnuc[idx];
        }
        add[idx] = g;
    }
    if (!wide) {
        copy_to_lds(Us, a.U, n * n);
        for (int idx = tid; idx < n * n; idx += kThreads) {
            const int ai = idx / n, i = idx - ai * n;  // Y[a][i]; y2 is stored [i][a]
            Y[idx] = a.Y1[idx] + 0.5 * a.y2[i * n + ai];
        }
    }
    auto Uv = [&](int i, int j) { return wide ? a.U[i * n + j] : Us[i * n + j]; };
    auto Yv = [&](int k, int j) { return wide ? a.Y1[k * n + j] + 0.5 * a.y2[j * n + k] : Y[k * n + j]; };
    if (tid < n) {
        const double s = a.s[tid];
        const bool ok = s > 1.0e-15;
        ss[tid] = s;
        rs[tid] = ok ? sqrt(s) : 0.0;
        fs[tid] = ok ? 1.0 / sqrt(s) : 0.0;
    }
    for (int idx = tid; idx < 3 * n; idx += kThreads) {
        const int m_ = idx / 3, x = idx - 3 * m_;
        // (eight loads in flight: the partials of one (m, x) are a chain of nchunk >= n dependent round trips otherwise)
        const double *p = a.t2part + ((int64_t)m_ * 3 + x) * a.nchunk;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
        int ch = 0;
        for (; ch + 8 <= a.nchunk; ch += 8) {
            s0 += p[ch];
            s1 += p[ch + 1];
            s2 += p[ch + 2];
            s3 += p[ch + 3];
            s4 += p[ch + 4];
            s5 += p[ch + 5];
            s6 += p[ch + 6];
            s7 += p[ch + 7];
        }
        for (; ch < a.nchunk; ++ch) s0 += p[ch];
        t2[x * n + m_] = ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7));
    }
    __syncthreads();
    // Q = U^T Y
    mm16(n, [&](int i, int k) { return Uv(k, i); }, [&](int k, int j) { return Yv(k, j); },
         [&](int i, int j, double v) { Q[i * n + j] = v; });
    __syncthreads();
    // W = (Q U) o F
    mm16(n, [&](int i, int k) { return Q[i * n + k]; }, [&](int k, int j) { return Uv(k, j); },
         [&](int i, int j, double v) {
             double F;
             if (rs[i] > 0.0 && rs[j] > 0.0) F = -1.0 / (rs[i] * rs[j] * (rs[i] + rs[j]));
             else if (ss[i] != ss[j]) F = (fs[i] - fs[j]) / (ss[i] - ss[j]);
             else F = 0.0;
             W[i * n + j] = v * F;
         });
    __syncthreads();
    // Q = U W
    mm16(n, [&](int i, int k) { return Uv(i, k); }, [&](int k, int j) { return W[k * n + j]; },
         [&](int i, int j, double v) { Q[i * n + j] = v; });
    __syncthreads();
    // W = Q U^T
    mm16(n, [&](int i, int k) { return Q[i * n + k]; }, [&](int k, int j) { return Uv(j, k); },
         [&](int i, int j, double v) { W[i * n + j] = v; });
    __syncthreads();
    // grad[A,x] = - sum_{mu in A} sum_nu ip[x,mu,nu] (W[mu,nu] + W[nu,mu])
    //             - 1/2 sum_{m in A} t2[x][m] + scale1 * (term3 + gnuc)
    if (stage_ip) {  // Y, Q, Us are free now: ip[x] -> {Y, Q, Us}[x]
#pragma unroll
        for (int u = 0; u < kIpf; ++u) {
            const int idx = tid + kThreads * u;
            if (kThreads * u < 3 * n * n && idx < 3 * n * n) {
                const int x = idx / (n * n);
                (x == 0 ? Y : x == 1 ? Q : Us)[idx - x * n * n] = ipf[u];
            }
        }
        __syncthreads();
    }
    // two short steps instead of one wave-wide reduction per (atom, x): q[x][mu] = sum_nu ip[x,mu,nu] (W + W^T)[mu,nu]
    // + t2[x][mu] / 2 by one thread per (x, mu) (sum_A (p1 - p0) = n: 3 n dots of length n in all), then one thread
    // per (atom, x) adds up its AOs
    for (int idx = tid; idx < 3 * n; idx += kThreads) {
        const int x = idx / n, mu = idx - x * n;
        const double *ipx = x == 0 ? Y : x == 1 ? Q : Us;
        double s0 = 0.0, s1 = 0.0;
        int nu = 0;
        for (; nu + 2 <= n; nu += 2) {
            const double i0 = stage_ip ? ipx[mu * n + nu] : a.ipovlp[(x * n + mu) * n + nu];
            const double i1 = stage_ip ? ipx[mu * n + nu + 1] : a.ipovlp[(x * n + mu) * n + nu + 1];
            s0 = fma(i0, W[mu * n + nu] + W[nu * n + mu], s0);
            s1 = fma(i1, W[mu * n + nu + 1] + W[(nu + 1) * n + mu], s1);
        }
        if (nu < n) {
            const double i0 = stage_ip ? ipx[mu * n + nu] : a.ipovlp[(x * n + mu) * n + nu];
            s0 = fma(i0, W[mu * n + nu] + W[nu * n + mu], s0);
        }
        t2[idx] = (s0 + s1) + 0.5 * t2[idx];
    }
    __syncthreads();
    for (int ax = tid; ax < a.natm * 3; ax += kThreads) {
        const int A = ax / 3, x = ax - 3 * A;
        double s = 0.0;
        for (int mu = sl[2 * A]; mu < sl[2 * A + 1]; ++mu) s += t2[x * n + mu];
        a.grad[ax] = add[ax] - s;
    }
}

int launch_grad_final(const GradFinalArgs &a, int count, hipStream_t st) {
    const size_t lds = sizeof(double) * ((size_t)(a.n > 64 ? 2 : 4) * a.n * a.n + 6 * a.n + 3 * (size_t)a.natm) +
                       sizeof(int) * 2 * (size_t)a.natm + 16;
    if (a.n > 32 && a.n <= 64) {
        static LdsAttr attr;
        if (int rc = allow_dynamic_lds(grad_final_kernel<64>, attr, 160 * 1024, "grad_final")) return rc;
        hipLaunchKernelGGL(grad_final_kernel<64>, dim3(count), dim3(kThreads), lds, st, a);
    } else {
        static LdsAttr attr;
        if (int rc = allow_dynamic_lds(grad_final_kernel<32>, attr, 160 * 1024, "grad_final")) return rc;
        hipLaunchKernelGGL(grad_final_kernel<32>, dim3(count), dim3(kThreads), lds, st, a);
    }
    EVC_LAUNCH_CHECK("grad_final");
    return 0;
}

}  // namespace evc
