// Streaming t-RDM contractions (HBM-bandwidth bound):
//   K5/K4  rows GEMV   y[g][r]   = sum_c A[r,c] v[g][c]     (H_ab build,      evcont.py:38-68)
//   K8/K7  cols GEMV   out[g][c] = sum_r w[g][r] A[r,c]     (predicted RDMs,  gradients_loewdin.py:343-356)
// A (the t-RDM) is shared by a batch of geometries, so one pass over the 0.68-2.6 GB matrix serves
// G evaluations: G <= 8 per pass with the VALU kernels of this file, 12..64 with the matrix-core
// variants of gemv_mfma.hip, gemv_lds.hip and gemv_cols_lds.hip (gemv_dispatch.hip plans the passes of a call).
// Each launch carries TWO problems (the two-body and the one-body t-RDM) so the small one rides
// along with the big one instead of costing a kernel boundary.
#include <stdlib.h>

#include "common.hpp"
#include "kernels.hpp"

namespace evc {

constexpr int kChunk = 512;  // columns per workgroup step (256 lanes x 16 B)

__device__ __forceinline__ double2 ld_stream(const double *p) {
    return *reinterpret_cast<const double2 *>(p);
}

// Wave reduction of N (power of two <= 64) per-lane values with N-1 shuffles instead of 6N: at each
// butterfly step a lane sends the half of its values it does not keep.  On return every lane holds
// the wave-wide sum of value index lane >> (6 - log2 N).
template <int N, int M, int OFF>
__device__ __forceinline__ void multi_reduce_step(double (&v)[N], int lane) {
    if constexpr (M > 1) {
        const bool up = (lane & OFF) != 0;
#pragma unroll
        for (int i = 0; i < M / 2; ++i) {
            const double send = up ? v[i] : v[i + M / 2];
            const double keep = up ? v[i + M / 2] : v[i];
            v[i] = keep + __shfl_xor(send, OFF, kWave);
        }
        multi_reduce_step<N, M / 2, OFF / 2>(v, lane);
    } else if constexpr (OFF >= 1) {
        v[0] += __shfl_xor(v[0], OFF, kWave);
        multi_reduce_step<N, 1, OFF / 2>(v, lane);
    }
}

template <int N>
__device__ __forceinline__ double multi_reduce(double (&v)[N], int lane) {
    multi_reduce_step<N, N, 32>(v, lane);
    return v[0];
}

// ------------------------------------------------------------------ rows GEMV
// Workgroup = 256 lanes x 16 B = one 512-column chunk of RB rows per step; a block owns a span of
// `span_cols` columns, keeps v[g] for the chunk in registers and RB*G accumulators per lane.
// Partials go to ws[g][span][row]; the consumer sums the spans in fixed order (deterministic).
template <int RB, int G>
__global__ __launch_bounds__(256) void gemv_rows_kernel(GemvRowsLaunch L, int g0) {
    constexpr int NV = RB * G;
    __shared__ double red[NV][4];
    int bid = blockIdx.x;
    const int which = bid >= L.nblk0 ? 1 : 0;
    if (which) bid -= L.nblk0;
    const RowProblem &P = L.p[which];
    const int span = bid % P.nspans;
    const int rb = bid / P.nspans;
    const int64_t row0 = (int64_t)rb * RB;
    const int nrows = (int)min((int64_t)RB, P.rows - row0);
    const int tid = threadIdx.x;

    int64_t c = (int64_t)span * P.span_cols + tid * 2;
    const int64_t cend = min(P.cols, (int64_t)(span + 1) * P.span_cols);
    const int64_t ld = P.ld;
    const double *__restrict__ v = P.v + (int64_t)g0 * P.vstride;
    const int64_t vs = P.vstride;
    // rows past the end of a ragged last block re-read the last valid row (results discarded)
    const double *__restrict__ Ar[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) Ar[r] = P.A + (row0 + (r < nrows ? r : nrows - 1)) * ld;

    double acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.0;

    for (; c + 1 < cend; c += kChunk) {
        double2 a[RB], vv[G];
#pragma unroll
        for (int r = 0; r < RB; ++r) a[r] = ld_stream(Ar[r] + c);
#pragma unroll
        for (int g = 0; g < G; ++g) vv[g] = ld_stream(v + g * vs + c);
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int g = 0; g < G; ++g) acc[r * G + g] = fma(a[r].y, vv[g].y, fma(a[r].x, vv[g].x, acc[r * G + g]));
    }
    if (c < cend) {  // odd `cols`: last single column
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const double ax = Ar[r][c];
#pragma unroll
            for (int g = 0; g < G; ++g) acc[r * G + g] = fma(ax, v[g * vs + c], acc[r * G + g]);
        }
    }

    const int lane = tid & 63, wave = tid >> 6;
    const double s = multi_reduce<NV>(acc, lane);
    constexpr int kShift = (NV >= 64) ? 0 : (NV == 32 ? 1 : NV == 16 ? 2 : NV == 8 ? 3 : NV == 4 ? 4 : NV == 2 ? 5 : 6);
    if ((lane & ((1 << kShift) - 1)) == 0) red[lane >> kShift][wave] = s;
    __syncthreads();
    if (tid < NV) {
        const int r = tid / G, g = tid - r * G;
        if (r < nrows) {
            const double t = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
            P.partial[(int64_t)(g0 + g) * P.pstride + (int64_t)span * P.rows + row0 + r] = t;
        }
    }
}

// Batched variant for G >= 4.  With G vectors the lane-private form above re-reads the v tile once per
// row block (G/RB times the bytes of A through L2 and the texture path) and its RB*G accumulators cut
// the occupancy, i.e. the bytes in flight.  Here the roles are turned: the four waves of a workgroup
// take DIFFERENT rows (RBW each) of the SAME column tile (SUB sub-steps of 128 columns), the v tile
// (G x SUB*128 doubles) is staged once per workgroup in LDS, and every lane issues all RBW*SUB = 16
// independent 16-byte loads of A for the tile before the staging barrier, so a wave keeps 16 KB of the
// stream in flight with only RBW*G accumulators.  Each wave reduces its own rows (no cross-wave sum).
constexpr int kStep = 128;  // columns per sub-step (64 lanes x 16 B)

template <int RBW, int G, int SUB>
__global__ __launch_bounds__(256, 3) void gemv_rows_wr_kernel(GemvRowsLaunch L, int g0) {
    constexpr int NV = RBW * G;
    constexpr int TILE = SUB * kStep;        // columns per iteration
    constexpr int VPT = G * TILE / 256;      // doubles of the v tile each thread stages
    static_assert(VPT % 2 == 0 && (TILE % VPT) == 0, "tile shape");
    __shared__ __align__(16) double vt[G][TILE];
    int bid = blockIdx.x;
    const int which = bid >= L.nblk0 ? 1 : 0;
    if (which) bid -= L.nblk0;
    const RowProblem &P = L.p[which];
    const int span = bid % P.nspans;
    const int rg = bid / P.nspans;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t rows = P.rows, cols = P.cols, ld = P.ld;
    const int64_t row0 = (int64_t)rg * (4 * RBW) + wave * RBW;
    const int64_t cbeg = (int64_t)span * P.span_cols;
    const int64_t cend = min(cols, (int64_t)(span + 1) * P.span_cols);
    const double *__restrict__ v = P.v + (int64_t)g0 * P.vstride;
    const double *__restrict__ Ar[RBW];
#pragma unroll
    for (int r = 0; r < RBW; ++r) {
        int64_t rr = row0 + r;
        if (rr >= rows) rr = rows - 1;  // re-read a valid row, result discarded
        Ar[r] = P.A + rr * ld;
    }
    // staging role of this thread inside the v tile: VPT consecutive doubles of one vector
    const int sg = (tid * VPT) / TILE, sc = (tid * VPT) % TILE;
    const double *vsrc = v + (int64_t)sg * P.vstride;

    double acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.0;

    for (int64_t c0 = cbeg; c0 < cend; c0 += TILE) {
        double2 a[SUB][RBW];
        const bool full = c0 + TILE <= cend;   // (a span need not be a whole number of tiles)
        if (full) {
#pragma unroll
            for (int u = 0; u < SUB; ++u)
#pragma unroll
                for (int r = 0; r < RBW; ++r) a[u][r] = ld_stream(Ar[r] + c0 + u * kStep + lane * 2);
#pragma unroll
            for (int k = 0; k < VPT; k += 2)
                *reinterpret_cast<double2 *>(&vt[sg][sc + k]) = ld_stream(vsrc + c0 + sc + k);
        } else {
#pragma unroll
            for (int u = 0; u < SUB; ++u) {
                const int64_t c = c0 + u * kStep + lane * 2;
#pragma unroll
                for (int r = 0; r < RBW; ++r)
                    a[u][r] = (c + 1 < cend) ? ld_stream(Ar[r] + c) : make_double2(c < cend ? Ar[r][c] : 0.0, 0.0);
            }
#pragma unroll
            for (int k = 0; k < VPT; ++k) vt[sg][sc + k] = (c0 + sc + k < cend) ? vsrc[c0 + sc + k] : 0.0;
        }
        __syncthreads();  // v tile staged
#pragma unroll
        for (int u = 0; u < SUB; ++u)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const double2 vv = *reinterpret_cast<const double2 *>(&vt[g][u * kStep + lane * 2]);
#pragma unroll
                for (int r = 0; r < RBW; ++r)
                    acc[r * G + g] = fma(a[u][r].y, vv.y, fma(a[u][r].x, vv.x, acc[r * G + g]));
            }
        __syncthreads();  // everyone done with the tile before it is overwritten
    }
    const double s = multi_reduce<NV>(acc, lane);
    constexpr int kShift = (NV >= 64) ? 0 : (NV == 32 ? 1 : NV == 16 ? 2 : 3);
    if ((lane & ((1 << kShift) - 1)) == 0) {
        const int idx = lane >> kShift, r = idx / G, g = idx - r * G;
        if (idx < NV && row0 + r < rows)
            P.partial[(int64_t)(g0 + g) * P.pstride + (int64_t)span * rows + row0 + r] = s;
    }
}

// y[r] = alpha * sum_span partial[span][r]
__global__ void gemv_rows_reduce_kernel(const double *partial, int64_t rows, int nspans, double alpha,
                                        double *y) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    double s = 0.0;
    for (int k = 0; k < nspans; ++k) s += partial[(int64_t)k * rows + r];
    y[r] = alpha * s;
}

// The span decomposition (span_cols, nspans -> layout of the partials) comes with the plan; the rows a block takes are
// a property of the kernel variant only: nblocks = ceil(rows / rows per block) * nspans.
static dim3 rows_grid(GemvRowsLaunch &L, int rows_per_block) {
    for (RowProblem &P : L.p) P.nblocks = P.nblocks ? (int)(ceil_div(P.rows, rows_per_block) * P.nspans) : 0;
    L.nblk0 = L.p[0].nblocks;
    return dim3(L.p[0].nblocks + L.p[1].nblocks);
}

int launch_rows_valu(GemvRowsLaunch L, const GemvPass &ps, hipStream_t st) {
    const dim3 grid = rows_grid(L, 8);
    if (ps.G == 2) hipLaunchKernelGGL((gemv_rows_kernel<8, 2>), grid, dim3(256), 0, st, L, ps.g0);
    else hipLaunchKernelGGL((gemv_rows_kernel<8, 1>), grid, dim3(256), 0, st, L, ps.g0);
    EVC_LAUNCH_CHECK("gemv_rows");
    return 0;
}

// (wave-rows kernels for 4 / 8 geometries: the lane-private ones were slower)
int launch_rows_wave_rows(GemvRowsLaunch L, const GemvPass &ps, hipStream_t st) {
    const dim3 grid = rows_grid(L, ps.G == 8 ? 16 : 32);   // four waves of RBW = 4 / 8 rows
    if (ps.G == 8) hipLaunchKernelGGL((gemv_rows_wr_kernel<4, 8, 4>), grid, dim3(256), 0, st, L, ps.g0);
    else hipLaunchKernelGGL((gemv_rows_wr_kernel<8, 4, 2>), grid, dim3(256), 0, st, L, ps.g0);
    EVC_LAUNCH_CHECK("gemv_rows");
    return 0;
}

int launch_rows_reduce(const double *partial, int64_t rows, int nspans, double alpha, double *y, hipStream_t st) {
    hipLaunchKernelGGL(gemv_rows_reduce_kernel, dim3((unsigned)ceil_div(rows, 256)), dim3(256), 0, st, partial, rows,
                       nspans, alpha, y);
    EVC_LAUNCH_CHECK("gemv_rows_reduce");
    return 0;
}

// ------------------------------------------------------------------ cols GEMV
// Each lane owns two adjacent columns and walks down the rows with kU independent 16-byte loads in
// flight.  G = 1: the row weights are wave-uniform scalar loads.  G > 1: the weights of a 512-row
// tile are staged in LDS as wl[row][g] and read back as broadcasts.
constexpr int kU = 16;
constexpr int kWTile = 512;

template <int G>
__global__ __launch_bounds__(256) void gemv_cols_kernel(GemvColsLaunch L, int g0) {
    __shared__ double wl[(G > 1) ? kWTile * G : 1];
    int bid = blockIdx.x;
    const int which = bid >= L.nblk0 ? 1 : 0;
    if (which) bid -= L.nblk0;
    const ColProblem &P = L.p[which];
    const int64_t c = (int64_t)bid * kChunk + threadIdx.x * 2;
    const bool active = c < P.cols;
    const bool two = c + 1 < P.cols;
    const double *__restrict__ A = P.A + (active ? c : 0);
    const double *__restrict__ w = P.w + (int64_t)g0 * P.wstride;
    const int64_t ld = P.ld;
    const int64_t rows = P.rows;
    double sx[G], sy[G];
#pragma unroll
    for (int g = 0; g < G; ++g) sx[g] = sy[g] = 0.0;

    if constexpr (G == 1) {
        if (active && two) {
            int64_t r = 0;
            for (; r + kU <= rows; r += kU) {
                double2 a[kU];
#pragma unroll
                for (int u = 0; u < kU; ++u) a[u] = ld_stream(A + (r + u) * ld);
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    const double wr = w[r + u];
                    sx[0] = fma(wr, a[u].x, sx[0]);
                    sy[0] = fma(wr, a[u].y, sy[0]);
                }
            }
            for (; r < rows; ++r) {
                const double2 a = ld_stream(A + r * ld);
                const double wr = w[r];
                sx[0] = fma(wr, a.x, sx[0]);
                sy[0] = fma(wr, a.y, sy[0]);
            }
        } else if (active) {
            for (int64_t r = 0; r < rows; ++r) sx[0] = fma(w[r], A[r * ld], sx[0]);
        }
    } else {
        for (int64_t r0 = 0; r0 < rows; r0 += kWTile) {
            const int nr = (int)min((int64_t)kWTile, rows - r0);
            __syncthreads();
            // consecutive lanes read consecutive rows of one geometry's weight vector (coalesced)
            for (int idx = threadIdx.x; idx < nr * G; idx += 256) {
                const int g = idx / nr, r = idx - g * nr;
                wl[r * G + g] = w[(int64_t)g * P.wstride + r0 + r];
            }
            __syncthreads();
            if (active && two) {
                int r = 0;
                for (; r + kU <= nr; r += kU) {
                    double2 a[kU];
#pragma unroll
                    for (int u = 0; u < kU; ++u) a[u] = ld_stream(A + (r0 + r + u) * ld);
#pragma unroll
                    for (int u = 0; u < kU; ++u)
#pragma unroll
                        for (int g = 0; g < G; ++g) {
                            const double wr = wl[(r + u) * G + g];
                            sx[g] = fma(wr, a[u].x, sx[g]);
                            sy[g] = fma(wr, a[u].y, sy[g]);
                        }
                }
                for (; r < nr; ++r) {
                    const double2 a = ld_stream(A + (r0 + r) * ld);
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        const double wr = wl[r * G + g];
                        sx[g] = fma(wr, a.x, sx[g]);
                        sy[g] = fma(wr, a.y, sy[g]);
                    }
                }
            } else if (active) {
                for (int r = 0; r < nr; ++r) {
                    const double ax = A[(r0 + r) * ld];
#pragma unroll
                    for (int g = 0; g < G; ++g) sx[g] = fma(wl[r * G + g], ax, sx[g]);
                }
            }
        }
    }
    if (active) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            double *o = P.out + (int64_t)(g0 + g) * P.ostride + c;
            if (two) *reinterpret_cast<double2 *>(o) = make_double2(sx[g], sy[g]);
            else *o = sx[g];
        }
    }
}

// Row-split variant for matrices with few columns (the 8-fold compressed layout: 212 chunks of 512 columns do not
// fill 256 CUs): a block owns 128 columns, its four waves take every fourth group of 8 rows and the four partial
// sums are added in fixed order through LDS.  The row weights are wave-uniform loads.
template <int G>
__global__ __launch_bounds__(256) void gemv_cols_rs_kernel(GemvColsLaunch L, int g0) {
    __shared__ double2 red[4][G][64];
    constexpr int U = 16;
    int bid = blockIdx.x;
    const int which = bid >= L.nblk0 ? 1 : 0;
    if (which) bid -= L.nblk0;
    const ColProblem &P = L.p[which];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c = (int64_t)bid * 128 + lane * 2;
    const bool active = c < P.cols;
    const bool two = c + 1 < P.cols;
    const double *__restrict__ A = P.A + (active ? c : 0);
    const double *__restrict__ w = P.w + (int64_t)g0 * P.wstride;
    const int64_t ld = P.ld, rows = P.rows;
    double sx[G], sy[G];
#pragma unroll
    for (int g = 0; g < G; ++g) sx[g] = sy[g] = 0.0;
    if (active) {
        for (int64_t r = (int64_t)wave * U; r < rows; r += 4 * U) {
            double2 a[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t rr = r + u < rows ? r + u : rows - 1;   // clamped rows get weight 0 below
                a[u] = two ? ld_stream(A + rr * ld) : make_double2(A[rr * ld], 0.0);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const double wr = r + u < rows ? w[(int64_t)g * P.wstride + r + u] : 0.0;
                    sx[g] = fma(wr, a[u].x, sx[g]);
                    sy[g] = fma(wr, a[u].y, sy[g]);
                }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) red[wave][g][lane] = make_double2(sx[g], sy[g]);
    __syncthreads();
    for (int idx = threadIdx.x; idx < G * 64; idx += 256) {
        const int g = idx >> 6, ln = idx & 63;
        const int64_t cc = (int64_t)bid * 128 + ln * 2;
        if (cc < P.cols) {
            const double2 p0 = red[0][g][ln], p1 = red[1][g][ln], p2 = red[2][g][ln], p3 = red[3][g][ln];
            const double vx = (p0.x + p1.x) + (p2.x + p3.x), vy = (p0.y + p1.y) + (p2.y + p3.y);
            double *o = P.out + (int64_t)(g0 + g) * P.ostride + cc;
            if (cc + 1 < P.cols) *reinterpret_cast<double2 *>(o) = make_double2(vx, vy);
            else *o = vx;
        }
    }
}

// Row-slab form for a NARROW matrix with MANY rows -- the one-body t-RDM of a large training set, (T^2, N^2): 10 000 x 784
// at the Zundel shape with 100 training states.  The column-tiled kernels above give such a matrix two to seven
// workgroups that walk all its rows (0.3 ms at 0.2 TB/s, the tail of the whole K8 launch); here a workgroup takes a slab
// of rows x 512 columns (whole rows: 4-6 KB contiguous per row), eight geometries at a time, and leaves a partial row;
// a second, tiny launch adds the slabs in fixed order.
__global__ __launch_bounds__(256) void gemv_cols_slab_kernel(ColProblem P, int count, int nslab) {
    const int slab = blockIdx.x;
    const int64_t c = (int64_t)blockIdx.y * kChunk + threadIdx.x * 2;
    const bool active = c < P.cols, two = c + 1 < P.cols;
    const int64_t rps = (P.rows + nslab - 1) / nslab, r0 = (int64_t)slab * rps, r1 = min(P.rows, r0 + rps);
    const double *__restrict__ A = P.A + (active ? c : 0);
    for (int gb = 0; gb < count; gb += 8) {
        const int ng = min(8, count - gb);
        double2 acc[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) acc[g] = make_double2(0.0, 0.0);
        if (active) {
            int64_t r = r0;
            for (; r + 8 <= r1; r += 8) {   // eight independent row loads in flight
                double2 a[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) a[u] = two ? ld_stream(A + (r + u) * P.ld) : make_double2(A[(r + u) * P.ld], 0.0);
#pragma unroll
                for (int g = 0; g < 8; ++g)
                    if (g < ng) {
                        const double *wp = P.w + (int64_t)(gb + g) * P.wstride + r;
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            acc[g].x = fma(wp[u], a[u].x, acc[g].x);
                            acc[g].y = fma(wp[u], a[u].y, acc[g].y);
                        }
                    }
            }
            for (; r < r1; ++r) {
                const double2 a = two ? ld_stream(A + r * P.ld) : make_double2(A[r * P.ld], 0.0);
#pragma unroll
                for (int g = 0; g < 8; ++g)
                    if (g < ng) {
                        const double wr = P.w[(int64_t)(gb + g) * P.wstride + r];
                        acc[g].x = fma(wr, a.x, acc[g].x);
                        acc[g].y = fma(wr, a.y, acc[g].y);
                    }
            }
#pragma unroll
            for (int g = 0; g < 8; ++g)
                if (g < ng) {
                    double *o = P.part + (int64_t)(gb + g) * P.pstride + (int64_t)slab * P.ld + c;
                    if (two) *reinterpret_cast<double2 *>(o) = acc[g];
                    else *o = acc[g].x;
                }
        }
    }
}

__global__ __launch_bounds__(256) void gemv_cols_slab_reduce_kernel(ColProblem P, int nslab) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= P.cols) return;
    const double *p = P.part + (int64_t)blockIdx.y * P.pstride + c;
    double s0 = 0.0, s1 = 0.0;
    int k = 0;
    for (; k + 2 <= nslab; k += 2) {
        s0 += p[(int64_t)k * P.ld];
        s1 += p[(int64_t)(k + 1) * P.ld];
    }
    if (k < nslab) s0 += p[(int64_t)k * P.ld];
    P.out[(int64_t)blockIdx.y * P.ostride + c] = s0 + s1;
}

// G = 1, 2, 4 or 8 geometries [g0, g0 + G): the column-tiled kernel, 512 columns per block
int launch_cols_valu(GemvColsLaunch L, const GemvPass &ps, hipStream_t st) {
    L.nblk0 = (int)ceil_div(L.p[0].cols, kChunk);
    const dim3 grid(L.nblk0 + (int)ceil_div(L.p[1].cols, kChunk));
    if (ps.G == 8) hipLaunchKernelGGL((gemv_cols_kernel<8>), grid, dim3(256), 0, st, L, ps.g0);
    else if (ps.G == 4) hipLaunchKernelGGL((gemv_cols_kernel<4>), grid, dim3(256), 0, st, L, ps.g0);
    else if (ps.G == 2) hipLaunchKernelGGL((gemv_cols_kernel<2>), grid, dim3(256), 0, st, L, ps.g0);
    else hipLaunchKernelGGL((gemv_cols_kernel<1>), grid, dim3(256), 0, st, L, ps.g0);
    EVC_LAUNCH_CHECK("gemv_cols");
    return 0;
}

// ... the row-split kernel, 128 columns per block
int launch_cols_valu_rs(GemvColsLaunch L, const GemvPass &ps, hipStream_t st) {
    L.nblk0 = (int)ceil_div(L.p[0].cols, 128);
    const dim3 grid(L.nblk0 + (int)ceil_div(L.p[1].cols, 128));
    if (ps.G == 8) hipLaunchKernelGGL((gemv_cols_rs_kernel<8>), grid, dim3(256), 0, st, L, ps.g0);
    else if (ps.G == 4) hipLaunchKernelGGL((gemv_cols_rs_kernel<4>), grid, dim3(256), 0, st, L, ps.g0);
    else if (ps.G == 2) hipLaunchKernelGGL((gemv_cols_rs_kernel<2>), grid, dim3(256), 0, st, L, ps.g0);
    else hipLaunchKernelGGL((gemv_cols_rs_kernel<1>), grid, dim3(256), 0, st, L, ps.g0);
    EVC_LAUNCH_CHECK("gemv_cols");
    return 0;
}

// the narrow problem L.p[1] in row slabs for all ps.G geometries: the slab launch and the fixed-order sum of the slabs
int launch_cols_slab(GemvColsLaunch L, const GemvPass &ps, hipStream_t st) {
    const ColProblem &P = L.p[1];
    const int nslab = (int)(P.rows / 64 < kColSlabs ? P.rows / 64 : kColSlabs);
    hipLaunchKernelGGL(gemv_cols_slab_kernel, dim3((unsigned)nslab, (unsigned)ceil_div(P.cols, kChunk)), dim3(256), 0, st,
                       P, ps.G, nslab);
    EVC_LAUNCH_CHECK("gemv_cols_slab");
    hipLaunchKernelGGL(gemv_cols_slab_reduce_kernel, dim3((unsigned)ceil_div(P.cols, 256), (unsigned)ps.G), dim3(256), 0,
                       st, P, nslab);
    EVC_LAUNCH_CHECK("gemv_cols_slab_reduce");
    return 0;
}

}  // namespace evc
