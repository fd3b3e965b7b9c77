// The 8-fold compressed vector p8 of a fully symmetric 2-RDM (EVC_LAYOUT_SYM8) -> the dense symmetric (pair, pair) matrix
// SB[u][v] = 4 p8[tri(max(u,v), min(u,v))] at the row pitch pair_ld(n), as a mirrored-tile copy (unpack8_prep_kernel of
// grad_tail.hip and unpack8_pairs_kernel of pack.hip).
// Work unit of a workgroup: ONE tile of kUtRows rows x kUtCols columns of one geometry's lower triangle, rows u0 = 64 I,
// columns v0 = 32 J, J < min(2 I + 2, column blocks): every tile that holds an element v <= u.  In packed storage the row
// segment p[tri(u, v0) ..] is contiguous, so a wave's load instruction reads two runs of 256 bytes; a thread requests its
// eight elements before it uses the first.  The tile goes to SB[u][v0 ..] straight from the registers and to
// SB[v][u0 ..], the mirror image, through a transposed LDS copy (pitch 65: the writes of a 32-lane group fall on 32
// different banks, the reads run along a row), in runs of 512 bytes.
// Positions of a tile without an element of packed storage (v > u above the diagonal, u >= npairs below the last row)
// stand for the nearest one that has one, (uc, vc) = (min(u, npairs - 1), min(v, uc)): they load it and store it where
// it belongs, SB[uc][vc] and SB[vc][uc] -- the value some other lane writes there as well.  So no load and no store
// stands under a condition (a store that may or may not have been issued turns the compiler's counted waits into
// waits for everything before it), nothing is read beyond tri(npairs - 1, npairs - 1), no row or column >= npairs is
// written (the columns between npairs and the pitch stay as they are), and what the mirror image of a tile on the
// diagonal lacks (v > u) comes from the tiles below it.
// N = 30: 71 tiles per geometry, 2272 workgroups for 32 geometries, three resident per CU in unpack8_prep_kernel (the
// 52 KB of LDS that ride with grad_prep).  Measured there, one stream (profiles/r06_*): 17.4-18.6 us against 23.6-25.6 of
// the row-per-wave gather; two / three tiles per workgroup with all their loads requested up front 19.1 / 19.3-20.2,
// tiles of 32 x 32 19.7-20.2, 128 x 32 19.8-20.0, 64 x 64 17.7.
#pragma once
#include "common.hpp"

namespace evc {

constexpr int kUtRows = 64, kUtCols = 32, kUtPitch = kUtRows + 1;
constexpr int kUtLoadRows = 256 / kUtCols, kUtMirrorCols = 256 / kUtRows;   // rows / columns 256 threads cover per instruction
constexpr size_t kUtLds = sizeof(double) * kUtCols * kUtPitch;              // bytes of dynamic LDS: the transposed tile

// column blocks of row block I that hold an element of the lower triangle
__host__ __device__ inline int unpack_tile_cols(int npairs, int I) {
    const int ncb = (npairs + kUtCols - 1) / kUtCols, want = ((I + 1) * kUtRows + kUtCols - 1) / kUtCols;
    return want < ncb ? want : ncb;
}

// tiles = workgroups (of 256 threads) per geometry
__host__ __device__ inline int unpack_tile_count(int npairs) {
    int t = 0;
    for (int I = 0; I * kUtRows < npairs; ++I) t += unpack_tile_cols(npairs, I);
    return t;
}

// Block b of count * bpg -> (geometry, block of the geometry).  Blocks of eight consecutive geometries interleaved: the
// workgroups are dealt round-robin to the 8 XCDs, so each XCD works through one geometry's packed vector at a time; the
// count % 8 last geometries in plain (geometry, block) order.
__device__ __forceinline__ void unpack_tile_geom(int64_t b, int count, int bpg, int &geom, int &blk) {
    const int nx = count & ~7;
    if (b < (int64_t)nx * bpg) {
        const int xcd = (int)(b & 7), slot = (int)(b >> 3);
        geom = (slot / bpg) * 8 + xcd;
        blk = slot % bpg;
    } else {
        const int64_t r = b - (int64_t)nx * bpg;
        geom = nx + (int)(r / bpg);
        blk = (int)(r % bpg);
    }
}

// Tile t < unpack_tile_count(npairs) of ONE geometry (p: its packed vector, sb: its dense matrix) by a workgroup of 256
// threads; tile: kUtLds bytes of LDS.
__device__ __forceinline__ void unpack8_tile(const double *__restrict__ p, double *__restrict__ sb, int npairs, int ld,
                                             int t, double *tile) {
    constexpr int kPer = kUtRows * kUtCols / 256;   // elements of the tile per thread
    const int tid = threadIdx.x;
    const int lc = tid % kUtCols, lr = tid / kUtCols;   // load and direct store: column lc, rows lr + 8 k
    const int mr = tid % kUtRows, mc = tid / kUtRows;   // mirrored store: tile row mr (along the run), tile columns mc + 4 k
    int I = 0, J = t;
    for (int nc; J >= (nc = unpack_tile_cols(npairs, I)); ++I) J -= nc;
    const int u0 = I * kUtRows, v0 = J * kUtCols, ulast = npairs - 1;
    double x[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int u = u0 + lr + kUtLoadRows * k, v = v0 + lc;
        const int uc = u < ulast ? u : ulast, vc = v < uc ? v : uc;
        x[k] = p[tri_index(uc, vc)];
    }
    __builtin_amdgcn_sched_barrier(0);   // (every load is requested before the first is waited for)
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int u = u0 + lr + kUtLoadRows * k, v = v0 + lc;
        const int uc = u < ulast ? u : ulast, vc = v < uc ? v : uc;
        const double y = 4.0 * x[k];
        sb[(int64_t)uc * ld + vc] = y;
        tile[lc * kUtPitch + lr + kUtLoadRows * k] = y;
    }
    lds_barrier();
    double y[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) y[k] = tile[(mc + kUtMirrorCols * k) * kUtPitch + mr];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int u = u0 + mr, v = v0 + mc + kUtMirrorCols * k;
        const int uc = u < ulast ? u : ulast, vc = v < uc ? v : uc;
        sb[(int64_t)vc * ld + uc] = y[k];
    }
}

}  // namespace evc
