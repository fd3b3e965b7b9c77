// The batched streaming contractions with the t-RDM streamed through LDS by LDS-DMA (lds_dma.hpp).
// K5 (this file; batches of 12 .. 64 geometries per pass); K8 (17 .. 32): gemv_cols_lds.hip.
//   Y[row][g] = sum_c A[row][c] v[g][c]      (reference: ab_initio_eigenvector_continuation.py:57-64, the
//   np.einsum / np.sum contractions of the stored transition RDMs with the rotated integrals)
//
// Why a second rows kernel (round 3, tools/micro/rows_pattern.hip with the caches flushed by a READ of 2 GB before
// every launch): the fragment-shaped loads of gemv_rows_mfma_pipe_kernel (a load instruction = 16 rows x 64 bytes)
// read the 210 x 108 345 matrix COLD at 4.0 TB/s, whole-line pieces at 5.0 TB/s -- the earlier comparison (5.5 against
// 5.9 TB/s) had the 182 MB matrix sitting in the 256 MB memory-side cache between the repeats, which the kernel in
// situ never sees (a batch moves 1.4 GB between two passes over the matrix).  Here every load instruction moves
// 8 rows x 128 bytes (whole cache lines) straight into LDS, no VGPRs in between, so one wave per SIMD keeps a whole
// image (30-34 instructions = 30-34 KB) in flight, and the MFMA fragments come out of LDS with ds_read_b128.
//
// Decomposition: block = (column span, row group of NT 16-row tiles), one block per CU, exactly as many blocks as
// units of work (host-built block table).  The four waves interleave the 16-column chunks of the span (128 bytes per
// row: one cache line) and are completely independent until the epilogue: no barrier in the stream.  A wave's LDS
// image holds NCH chunks, each GS tiles of geometry vectors (16 geometries x 16 columns) followed by NT tiles of
// matrix rows, 2 KB per tile.  Slot p of the image is refilled for the NEXT image one position after it was read, so
// the image is a sliding window and (NSI - 1) tiles = 2 (NSI - 1) instructions are in flight all the time; LDS-DMA
// completes in order, so the wait in front of the reads of slot p is the constant vmcnt(2 (NSI - 2)).
// Shapes (NT, NCH) = (14,1) (7,2) (4,3) (2,4): see lds_pick_nt (gemv_dispatch.hip) for what the row groups buy.
//
// LDS image of a tile (rule "linear destination, swizzled SOURCE, same swizzle on the read"): instruction j of a
// tile writes 1 KB = rows 8j..8j+7 x 128 bytes, lane i -> row 8j + (i >> 3), 16-byte position i & 7; the position
// holds piece q = pos ^ ((row >> 1) & 7) of the row.  A fragment read (ds_read_b128: lane (l15, l4) takes piece
// 4u + l4 of row l15) is then conflict free in every 16-lane group of the instruction (SQ_LDS_BANK_CONFLICT = 0,
// profiles/r03_pmc_lds_sym8_batch32.csv).
#include <stdlib.h>

#include "common.hpp"
#include "kernels.hpp"
#include "lds_dma.hpp"

namespace evc {

namespace {

constexpr int kLW = kLdsChunkCols;  // columns per wave chunk
constexpr int kTileBytes = 2048;  // 16 rows x 16 columns

// two columns of the ragged last chunk, zero beyond the matrix
__device__ __forceinline__ double2 ld2g(const double *row, int64_t c, int64_t cols) {
    if (c + 1 < cols) return *reinterpret_cast<const double2 *>(row + c);
    return make_double2(c < cols ? row[c] : 0.0, 0.0);
}

}  // namespace

// Timing experiments (tools/micro/k5_stamps.py; build with EVC_DEBUG_STAMPS=1), compiled out of the product library.
#ifdef EVC_DEBUG_STAMPS
__device__ long long g_k5l_wg[1024 * 8];   // per workgroup: entry, main loop done (wave 0), exit, hw id, 4 epilogue stamps
#define EVC_K5L_WG(i_)                                                                 \
    do {                                                                               \
        if (threadIdx.x == 0 && blockIdx.x < 1024) {                                   \
            long long t_;                                                              \
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
            g_k5l_wg[8 * blockIdx.x + (i_)] = t_;                                      \
            if ((i_) == 0) {                                                           \
                unsigned hw_, xcc_;                                                    \
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_));      \
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));    \
                g_k5l_wg[8 * blockIdx.x + 3] = ((long long)(xcc_ & 0xF) << 32) | hw_;  \
            }                                                                          \
        }                                                                              \
    } while (0)
#else
#define EVC_K5L_WG(i_) do { } while (0)
#endif

// block -> which << 15 | row group << 8 | span (lds_block_map below)
struct LdsBlockMap {
    unsigned short e[256];
};

// One wave's state: everything the unrolled body needs.  NCH chunks (consecutive chunks of this wave, 64 columns
// apart) make one image of NSI = NCH (NT + GS) slots.
template <int GS, int NT, int NCH>
struct LdsRowsWave {
    static constexpr int NS = NT + GS;
    static constexpr int NSI = NS * NCH;
    const char *abase;       // first row of the row group, column 0 (wave-uniform)
    int64_t tile_stride;     // 16 rows in bytes
    int rows_left;           // rows of the matrix from the row group's first row on (>= 1)
    int64_t ld;
    int64_t clast;           // first column of this wave's last complete chunk (chunks beyond it re-read it)
    const char *vb[GS][2];   // per lane: its 16 bytes of its geometry's vector at column 0, both instructions of a tile
    unsigned voff[2];        // per lane: its 16 bytes relative to the tile's first row, column 0 (full tiles)
    unsigned lbase;          // LDS byte address of this wave's image
    int prow, ppiece;        // producer: row within the 8-row piece (lane >> 3) and 16-byte position (lane & 7)
    unsigned raddr[2];       // consumer: byte offset of (row l15, k pair u) within a tile

    // refill slot S of the image whose first chunk starts at column c0
    template <int S>
    __device__ __forceinline__ void issue(int64_t c0) const {
        constexpr int j = S / NS, sl = S % NS;
        const unsigned la = lbase + S * kTileBytes;
        int64_t cc = c0 + j * (4 * kLW);
        if (NCH > 1 && cc > clast) cc = clast;   // (a chunk the wave does not have: valid bytes, never consumed)
        if constexpr (sl < GS) {
            glds_v(vb[sl][0] + cc * 8, la);
            glds_v(vb[sl][1] + cc * 8, la + 1024);
        } else {
            constexpr int t = sl - GS;
            const int left = rows_left - 16 * t;   // rows of the matrix in and below this tile (wave-uniform)
            if (left >= 16) {
                const char *sb = abase + t * tile_stride + cc * 8;
                glds_s(voff[0], sb, la);
                glds_s(voff[1], sb, la + 1024);
            } else {
                // ragged or empty tile: rows beyond the matrix re-read its last row (their results are discarded)
                const int first = left >= 1 ? 16 * t : rows_left - 1;   // first row fetched, relative to the group
                const int last = left >= 1 ? left - 1 : 0;              // last valid row relative to `first`
                const char *sb = abase + (int64_t)first * ld * 8 + cc * 8;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int r = 8 * jj + prow;
                    const int q = ppiece ^ ((r >> 1) & 7);
                    const int rc = r < last ? r : last;
                    glds_s((unsigned)(((int64_t)rc * ld + 2 * q) * 8), sb, la + 1024 * jj);
                }
            }
        }
    }
};

// slot index known after unrolling: the chain folds to the one call
template <int GS, int NT, int NCH, int S = 0>
__device__ __forceinline__ void lds_issue_dyn(const LdsRowsWave<GS, NT, NCH> &w, int s, int64_t c0) {
    if constexpr (S < (NT + GS) * NCH) {
        if (s == S) w.template issue<S>(c0);
        else lds_issue_dyn<GS, NT, NCH, S + 1>(w, s, c0);
    }
}
// slots 0 .. NSI-2 (the prologue: slot NSI-1 is requested by position 0 of the image itself)
template <int GS, int NT, int NCH, int S = 0>
__device__ __forceinline__ void lds_issue_range(const LdsRowsWave<GS, NT, NCH> &w, int64_t c0) {
    if constexpr (S < (NT + GS) * NCH - 1) {
        w.template issue<S>(c0);
        lds_issue_range<GS, NT, NCH, S + 1>(w, c0);
    }
}

// GS sets of 16 geometries [g0, g0 + G), 16 (GS - 1) < G <= 16 GS; NT = tiles per row group (every row group runs NT
// tiles: tiles beyond the group's own are fetched from valid rows and discarded); NCH = chunks per image.
template <int GS, int NT, int NCH>
__global__ __launch_bounds__(256, 1) void gemv_rows_lds_kernel(GemvRowsLaunch L, LdsBlockMap M, int g0, int G) {
    extern __shared__ __align__(16) double lds_img[];
    using W = LdsRowsWave<GS, NT, NCH>;
    constexpr int NS = W::NS, NSI = W::NSI;
    constexpr int IMG = NSI * kTileBytes;   // bytes per wave
    // block -> (problem, span, row group) by the host's table: exactly one block per unit of work -- one workgroup
    // fits a CU, a launch of more blocks than CUs runs its last blocks in a second round (measured: +20 us)
    const unsigned e = M.e[blockIdx.x];
    const int which = e >> 15, rg = (e >> 8) & 127, span = e & 255;
    EVC_K5L_WG(0);
    const RowProblem &P = L.p[which];
    const int64_t rows = P.rows, cols = P.cols, ld = P.ld;
    const int tpg = L.tpg[which], trem = L.trem[which];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const int64_t row_base = (int64_t)(rg * tpg + min(rg, trem)) * 16;
    const int ntile = tpg + (rg < trem ? 1 : 0);  // tiles of this row group (the last one may be ragged)
    const int64_t cbeg = (int64_t)span * P.span_cols;
    const int64_t cend = min(cols, (int64_t)(span + 1) * P.span_cols);
    const int64_t cfull = min(cend, cols & ~(int64_t)(kLW - 1));   // chunks starting below this are complete
    int64_t c = cbeg + wave * kLW;
    const int nmy = c < cfull ? (int)((cfull - c + 4 * kLW - 1) / (4 * kLW)) : 0;   // complete chunks of this wave

    W w;
    w.abase = reinterpret_cast<const char *>(P.A + row_base * ld);
    w.tile_stride = 16 * ld * 8;
    w.rows_left = (int)(rows - row_base);
    w.ld = ld;
    w.clast = c + (int64_t)(nmy > 0 ? nmy - 1 : 0) * (4 * kLW);
    w.prow = lane >> 3;
    w.ppiece = lane & 7;
    w.lbase = (unsigned)(wave * IMG);   // the dynamic array is the only LDS of this kernel: it starts at address 0
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = 8 * j + w.prow;
        const int q = w.ppiece ^ ((r >> 1) & 7);
        w.voff[j] = (unsigned)(((int64_t)r * ld + 2 * q) * 8);
#pragma unroll
        for (int gs = 0; gs < GS; ++gs) {
            const int slot = 16 * gs + r;
            const int gg = g0 + (slot < G ? slot : 0);   // slots beyond G read geometry g0 (a valid address)
            w.vb[gs][j] = reinterpret_cast<const char *>(P.v + (int64_t)gg * P.vstride + 2 * q);
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
        w.raddr[u] = (unsigned)((l15 >> 3) * 1024 + (l15 & 7) * 128 + (((4 * u + l4) ^ ((l15 >> 1) & 7)) * 16));

    d4 acc[GS][NT];
#pragma unroll
    for (int gs = 0; gs < GS; ++gs)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[gs][t] = (d4){0.0, 0.0, 0.0, 0.0};

    const char *img = reinterpret_cast<const char *>(lds_img) + wave * IMG;
    double2 bf[GS][2], bfn[GS][2];   // geometry-vector fragments of the chunk in work / of the chunk being opened
    double2 af[2][2];                // matrix fragments, alternating tiles
#define EVC_LDS_MMA(T_, AF_)                                                                    \
    {                                                                                           \
        _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                         \
            _Pragma("unroll") for (int gs = 0; gs < GS; ++gs)                                   \
                acc[gs][T_] = mfma_f64(AF_[u].x, bf[gs][u].x, acc[gs][T_]);                       \
            _Pragma("unroll") for (int gs = 0; gs < GS; ++gs)                                   \
                acc[gs][T_] = mfma_f64(AF_[u].y, bf[gs][u].y, acc[gs][T_]);                       \
        }                                                                                       \
    }
// One image: chunks at C0_, C0_ + 64, ... of which NV_ are the wave's own; NEXT_: another image follows at CN_ (its slots
// are refilled one position behind the reads).  PEND_: the last matrix tile of the chunk before still waits for its MFMAs
// (they run behind the first fragment read of the next chunk, so no LDS latency is exposed between chunks).
// Position p = (chunk j of the image, slot sl): wait for slot p, read its fragments, run the MFMAs of the tile before,
// refill slot p - 1 (position 0: the image's own last slot).  LDS-DMA completes in order and NSI - 2 tiles are
// younger than slot p whenever it is waited for: the constant vmcnt(2 (NSI - 2)) in the stream, counted down in the
// last image.
#define EVC_LDS_IMAGE(NEXT_, C0_, CN_, NV_)                                                                 \
    {                                                                                                       \
        _Pragma("unroll") for (int p = 0; p < NSI; ++p) {                                                   \
            const int j = p / NS, sl = p - j * NS;                                                          \
            wait_vm_n((NEXT_) || p == 0 ? 2 * (NSI - 2) : (p < NSI - 1 ? 2 * (NSI - 1 - p) : 0));            \
            if (j < (NV_)) {                                                                                \
                const char *tp = img + p * kTileBytes;                                                      \
                if (sl < GS) {                                                                              \
                    _Pragma("unroll") for (int u = 0; u < 2; ++u)                                           \
                        bfn[sl < GS ? sl : 0][u] = *reinterpret_cast<const double2 *>(tp + w.raddr[u]);     \
                    if (sl == 0 && pend) EVC_LDS_MMA(NT - 1, af[(NS - 1) & 1])                              \
                } else {                                                                                    \
                    if (sl == GS) {                                                                         \
                        _Pragma("unroll") for (int gs = 0; gs < GS; ++gs)                                   \
                            _Pragma("unroll") for (int u = 0; u < 2; ++u) bf[gs][u] = bfn[gs][u];           \
                    }                                                                                       \
                    _Pragma("unroll") for (int u = 0; u < 2; ++u)                                           \
                        af[sl & 1][u] = *reinterpret_cast<const double2 *>(tp + w.raddr[u]);                \
                    if (sl >= GS + 1) EVC_LDS_MMA(sl - GS - 1 >= 0 ? sl - GS - 1 : 0, af[(sl - 1) & 1])     \
                    if (sl == NS - 1) pend = true;                                                          \
                }                                                                                           \
            }                                                                                               \
            __builtin_amdgcn_sched_barrier(0);                                                              \
            wait_lds();   /* the reads of slot p - 1 (and of slot p) have left LDS: the slot may be refilled */ \
            if (p == 0) w.template issue<NSI - 1>(C0_);                                                     \
            else if (NEXT_) lds_issue_dyn<GS, NT, NCH>(w, p - 1, CN_);                                      \
        }                                                                                                   \
    }
    bool pend = false;
    if (nmy > 0) {
        lds_issue_range<GS, NT, NCH>(w, c);   // slots 0 .. NSI-2 of the first image
        int left = nmy;
        for (; left > NCH; left -= NCH) {
            EVC_LDS_IMAGE(true, c, c + NCH * 4 * kLW, NCH)
            c += NCH * 4 * kLW;
        }
        EVC_LDS_IMAGE(false, c, c, left)
        EVC_LDS_MMA(NT - 1, af[(NS - 1) & 1])   // (pend is set: the image held at least one chunk)
    }
#undef EVC_LDS_IMAGE
    // the ragged last chunk of the matrix (fewer than 16 columns): the wave whose turn it is, with guarded loads
    const int64_t ctail = cols & ~(int64_t)(kLW - 1);
    if (ctail < cols && ctail >= cbeg && ctail < cend && (int)(((ctail - cbeg) / kLW) & 3) == wave) {
        wait_vm<0>();
#pragma unroll
        for (int gs = 0; gs < GS; ++gs) {
            const int slot = 16 * gs + l15;
            const double *vr = P.v + (int64_t)(g0 + (slot < G ? slot : 0)) * P.vstride;
#pragma unroll
            for (int u = 0; u < 2; ++u) bf[gs][u] = ld2g(vr, ctail + 8 * u + 2 * l4, cols);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const double *ar = P.A + min(row_base + 16 * t + l15, rows - 1) * ld;
#pragma unroll
            for (int u = 0; u < 2; ++u) af[0][u] = ld2g(ar, ctail + 8 * u + 2 * l4, cols);
            EVC_LDS_MMA(t, af[0])
        }
    }
#undef EVC_LDS_MMA
    EVC_K5L_WG(1);
    // Cross-wave sum through the (now idle) images, one geometry set per pass, as a reduce-scatter: tile tt belongs to
    // wave tt & 3; the other three waves file their accumulators of it in the accumulator's own layout
    // ([tile][copy][half][lane][2 doubles]: 16-byte LDS accesses, lanes 16 bytes apart), the owner adds the four in wave order --
    // (w0 + w1) + (w2 + w3), whoever owns the tile -- and stores the tile straight from its registers.
    wait_vm<0>();
    d2 *red = reinterpret_cast<d2 *>(lds_img);
#pragma unroll
    for (int gs = 0; gs < GS; ++gs) {
        __syncthreads();
        if (gs == 0) EVC_K5L_WG(4);
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
            if ((tt & 3) != wave) {
                const int k = (wave - (tt & 3) - 1) & 3;   // 0..2: wave owner+1+k
                // (two 16-byte planes: consecutive lanes 16 bytes apart -- a 32-byte lane pitch is a 2-way conflict)
                red[((tt * 3 + k) * 2 + 0) * 64 + lane] = (d2){acc[gs][tt][0], acc[gs][tt][1]};
                red[((tt * 3 + k) * 2 + 1) * 64 + lane] = (d2){acc[gs][tt][2], acc[gs][tt][3]};
            }
        }
        if (gs == 0) EVC_K5L_WG(5);
        __syncthreads();
        if (gs == 0) EVC_K5L_WG(6);
        const int g = 16 * gs + l15;
        double *dst = P.partial + (int64_t)(g0 + g) * P.pstride + (int64_t)span * rows + row_base + l4;
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
            if ((tt & 3) == wave && tt < ntile) {
                d4 v[4];
                v[tt & 3] = acc[gs][tt];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const d2 lo = red[((tt * 3 + k) * 2 + 0) * 64 + lane], hi = red[((tt * 3 + k) * 2 + 1) * 64 + lane];
                    v[((tt & 3) + 1 + k) & 3] = (d4){lo[0], lo[1], hi[0], hi[1]};
                }
                const d4 sum = (v[0] + v[1]) + (v[2] + v[3]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t row = row_base + tt * 16 + l4 + 4 * r;
                    if (row < rows && g < G) dst[tt * 16 + 4 * r] = sum[r];
                }
            }
        }
        if (gs == 0) EVC_K5L_WG(7);
    }
    EVC_K5L_WG(2);
}

// ---------------------------------------------------------------------------------- host side
// These kernels put ONE workgroup on a CU (their LDS images fill it) and size their grids for a whole MI355X (kLdsBlocks,
// kLdsBlocksSmall of kernels.hpp): the plan of gemv_dispatch.hip names them only on a device with that many CUs, and
// chooses the kernel shape (NT tiles per row group, NCH chunks per image: every shape keeps 16-18 tiles = 32-36 KB in
// flight per wave) and the span decomposition with it.

// Blocks are dealt to the 8 XCDs round-robin by their index (each XCD has its own L2): the row groups of one span,
// which read the same pieces of the geometry vectors, get indices that are congruent mod 8 as long as the XCD has
// `nrg` indices left; the last spans take what remains.  The small problem's blocks come first.
static void lds_block_map(const GemvRowsLaunch &L, int nb1, int nb0, LdsBlockMap &M) {
    int n = 0;
    for (int b = 0; b < nb1; ++b) M.e[n++] = (unsigned short)(1u << 15 | (unsigned)(b % L.nrg[1]) << 8 | (unsigned)(b / L.nrg[1]));
    int next[8], left[8];   // next free index of each XCD, indices it has left
    for (int x = 0; x < 8; ++x) {
        next[x] = nb1 + ((x - nb1) & 7);
        left[x] = next[x] < nb1 + nb0 ? (nb1 + nb0 - 1 - next[x]) / 8 + 1 : 0;
    }
    const int nrg = L.nrg[0];
    int x = nb1 & 7;
    for (int s = 0; s < L.p[0].nspans; ++s) {
        int pick = -1;
        for (int k = 0; k < 8 && pick < 0; ++k)   // round-robin over the XCDs that can still take a whole span
            if (left[(x + k) & 7] >= nrg) pick = (x + k) & 7;
        for (int rg = 0; rg < nrg; ++rg) {
            int xx = pick;
            if (xx < 0) {   // no XCD has room for the whole span: the one with the most indices left, block by block
                xx = 0;
                for (int k = 1; k < 8; ++k)
                    if (left[k] > left[xx]) xx = k;
            }
            M.e[next[xx]] = (unsigned short)((unsigned)rg << 8 | (unsigned)s);
            next[xx] += 8;
            --left[xx];
        }
        if (pick >= 0) x = (pick + 1) & 7;
    }
}

template <int GS, int NT, int NCH>
static int lds_launch(const GemvRowsLaunch &L, const LdsBlockMap &M, int nblocks, int g0, int G, hipStream_t st) {
    constexpr int lds = 4 * (NT + GS) * NCH * kTileBytes;
    static LdsAttr attr;
    if (int rc = allow_dynamic_lds(gemv_rows_lds_kernel<GS, NT, NCH>, attr, lds, "gemv_rows_lds")) return rc;
    hipLaunchKernelGGL((gemv_rows_lds_kernel<GS, NT, NCH>), dim3(nblocks), dim3(256), lds, st, L, M, g0, G);
    EVC_LAUNCH_CHECK("gemv_rows_lds");
    return 0;
}

// <GS, NT, NCH> = ps.t: one kernel shape per launch, the large problem's (the small problem's row groups are dealt for
// the same shape).  Four geometry sets (33 .. 64 geometries per pass): 8 accumulator registers per (set, tile) -- 7 tiles
// at most -- and fewer chunks per image, the four vector tiles of a chunk count.
int launch_rows_lds(GemvRowsLaunch L, const GemvPass &ps, hipStream_t st) {
    const int ntg = ps.t[1];
    for (int k = 0; k < 2; ++k) {
        const int nt = (int)ceil_div(L.p[k].rows > 0 ? L.p[k].rows : 1, 16);
        L.nrg[k] = (int)ceil_div(nt, ntg);
        L.tpg[k] = nt / L.nrg[k];
        L.trem[k] = nt % L.nrg[k];
        if (!L.p[k].nblocks) L.p[k].nspans = 0;
        EVC_REQUIRE(L.p[k].span_cols % kLW == 0, "gemv_rows_lds: span of %lld columns", (long long)L.p[k].span_cols);
        EVC_REQUIRE(!L.p[k].nblocks || (aligned16(L.p[k].A) && aligned16(L.p[k].v) && L.p[k].ld % 2 == 0 &&
                                        L.p[k].vstride % 2 == 0),
                    "gemv_rows_lds: operands must be 16-byte aligned with even pitches");
        EVC_REQUIRE(L.p[k].nspans <= 255 && L.nrg[k] <= 127, "gemv_rows_lds: %d spans x %d row groups", L.p[k].nspans,
                    L.nrg[k]);
    }
    const int nb0 = L.nrg[0] * L.p[0].nspans, nb1 = L.nrg[1] * L.p[1].nspans;
    EVC_REQUIRE(nb0 + nb1 > 0 && nb0 + nb1 <= 256, "gemv_rows_lds: %d blocks", nb0 + nb1);
    L.nblk0 = nb0;
    L.nblk1 = nb1;
    LdsBlockMap M;
    lds_block_map(L, nb1, nb0, M);
    const int nb = nb0 + nb1, gs = ps.t[0], g0 = ps.g0, G = ps.G;
#define EVC_LDS_12(NT_, NCH_) (gs == 2 ? lds_launch<2, NT_, NCH_>(L, M, nb, g0, G, st) : lds_launch<1, NT_, NCH_>(L, M, nb, g0, G, st))
    switch (ntg) {
        case 14: if (gs <= 2) return EVC_LDS_12(14, 1); break;
        case 7: return gs == 4 ? lds_launch<4, 7, 1>(L, M, nb, g0, G, st) : EVC_LDS_12(7, 2);
        case 4: return gs == 4 ? lds_launch<4, 4, 2>(L, M, nb, g0, G, st) : EVC_LDS_12(4, 3);
        case 2: return gs == 4 ? lds_launch<4, 2, 2>(L, M, nb, g0, G, st) : EVC_LDS_12(2, 4);
    }
#undef EVC_LDS_12
    set_error("gemv_rows_lds: no kernel <%d,%d,%d>", ps.t[0], ntg, ps.t[2]);
    return -1;
}

}  // namespace evc

#ifdef EVC_DEBUG_STAMPS
extern "C" int evc_debug_read_k5l(long long *stamps) {
    return (int)hipMemcpyFromSymbol(stamps, HIP_SYMBOL(evc::g_k5l_wg), sizeof(long long) * 1024 * 8);
}
#endif
