// K8 through LDS-DMA (lds_dma.hpp; batches of 17 .. 32 geometries per pass): gemv_cols_lds_kernel and, for tall matrices,
// gemv_cols_lds_slab_kernel.  (K5 through LDS-DMA: gemv_lds.hip; the plan that names these kernels: gemv_dispatch.hip.)
//   O[g][c] = sum_r w[g][r] A[r][c]      (reference: ab_initio_gradients_loewdin.py:343-356, the predicted RDMs as the
//   weighted sum of the stored transition RDMs)
// M <-> 16 geometries, N <-> 16 columns, K <-> 4 rows per MFMA.  A wave owns whole 16-column tiles (128 bytes = one cache
// line per row) and sums over ALL rows itself: no partial sums, no cross-wave reduction, no barrier after the weights
// are staged.  The matrix streams through a per-wave ring of D pieces (a piece = one LDS-DMA instruction = 8 rows x
// 128 bytes, in the order of the wave's tiles), D - 1 of them in flight; the weights of the whole launch sit in LDS as
// wl[row][32 geometries] (the two halves of a row swapped on odd rows: the two rows a 32-lane group reads fall on
// different banks).  Per piece: 2 + 4 ds_read_b64, 4 MFMAs (two K steps x two geometry sets), one refill.
// A tile's pieces are padded to an even number (weights of the padding rows are zero, its loads re-read the last row), so
// the loop body is two pieces with alternating fragment registers: the MFMAs of a piece run behind the fragment reads of
// the next one.
#include "common.hpp"
#include "kernels.hpp"
#include "lds_dma.hpp"

namespace evc {

template <int GS, int D, int NW>
__device__ __forceinline__ void cols_lds_body(const ColProblem &P, int g0, int G, int blk, int nblk, double *lds, int wave,
                                              int lane) {
    const int l15 = lane & 15, l4 = lane >> 4;
    const int rows = (int)P.rows;
    const int64_t cols = P.cols, ld = P.ld;
    const int NP = (rows + 7) >> 3;          // pieces per tile
    const int H = (NP + 1) >> 1;             // loop iterations per tile (two pieces each)
    const int NPe = 2 * H;
    const int rows_w = NPe * 8;              // weight rows in LDS (zero beyond the matrix)
    // ---- weights -> LDS (the only barrier of the kernel)
    for (int idx = threadIdx.x; idx < rows_w * 32; idx += 64 * NW) {
        const int r = idx >> 5, sl = idx & 31;
        double v = 0.0;
        if (r < rows && sl < G && sl < 16 * GS) {
            const int gg = g0 + sl;
            v = P.wt ? P.wt[(int64_t)(gg - gg % kMaxBatchG) * P.wstride + (int64_t)r * kMaxBatchG + gg % kMaxBatchG]
                     : P.w[(int64_t)gg * P.wstride + r];
        }
        lds[r * 32 + ((((sl >> 4) ^ (r & 1)) & 1) << 4) + (sl & 15)] = v;
    }
    __syncthreads();
    const int ntiles = (int)((cols + 15) >> 4);
    // tiles of this wave: (k nblk + blk) NW + wave, k = 0, 1, ... (the waves of a workgroup take adjacent tiles)
    const int tstride = nblk * NW;
    int ctile = blk * NW + wave;             // consumer's tile
    if (ctile >= ntiles) return;
    const unsigned ring = (unsigned)(rows_w * 256 + wave * D * 1024);   // LDS byte address of this wave's ring
    // producer lane constants: its 16 bytes of a piece
    const int prow = lane >> 3, ppos = lane & 7;
    const int last_valid = rows - 1 - 8 * (NP - 1);   // last valid row of the last piece, relative to it
    const unsigned voff = (unsigned)(((int64_t)prow * ld + 2 * ppos) * 8);
    const unsigned voff_last = (unsigned)(((int64_t)(prow < last_valid ? prow : last_valid) * ld + 2 * ppos) * 8);
    const unsigned voff_dummy = (unsigned)(2 * ppos * 8);
    const char *Ab = reinterpret_cast<const char *>(P.A);
    // producer cursor
    int ptile = ctile, ppiece = 0, pslot = 0;
    bool pdone = false;
    // one piece into ring slot pslot, cursor advanced: scalar work only (the vector pipe belongs to the FP64 MFMAs --
    // a vector instruction of this wave waits for them) and a short common path: a full piece of a tile that does not
    // hold the matrix's last columns; `psb` runs along the rows of the producer's tile
    const int64_t piece_step = 8 * ld * 8;
    const int tail_tile = (int)(ld >> 4) < ntiles && (((int64_t)(ld >> 4) * 16 + 16) > ld) ? (int)(ld >> 4) : -1;
    const char *psb = Ab + (int64_t)ptile * 128;
    int pfast = ptile == tail_tile ? 0 : NP - 1;   // pieces of the producer's tile that take the common path
#define EVC_COLS_PRODUCE()                                                                                       \
    {                                                                                                            \
        const unsigned la = uniform_u32(ring + (unsigned)pslot * 1024);                                          \
        if (ppiece < pfast) glds_s(voff, uniform_ptr(psb), la);                                                  \
        else {                                                                                                   \
            unsigned back = 0; /* the tile with the matrix's last columns: stay inside the row (ld is even) */   \
            if (ptile == tail_tile) {                                                                            \
                const int over = 2 * ppos - (int)(ld - 2 - (int64_t)ptile * 16);                                 \
                back = over > 0 ? (unsigned)(over * 8) : 0u;                                                     \
            }                                                                                                    \
            if (ppiece < NP - 1) glds_s(voff - back, uniform_ptr(psb), la);                                      \
            else if (ppiece == NP - 1) glds_s(voff_last - back, uniform_ptr(psb), la);                           \
            else glds_s(voff_dummy - back, uniform_ptr(Ab + ((int64_t)(rows - 1) * ld + (int64_t)ptile * 16) * 8), la); \
        }                                                                                                        \
        pslot = pslot + 1 == D ? 0 : pslot + 1;                                                                  \
        psb += piece_step;                                                                                       \
        if (++ppiece == NPe) {                                                                                   \
            ppiece = 0;                                                                                          \
            ptile += tstride;                                                                                    \
            psb = Ab + (int64_t)ptile * 128;                                                                     \
            pfast = ptile == tail_tile ? 0 : NP - 1;                                                             \
            if (ptile >= ntiles) pdone = true;                                                                   \
        }                                                                                                        \
    }
#pragma unroll 1
    for (int i = 0; i < D - 1; ++i) {
        if (!pdone) EVC_COLS_PRODUCE()
        else {   // (fewer pieces than ring slots: keep the in-order count with re-reads of the last row)
            const char *sb = Ab + (int64_t)(rows - 1) * ld * 8;
            glds_s(voff_dummy, uniform_ptr(sb), uniform_u32(ring + (unsigned)pslot * 1024));
            pslot = pslot + 1 == D ? 0 : pslot + 1;
        }
    }
    // consumer
    const unsigned xlane = (unsigned)(l4 * 128 + l15 * 8);                       // B fragment within a piece
    unsigned wl0[GS];                                                           // weight fragment of piece 0, K step 0
#pragma unroll
    for (int gs = 0; gs < GS; ++gs) wl0[gs] = (unsigned)(l4 * 256 + (((gs ^ (l4 & 1)) & 1) << 7) + l15 * 8);
    const char *ldsb = reinterpret_cast<const char *>(lds);
    int cslot = 0;
    d4 acc[GS];
    double xa[2], xb[2], wa[2][GS], wb[2][GS];
#define EVC_COLS_READ(X_, W_, PIECE_)                                                                         \
    {                                                                                                        \
        const char *xp = ldsb + ring + (unsigned)cslot * 1024 + xlane;                                       \
        X_[0] = *reinterpret_cast<const double *>(xp);                                                       \
        X_[1] = *reinterpret_cast<const double *>(xp + 512);                                                 \
        _Pragma("unroll") for (int gs = 0; gs < GS; ++gs) {                                                  \
            const char *wp = ldsb + (unsigned)(PIECE_) * 2048 + wl0[gs];                                     \
            W_[0][gs] = *reinterpret_cast<const double *>(wp);                                               \
            W_[1][gs] = *reinterpret_cast<const double *>(wp + 1024);                                        \
        }                                                                                                    \
        cslot = cslot + 1 == D ? 0 : cslot + 1;                                                              \
    }
#define EVC_COLS_MMA_K(X_, W_, K_)                                                                           \
    {                                                                                                        \
        _Pragma("unroll") for (int gs = 0; gs < GS; ++gs) acc[gs] = mfma_f64(W_[K_][gs], X_[K_], acc[gs]);     \
    }
#define EVC_COLS_MMA(X_, W_)                                                                                 \
    {                                                                                                        \
        EVC_COLS_MMA_K(X_, W_, 0)                                                                            \
        EVC_COLS_MMA_K(X_, W_, 1)                                                                            \
    }
// Position n of the wave's piece sequence: wait for piece n (D - 2 pieces are younger while the producer runs), read
// its fragments, start the MFMAs of piece n - 1, and refill the slot read at position n - 1 BETWEEN the two halves of
// those MFMAs: the scalar work of the refill and the LDS latency of piece n hide behind them.
#define EVC_COLS_STEP(X_, W_, PIECE_, XP_, WP_, MMA_)                                                        \
    {                                                                                                        \
        if (pdone) wait_vm<0>();                                                                             \
        else wait_vm<D - 2>();                                                                               \
        EVC_COLS_READ(X_, W_, PIECE_)                                                                        \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
        if (MMA_) EVC_COLS_MMA_K(XP_, WP_, 0)                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
        wait_lds();                                                                                          \
        if (!pdone) EVC_COLS_PRODUCE()                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
        if (MMA_) EVC_COLS_MMA_K(XP_, WP_, 1)                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
    }
    for (; ctile < ntiles; ctile += tstride) {
#pragma unroll
        for (int gs = 0; gs < GS; ++gs) acc[gs] = (d4){0.0, 0.0, 0.0, 0.0};
        for (int it = 0; it < H; ++it) {
            EVC_COLS_STEP(xa, wa, 2 * it, xb, wb, it > 0)
            EVC_COLS_STEP(xb, wb, 2 * it + 1, xa, wa, true)
        }
        EVC_COLS_MMA(xb, wb)
        // D[i][j]: i = geometry l4 + 4 reg, j = column l15
        const int64_t c = (int64_t)ctile * 16 + l15;
        if (c < cols) {
#pragma unroll
            for (int gs = 0; gs < GS; ++gs)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int g = 16 * gs + l4 + 4 * r;
                    if (g < G) P.out[(int64_t)(g0 + g) * P.ostride + c] = acc[gs][r];
                }
        }
    }
#undef EVC_COLS_READ
#undef EVC_COLS_MMA
#undef EVC_COLS_MMA_K
#undef EVC_COLS_STEP
#undef EVC_COLS_PRODUCE
    wait_vm<0>();
}

// Tall matrices (large training sets: more rows than weights fit in LDS): the rows go in SLABS of kSlabRows; a wave owns
// NTW ADJACENT column tiles (one workgroup round), keeps their accumulators and walks slab by slab, piece by piece, tile by
// tile -- so it still sums over all rows itself (no partial sums), a piece's weights are read once for all its tiles, and
// a workgroup's eight waves read 8 NTW x 128 contiguous bytes of every row within a few steps (DRAM pages are reused:
// tile-by-tile order, each 128-byte piece of a row on its own, streamed a cold 3.4 GB matrix at 4.4 TB/s).
// The weights of slab s + 1 are fetched by LDS-DMA from the transposed copy `wt` (rows x 32, contiguous) into the second
// weight buffer while slab s is in work: each wave issues its share at the start of slab s, and the constant vmcnt
// waits of the piece stream retire them long before the slab ends, so the slab boundary is ONE LDS-only barrier and the
// ring never drains.  (The one-body problem has no transposed weights: its few workgroups stage a slab with plain
// loads between two barriers.)  Waves at the end of the matrix run their missing tiles on the last tile (not stored).
constexpr int kSlabRows = 160;          // 20 pieces; two weight buffers of 40 KB + eight rings of 10 KB = 160 KB
constexpr int kSlabRing = 10;
template <int GS, int NTW>
__device__ __forceinline__ void cols_lds_slab_body(const ColProblem &P, int g0, int G, int blk, int nblk, double *lds,
                                                   int wave, int lane) {
    constexpr int NW = 8, D = kSlabRing;
    constexpr unsigned WB = kSlabRows * 256;   // bytes of one weight buffer
    const int l15 = lane & 15, l4 = lane >> 4;
    const int rows = (int)P.rows;
    const int64_t cols = P.cols, ld = P.ld;
    const int nslab = (rows + kSlabRows - 1) / kSlabRows;
    const int ntiles = (int)((cols + 15) >> 4);
    const bool dma_w = P.wt != nullptr;        // workgroup-uniform
    const int tile0 = (blk * NW + wave) * NTW; // this wave's tiles: tile0 .. tile0 + NTW - 1
    const bool active = tile0 < ntiles;
    // pieces of slab s (even: the weights of the padding rows are zero, its loads re-read the matrix's last row)
    auto slab_pieces = [&](int sidx) {
        const int left = rows - sidx * kSlabRows;
        const int np = ((left < kSlabRows ? left : kSlabRows) + 7) >> 3;
        return (np + 1) & ~1;
    };
    const unsigned ring = 2 * WB + (unsigned)(wave * D * 1024);   // LDS byte address of this wave's ring
    const int prow = lane >> 3, ppos = lane & 7;
    const char *Ab = reinterpret_cast<const char *>(P.A);
    const int tail_tile = (int)(ld >> 4) < ntiles && (((int64_t)(ld >> 4) * 16 + 16) > ld) ? (int)(ld >> 4) : -1;
    const unsigned voff_full = (unsigned)(((int64_t)prow * ld + 2 * ppos) * 8);
    // weights of slab `sidx` into buffer `buf` by LDS-DMA: instruction k covers rows 4k .. 4k+3 of the slab (1 KB, lane i ->
    // row 4k + (i >> 4), 16-byte piece i & 15); the piece holds geometries 16 (h ^ (row & 1)) + 2 (i & 7), + 1 with
    // h = (i >> 3) & 1: the halves of odd rows swapped (the image the fragment reads expect).  Rows beyond the matrix
    // fetch its last row and are zeroed once the buffer is complete.
    const double *wtb = dma_w ? P.wt + (int64_t)(g0 - g0 % kMaxBatchG) * P.wstride + g0 % kMaxBatchG : nullptr;
    auto issue_weights = [&](int sidx, int buf) {
        const int r00 = sidx * kSlabRows;
        for (int k = wave; k < kSlabRows / 4; k += NW) {
            const int rl = 4 * k + (lane >> 4), r = r00 + rl;
            const int rc = r < rows ? r : rows - 1;
            const int h = (lane >> 3) & 1;
            const double *src = wtb + (int64_t)rc * kMaxBatchG + 16 * (h ^ (rl & 1)) + 2 * (lane & 7);
            glds_v(src, uniform_u32((unsigned)buf * WB + (unsigned)k * 1024));
        }
    };
    // producer cursor: slab, piece, tile (the order the consumer reads in)
    int pslab = 0, pj = 0, ppiece = 0, pslot = 0, pnp = slab_pieces(0);
    bool pdone = !active;
#define EVC_SLAB_PRODUCE()                                                                                       \
    {                                                                                                            \
        const int pt_ = tile0 + pj;                                                                              \
        const int ptile = pt_ < ntiles ? pt_ : ntiles - 1;          /* (a tile the wave does not have) */        \
        const int r0 = pslab * kSlabRows + 8 * ppiece;              /* first row of the piece */                 \
        const int rf = r0 < rows ? r0 : rows - 1;                   /* (padding piece: the last row) */          \
        const int lastv = rows - 1 - rf;                            /* last valid row relative to rf */          \
        unsigned vo = voff_full;                                    /* (common path: no vector arithmetic) */    \
        if (lastv < 7 || ptile == tail_tile) {                                                                   \
            const int rr = prow < lastv ? prow : lastv;                                                          \
            vo = (unsigned)(((int64_t)rr * ld + 2 * ppos) * 8);                                                  \
            if (ptile == tail_tile) { /* stay inside the row (ld is even) */                                     \
                const int over = 2 * ppos - (int)(ld - 2 - (int64_t)ptile * 16);                                 \
                if (over > 0) vo -= (unsigned)(over * 8);                                                        \
            }                                                                                                    \
        }                                                                                                        \
        glds_s(vo, uniform_ptr(Ab + ((int64_t)rf * ld + (int64_t)ptile * 16) * 8),                               \
               uniform_u32(ring + (unsigned)pslot * 1024));                                                      \
        pslot = pslot + 1 == D ? 0 : pslot + 1;                                                                  \
        if (++pj == NTW) {                                                                                       \
            pj = 0;                                                                                              \
            if (++ppiece == pnp) {                                                                               \
                ppiece = 0;                                                                                      \
                if (++pslab == nslab) pdone = true;                                                              \
                else pnp = slab_pieces(pslab);                                                                   \
            }                                                                                                    \
        }                                                                                                        \
    }
    if (dma_w) issue_weights(0, 0);
#pragma unroll 1
    for (int i = 0; i < D - 1; ++i) {
        if (!pdone) EVC_SLAB_PRODUCE()
        else {   // (fewer pieces than ring slots: keep the in-order count with re-reads of the last row)
            glds_s((unsigned)(2 * ppos * 8), uniform_ptr(Ab + (int64_t)(rows - 1) * ld * 8),
                   uniform_u32(ring + (unsigned)pslot * 1024));
            pslot = pslot + 1 == D ? 0 : pslot + 1;
        }
    }
    const unsigned xlane = (unsigned)(l4 * 128 + l15 * 8);
    unsigned wl0[GS];
#pragma unroll
    for (int gs = 0; gs < GS; ++gs) wl0[gs] = (unsigned)(l4 * 256 + (((gs ^ (l4 & 1)) & 1) << 7) + l15 * 8);
    const char *ldsb = reinterpret_cast<const char *>(lds);
    int cslot = 0;
    d4 acc[NTW][GS];
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
        for (int gs = 0; gs < GS; ++gs) acc[j][gs] = (d4){0.0, 0.0, 0.0, 0.0};
    double x[2][NTW][2];   // [piece parity][tile][K step]
    double wf[2][2][GS];   // [piece parity][K step][geometry set]
// position (piece parity Q_, tile J_): wait for its piece, read the matrix fragments (and, at the first tile, the piece's
// weights), first half of the MFMAs of the position before (PQ_, PJ_), refill, second half
#define EVC_SLAB_STEP(Q_, J_, PIECE_, PQ_, PJ_, MMA_)                                                        \
    {                                                                                                        \
        if (pdone) wait_vm<0>();                                                                             \
        else wait_vm<D - 2>();                                                                               \
        {                                                                                                    \
            const char *xp = ldsb + ring + (unsigned)cslot * 1024 + xlane;                                   \
            x[Q_][J_][0] = *reinterpret_cast<const double *>(xp);                                            \
            x[Q_][J_][1] = *reinterpret_cast<const double *>(xp + 512);                                      \
            if ((J_) == 0) {                                                                                 \
                _Pragma("unroll") for (int gs = 0; gs < GS; ++gs) {                                          \
                    const char *wp = ldsb + wbuf + (unsigned)(PIECE_) * 2048 + wl0[gs];                      \
                    wf[Q_][0][gs] = *reinterpret_cast<const double *>(wp);                                   \
                    wf[Q_][1][gs] = *reinterpret_cast<const double *>(wp + 1024);                            \
                }                                                                                            \
            }                                                                                                \
            cslot = cslot + 1 == D ? 0 : cslot + 1;                                                          \
        }                                                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
        if (MMA_) {                                                                                          \
            _Pragma("unroll") for (int gs = 0; gs < GS; ++gs)                                                \
                acc[PJ_][gs] = mfma_f64(wf[PQ_][0][gs], x[PQ_][PJ_][0], acc[PJ_][gs]);                         \
        }                                                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
        wait_lds();                                                                                          \
        if (!pdone) EVC_SLAB_PRODUCE()                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
        if (MMA_) {                                                                                          \
            _Pragma("unroll") for (int gs = 0; gs < GS; ++gs)                                                \
                acc[PJ_][gs] = mfma_f64(wf[PQ_][1][gs], x[PQ_][PJ_][1], acc[PJ_][gs]);                         \
        }                                                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
    }
    for (int sidx = 0; sidx < nslab; ++sidx) {
        const unsigned wbuf = dma_w ? (unsigned)(sidx & 1) * WB : 0u;
        const int r00 = sidx * kSlabRows;
        if (dma_w) {
            // every DMA of this slab's weights (issued a slab ago, or in the prologue) has been retired by the piece
            // waits since; a wave that had no pieces to wait for waits here
            if (sidx == 0 || !active || pdone) wait_vm<0>();
            lds_barrier();   // ... by EVERY wave: the buffer is complete; and nobody reads the other buffer any more
            // rows of the slab beyond the matrix: zero weights (they were fetched from the last row)
            if (r00 + kSlabRows > rows) {
                const int first = rows > r00 ? rows - r00 : 0;
                for (int idx = threadIdx.x; idx < (kSlabRows - first) * 32; idx += 64 * NW)
                    lds[wbuf / 8 + (first + (idx >> 5)) * 32 + (idx & 31)] = 0.0;
                lds_barrier();
            }
            if (sidx + 1 < nslab) issue_weights(sidx + 1, (sidx + 1) & 1);
        } else {
            __syncthreads();   // every wave has read the last weights of the slab before
            for (int idx = threadIdx.x; idx < kSlabRows * 32; idx += 64 * NW) {
                const int rl = idx >> 5, sl = idx & 31, r = r00 + rl;
                double v = 0.0;
                if (r < rows && sl < G && sl < 16 * GS) v = P.w[(int64_t)(g0 + sl) * P.wstride + r];
                lds[rl * 32 + ((((sl >> 4) ^ (rl & 1)) & 1) << 4) + (sl & 15)] = v;
            }
            __syncthreads();
        }
        if (active) {
            const int H = slab_pieces(sidx) >> 1;
            for (int it = 0; it < H; ++it) {
#pragma unroll
                for (int j = 0; j < NTW; ++j) {   // piece 2 it; the position before: (piece 2 it - 1, last tile) or (this, j - 1)
                    if (j == 0) EVC_SLAB_STEP(0, 0, 2 * it, 1, NTW - 1, it > 0)
                    else EVC_SLAB_STEP(0, j, 2 * it, 0, (j > 0 ? j - 1 : 0), true)
                }
#pragma unroll
                for (int j = 0; j < NTW; ++j) {   // piece 2 it + 1
                    if (j == 0) EVC_SLAB_STEP(1, 0, 2 * it + 1, 0, NTW - 1, true)
                    else EVC_SLAB_STEP(1, j, 2 * it + 1, 1, (j > 0 ? j - 1 : 0), true)
                }
            }
            // the last position of the slab (its fragments are in registers: the next slab's weights do not matter)
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int gs = 0; gs < GS; ++gs)
                    acc[NTW - 1][gs] = mfma_f64(wf[1][k][gs], x[1][NTW - 1][k], acc[NTW - 1][gs]);
        }
    }
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const int64_t c = (int64_t)(tile0 + j) * 16 + l15;
        if (active && tile0 + j < ntiles && c < cols) {
#pragma unroll
            for (int gs = 0; gs < GS; ++gs)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int g = 16 * gs + l4 + 4 * r;
                    if (g < G) P.out[(int64_t)(g0 + g) * P.ostride + c] = acc[j][gs][r];
                }
        }
    }
#undef EVC_SLAB_STEP
#undef EVC_SLAB_PRODUCE
    wait_vm<0>();
}

template <int GS, int NTW>
__global__ __launch_bounds__(512, 1) void gemv_cols_lds_slab_kernel(GemvColsLaunch L, int nblk1, int g0, int G) {
    extern __shared__ __align__(16) double lds_cols_slab[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    // the few blocks of the small second problem are dispatched first
    if ((int)blockIdx.x < nblk1) cols_lds_slab_body<GS, 1>(L.p[1], g0, G, blockIdx.x, nblk1, lds_cols_slab, wave, lane);
    else cols_lds_slab_body<GS, NTW>(L.p[0], g0, G, blockIdx.x - nblk1, gridDim.x - nblk1, lds_cols_slab, wave, lane);
}

template <int GS, int D0, int D1, int NW>
__global__ __launch_bounds__(64 * NW, 1) void gemv_cols_lds_kernel(GemvColsLaunch L, int nblk1, int g0, int G) {
    extern __shared__ __align__(16) double lds_cols[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    // the few blocks of the small second problem are dispatched first
    if ((int)blockIdx.x < nblk1) cols_lds_body<GS, D1, NW>(L.p[1], g0, G, blockIdx.x, nblk1, lds_cols, wave, lane);
    else cols_lds_body<GS, D0, NW>(L.p[0], g0, G, blockIdx.x - nblk1, gridDim.x - nblk1, lds_cols, wave, lane);
}

// (host side: one workgroup per CU and grids sized for a whole MI355X, as for K5 -- see the host side of gemv_lds.hip)
template <int GS, int D0, int D1, int NW>
static int cols_lds_launch(const GemvColsLaunch &L, int nblk1, int nblk0, size_t lds, int g0, int G, hipStream_t st) {
    static LdsAttr attr;
    if (int rc = allow_dynamic_lds(gemv_cols_lds_kernel<GS, D0, D1, NW>, attr, 160 * 1024, "gemv_cols_lds")) return rc;
    hipLaunchKernelGGL((gemv_cols_lds_kernel<GS, D0, D1, NW>), dim3(nblk0 + nblk1), dim3(64 * NW), lds, st, L, nblk1, g0, G);
    EVC_LAUNCH_CHECK("gemv_cols_lds");
    return 0;
}

// <2, 12, D1, 8> = ps.t: two geometry sets (one set stays with the row-split kernel); ring depths of the two problems
// (the weights, rows x 32, and the rings fit the LDS); eight waves per workgroup (two per SIMD: with one wave per SIMD
// and rings of 24 the loop was bound by its own scalar instructions, 54 us against 43 at H30; removed).
// (Both LDS-staged K8 kernels need A 16-byte aligned with an even pitch: every caller has checked that -- check_set of
// workspace.hip for the calls on a training set, the roots calls among them, and evc_gemv_cols.)
int launch_cols_lds(GemvColsLaunch L, const GemvPass &ps, hipStream_t st) {
    const int d1 = ps.t[2], nw = 8;
    const int nblk1 = L.p[1].cols > 0 ? kLdsBlocksSmall : 0;
    // workgroups of the large problem: every wave the same number of 16-column tiles (rounds), in one round of blocks
    const int64_t ntiles = ceil_div(L.p[0].cols, 16);
    const int64_t rounds = ceil_div(ntiles, (int64_t)nw * kLdsBlocks);
    const int nblk0 = (int)ceil_div(ntiles, nw * rounds);
    auto need = [&](const ColProblem &P, int d) { return (size_t)(((P.rows + 15) / 16) * 16 * 256 + (int64_t)nw * d * 1024); };
    size_t lds = need(L.p[0], 12);
    if (L.p[1].cols > 0 && need(L.p[1], d1) > lds) lds = need(L.p[1], d1);
    return d1 == 12 ? cols_lds_launch<2, 12, 12, 8>(L, nblk1, nblk0, lds, ps.g0, ps.G, st)
                    : cols_lds_launch<2, 12, 6, 8>(L, nblk1, nblk0, lds, ps.g0, ps.G, st);
}

template <int NTW>
static int cols_lds_slab_launch(const GemvColsLaunch &L, int nblk1, int nblk0, int g0, int G, hipStream_t st) {
    const size_t lds = (size_t)2 * kSlabRows * 256 + (size_t)8 * kSlabRing * 1024;
    static LdsAttr attr;
    if (int rc = allow_dynamic_lds(gemv_cols_lds_slab_kernel<2, NTW>, attr, 160 * 1024, "gemv_cols_lds_slab")) return rc;
    hipLaunchKernelGGL((gemv_cols_lds_slab_kernel<2, NTW>), dim3(nblk0 + nblk1), dim3(512), lds, st, L, nblk1, g0, G);
    EVC_LAUNCH_CHECK("gemv_cols_lds_slab");
    return 0;
}

// <2, NTW> = ps.t: every wave's NTW tiles in one round of workgroups
int launch_cols_lds_slab(GemvColsLaunch L, const GemvPass &ps, hipStream_t st) {
    const int nblk0 = (int)ceil_div(ceil_div(L.p[0].cols, 16), 8 * ps.t[1]);
    const int nblk1 = L.p[1].cols > 0 ? (int)ceil_div(ceil_div(L.p[1].cols, 16), 8) : 0;
    switch (ps.t[1]) {
        case 1: return cols_lds_slab_launch<1>(L, nblk1, nblk0, ps.g0, ps.G, st);
        case 2: return cols_lds_slab_launch<2>(L, nblk1, nblk0, ps.g0, ps.G, st);
        case 3: return cols_lds_slab_launch<3>(L, nblk1, nblk0, ps.g0, ps.G, st);
        case 4: return cols_lds_slab_launch<4>(L, nblk1, nblk0, ps.g0, ps.G, st);
    }
    set_error("gemv_cols_lds_slab: no kernel <2,%d>", ps.t[1]);
    return -1;
}

}  // namespace evc
