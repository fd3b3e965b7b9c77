// The fully symmetric pair step of the compressed layout's pipeline (dense (pair, pair) operand in, dense (pair, pair)
// result out; electron_integral_utils.py:136 / ab_initio_gradients_loewdin.py:224-232 as two-sided rotations
// N_e = X^T M_e X of the n(n+1)/2 symmetric matrices M_e), 16 < n <= 30, with NO vector instruction beside the MFMAs
// in its steady state.
//
// Why (round 4): an FP64 MFMA and every other vector instruction share one pipe on gfx950 (profiles/
// mfma_f64_coissue.txt): pt_pipe_kernel (pair_pipe.hip) issued ~250 vector instructions per matrix -- address
// arithmetic, predicates, selects, multiplicities -- beside its 56 MFMAs and kept the matrix pipe 49 % busy.  Loads,
// stores, LDS and scalar instructions DO issue while an MFMA executes.  Here everything per matrix is one of those:
//   * the operand row (one packed symmetric matrix, n(n+1)/2 doubles) comes by LDS-DMA (glds_s of lds_dma.hpp:
//     scalar row base + four lane-constant offsets) into the wave's LDS row; the fragments are read from it at sixteen
//     lane-constant addresses; the wait for the DMA is a counted vmcnt (the stores issued behind it are counted per
//     wave on the host side of the loop, all conditions wave-uniform);
//   * the stage is slot-major, [buffer][slot][row u] with a slot pitch of 32 bytes mod 128: the 12 stage writes of a
//     matrix are conflict free at lane-constant addresses, buffer and slot are IMMEDIATE offsets (the loop is unrolled
//     over the four (matrix parity, tile parity) phases), the write-out reads its two columns with two ds_read_b64,
//     conflict free as well;
//   * the write-out store is `scalar base + lane-constant offset`; rows are written in whole 16-row groups per wave
//     (the result buffer has pair_ld(n) rows), columns in whole tiles of 8 (its pitch is pair_ld(n)): no predicates;
//   * multiplicities are left to the consumers (the HBM-bound int2e_ip1 dot weighs its operand itself).
// The pipeline around these pieces is pt_pipe_kernel's: one matrix per iteration, result i-1 staged during the H phase
// of matrix i, one barrier per tile of eight leading pairs, tile j written out during the N phases of the two
// iterations behind its barrier, two workgroups per CU.
#include "pair_dma.hpp"

namespace evc {

// arguments of y2d_kernel: the Y2 contraction alone, or what it adds to the first gradient-side pair step
struct Y2dArgs {
    const double *SB, *M1, *X;   // rows v of SB and of the first pair step's intermediate, pitch pair_ld(n); X (n, n)
    double *partial;             // [slab][n][n] per geometry
    int64_t sX, sws;
    int n, tiles_per_wg, ppt;
};

// MODE 0: dense (pair, pair) result out[tri(r',s')][tri(p,q)], pitch out_ld.
// MODE 1: the 8-fold compressed packed vector packed[tri(u, v)], u = tri(r',s') >= v = tri(p,q), times the
//         multiplicities of both pairs (and diag_mult on u == v): the write-out walks the rows u = ur + 64 k from 0 with
//         lane-constant offsets tri(u) and skips the passes above the diagonal (k < v / 64, wave-uniform); the pass that
//         holds the diagonal takes a slower, predicated body, once per tile (store_pass).
//
// Y2 (MODE 0, the first gradient-side step, ct = 1): the H = M_e X this step forms is T_e X^T of the Y2 contraction
//   Y2 = sum_e mult(e) T_e X^T M1_e   (ab_initio_gradients_loewdin.py:210-232),
// so a third phase per matrix adds (mult(e) / 2) H M1_e to one accumulator set (a wave-uniform branch on the scalar
// (p, q) of the pair takes the diagonal pairs apart) -- 32 MFMAs instead of the 64 of a kernel of its own, and SB is
// read once.  H leaves the MFMAs as an accumulator (rows on registers and lane groups), which serves X^T H as its
// B operand; H M1_e wants it as the A operand (rows on lanes): the wave writes it into its LDS square during the first
// N-phase steps and reads the fragments back during the last ones, all at lane-constant addresses.  The M1 row comes
// by LDS-DMA into a second row of the wave: fragments read during the Y phase, the next row requested behind them.
//
// DOT (MODE 0, the second gradient-side step): the result R_e = row e = tri(hi, lo) of the AO-basis 2-RDM is not written
// but contracted where it stands in the stage, as the pair blocks of ip1_dh_kernel (ip1.hip) contract it:
//   t2part[(hi 3 + x) nchunk + lo] = sum_f w(f) R_e[f] ip1[x][hi][lo][f],   and for hi != lo with hi <-> lo,
// w(f) = 1 on the diagonal pairs f = tri(c, c), else 2.  The write-out has its own thread map here: thread t takes ONE
// pair of the tile (slot t / 32) and the rows f = 64 k + 2 u, + 1 (u = t % 32) of pass k -- one 16-byte LDS read of the
// stage, and six 16-byte loads of int2e_ip1 (two orders of the pair x three components) that run along f across the
// lanes, 512 contiguous bytes per row and wave as in ip1_dh_kernel (8-byte loads of two pairs per thread, in the map of
// the storing write-out, touch four rows per quad of lanes: 113 us per launch however many were in flight).  The
// addresses do not depend on the step's result, so the elements are requested one iteration ahead: the four passes of
// a phase have a register set each, and behind pass k that set is reloaded with pass k + 4 (odd iterations: pass k - 4
// of the next tile) -- 24 loads of 16 bytes per lane in flight, 98 KB per CU, through an H phase and more.  That costs
// 96 VGPRs: ONE workgroup per CU (the launch is bound by the int2e_ip1 stream, not by the MFMAs), tiles per workgroup as
// for the Y2 pair step.  Behind pass 7 of a tile each wave adds the six sums of its two pairs over its lanes (DPP and one
// shuffle) into LDS behind the stage (one buffer per tile parity); the first 48 threads write the tile's 48 entries
// behind the next barrier.
template <int MODE, bool Y2, bool DOT = false>
__device__ __forceinline__ void ptd_body(const PairTransformArgs &a, const Y2dArgs &y, const PairDotArgs &dt = PairDotArgs{}) {
    constexpr int KS = 8, NT = 2;
    constexpr unsigned kPdStage = Y2 ? kPdStageY : evc::kPdStage;   // (shadows the namespace constant)
    static_assert(!Y2 || MODE == 0, "the Y2 phase belongs to the dense step");
    static_assert(!DOT || (MODE == 0 && !Y2), "the int2e_ip1 dot belongs to the dense step alone");
    extern __shared__ __align__(16) char lds[];   // the only LDS of this kernel: it starts at LDS address 0
    const int n = a.n;
    const int npairs = n * (n + 1) / 2;
    const int in_ld = a.in_ld ? a.in_ld : npairs, out_ld = a.out_ld;   // (0: the caller's s4 matrix, pitch n(n+1)/2)
    const int64_t g = blockIdx.y;
    const double *__restrict__ in = a.in + g * a.sin;
    const double *__restrict__ C = a.C + g * a.sC;
    const int ntiles = (npairs + 7) / 8;
    const int t_begin = blockIdx.x * a.tiles_per_wg, t_end = min(ntiles, t_begin + a.tiles_per_wg);
    if (t_begin >= t_end) {
        if constexpr (Y2) {   // (every workgroup writes its slab)
            double *dst = y.partial + g * y.sws + (int64_t)blockIdx.x * n * n;
            for (int idx = threadIdx.x; idx < n * n; idx += 256) dst[idx] = 0.0;
        }
        return;
    }
    const int niter = 2 * (t_end - t_begin);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;

    // this wave's leading pair of iteration i: e0 + 4 i.  The DMA reads 16-byte aligned granules: the window of a row
    // starts dw doubles in front of it (dw = 1 when the row starts on an odd multiple of 8 bytes); rows 4 apart -- and
    // the row idle slots fall back to, row `wave` -- have the same dw whatever the pitch
    const int e0 = 8 * t_begin + wave;
    const int dw = (int)(((reinterpret_cast<uintptr_t>(in) >> 3) + (uintptr_t)((int64_t)e0 * in_ld)) & 1);
    const unsigned rowb = (unsigned)wave * kPdRB;
    unsigned fa[NT][KS];   // LDS address of fragment (rt, kk) of the symmetric matrix in the wave's row
#pragma unroll
    for (int rt = 0; rt < NT; ++rt)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const int r = rt * 16 + l15, s = 4 * kk + l4;
            const int hi = s > r ? s : r, lo = s > r ? r : s;
            fa[rt][kk] = (r < n && s < n) ? rowb + 8u * (unsigned)(dw + hi * (hi + 1) / 2 + lo) : rowb + kPdRaw * 1024;
        }
    if (lane < 8) *reinterpret_cast<double *>(lds + rowb + kPdRaw * 1024 + 8 * lane) = 0.0;
    const RowDma dma((unsigned)(((npairs + dw) * 8 + 15) & ~15), lane);   // (the bytes of the window)
    const int npieces = dma.npieces;
    auto dma_row = [&](int e) {
        const int ec = e < npairs ? e : wave;
        dma.request(reinterpret_cast<const char *>(in + (int64_t)ec * in_ld) - 8 * dw, rowb);
    };
    dma_row(e0);
    // Y2: the M1 row of the same pair (rows on 16-byte granules: the launch checks it, the window is the SB row's)
    [[maybe_unused]] const double *__restrict__ M1 = Y2 ? y.M1 + g * y.sws : nullptr;
    constexpr unsigned kRowM = 4 * kPdRB;   // the wave's M1 row: this far behind its SB row
    [[maybe_unused]] auto dma_mrow = [&](int e) {
        const int ec = e < npairs ? e : wave;
        dma.request(reinterpret_cast<const char *>(M1 + (int64_t)ec * in_ld), rowb + kRowM);
    };
    if constexpr (Y2) {
        if (lane < 8) *reinterpret_cast<double *>(lds + rowb + kRowM + kPdRaw * 1024 + 8 * lane) = 0.0;
        dma_mrow(e0);
    }

    // the X fragments straight from global memory (16 rows of 128 bytes per load instruction)
    double xf[KS][NT];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int d = 4 * kk + l4, c = t * 16 + l15;
            const bool ok = d < n && c < n;
            const double *src = C + (ok ? (a.ct ? c * n + d : d * n + c) : 0);
            const double v = *src;
            xf[kk][t] = ok ? v : 0.0;
        }

    // stage address of result register f = tile * 4 + reg (tiles (0,0), (1,0), (1,1)) for slot `wave` of buffer 0;
    // registers that hold no result go to the 16 dump doubles behind the column's rows
    unsigned sa[2][12];   // [buffer]: (an immediate offset beyond 32 KB makes the compiler emit `v_add_u32 v, 0, v` per write)
#pragma unroll
    for (int f = 0; f < 12; ++f) {
        const int tile = f / 4, reg = f % 4;
        const int it = tile == 0 ? 0 : 1, st = tile == 2 ? 1 : 0;
        const int r2 = it * 16 + l4 + 4 * reg, s2 = st * 16 + l15;
        const bool ok = r2 < n && s2 <= r2;
        sa[0][f] = opaque(kPdStage + (unsigned)wave * kPdP + 8u * (unsigned)(ok ? r2 * (r2 + 1) / 2 + s2 : npairs + l15));
        sa[1][f] = opaque(sa[0][f] + 8u * kPdP);
    }
    // write-out: thread (wl, ur) takes the columns wl, wl + 1 (wl even) of the rows ur + 64 k; a wave writes whole
    // groups of 16 rows (the result buffer has pair_ld(n) rows): pass k of this wave is valid <=> 64 k + 16 wave < npairs
    const int wl = 2 * (threadIdx.x & 3), ur = threadIdx.x >> 2;
    const unsigned wo = opaque(kPdStage + (unsigned)wl * kPdP + 8u * (unsigned)ur);
    const unsigned gvo = (unsigned)((ur * out_ld + wl) * 8);
    char *outg = reinterpret_cast<char *>(MODE == 0 ? a.out + g * a.sout : a.packed + g * a.spacked);
    [[maybe_unused]] unsigned tv[8];     // MODE 1: byte offset of (row ur + 64 k, column wl) in the packed vector
    [[maybe_unused]] double frow[8];     // MODE 1: multiplicity of row ur + 64 k
    if constexpr (MODE == 1) {
        // table of pair multiplicities (the diagonal pairs u = tri(i,i) = i (i + 3) / 2 are 1, the others 2)
        for (int u = threadIdx.x; u < 512; u += 256) {
            const int r = tri_row_small(u);
            *(lds_f32 *)(uintptr_t)(kPdTab + 4u * (unsigned)u) = (u == r * (r + 3) / 2) ? 1.0f : 2.0f;
        }
        if (blockIdx.x == 0)   // zero the padding [M, packed_len) once per geometry
            zero_packed_tail(a.packed + g * a.spacked, (int64_t)npairs * (npairs + 1) / 2, a.packed_len);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int u = ur + 64 * k;
            tv[k] = (unsigned)((u * (u + 1) / 2 + wl) * 8);
            frow[k] = (double)*(lds_f32 *)(uintptr_t)(kPdTab + 4u * (unsigned)(u & 511));
        }
    }
    const int wrows = DOT ? npairs : npairs - 16 * wave;   // pass k valid <=> 64 k < wrows (DOT: every wave takes all 64 rows)
    int vmask = 0;   // bit k: this wave writes pass k
#pragma unroll
    for (int k = 0; k < 8; ++k) vmask |= (64 * k < wrows) ? 1 << k : 0;
    vmask = __builtin_amdgcn_readfirstlane(vmask);
    int cntA = 0, cntB = 0;
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        cntA += (64 * c < wrows) ? 1 : 0;
        cntB += (64 * (4 + c) < wrows) ? 1 : 0;
    }
    // THE COUNTED WAIT for the operand row of matrix i + 1, requested in the last N phase: what the wave issued behind that
    // request may stay in flight.  Dense store: the stores of that phase's passes c = 1..3 (none before iteration 2).
    // Packed store: they vary from tile to tile -- vmcnt(0), they are a phase old by then.  DOT: its int2e_ip1 loads are
    // buffer loads the compiler counts -- vmcnt(0).  (Y2 adds the DMA of its M1 row: y2_wait_sb_row.)
    auto younger = [&](bool odd, int i) { return (MODE == 0 && !DOT && i >= 3) ? (odd ? cntA : cntB) : 0; };
    // The storing write-outs: pass k of the tile at `ob` from the thread's stage values dv.  Packed: kd is the pass that
    // holds the diagonal u == v of this tile's columns, cf the multiplicities of the thread's two columns.
    [[maybe_unused]] auto store_pass = [&](int k, d2 dv, char *ob, int kd, d2 cf, int jt) {
        if constexpr (MODE == 0) {
            gstore16(gvo, dv, ob + (int64_t)(64 * k) * out_ld * 8);
        } else {
            const int u = ur + 64 * k;
            d2 f = cf * frow[k];
            if (k != kd) {          // below the diagonal: both columns, rows beyond the last one masked
                const d2 v = dv * f;
                if (u < npairs) gstore16(tv[k], v, ob);
            } else {                // the diagonal pass: column v of row u only for u >= v, diag_mult on u == v
                const int d = u - (8 * (t_begin + jt) + wl);
                if (d == 0) f[0] *= a.diag_mult;
                if (d == 1) f[1] *= a.diag_mult;
                const d2 v = dv * f;
                if (u < npairs) {
                    if (d >= 1) *reinterpret_cast<d2 *>(ob + tv[k]) = v;
                    else if (d == 0) *reinterpret_cast<double *>(ob + tv[k]) = v[0];
                }
            }
        }
    };
    // DOT: the thread's pair of the tile and its row pair; of the rows 64 k + 2 du, + 1 a bit each for "diagonal pair"
    // (weight 1, else 2; bits k, 8 + k) and for "a row of the result" (bits 16 + k, 24 + k); the int2e_ip1 blocks of the
    // three components; the offsets bo of the rows (hi, lo), (lo, hi) of the tile being loaded; the sums; the register
    // sets of the four passes of a phase
    [[maybe_unused]] const int dslot = threadIdx.x >> 5, du = threadIdx.x & 31;
    [[maybe_unused]] const unsigned wod = DOT ? opaque(kPdStage + (unsigned)dslot * kPdP + 16u * (unsigned)du) : 0u, du16 = 16u * (unsigned)du;
    [[maybe_unused]] double acc[6];
    [[maybe_unused]] d2 qb[4][6];
    [[maybe_unused]] unsigned wm = 0, bo[2] = {0, 0};
    // (buffer loads: a 32-bit lane offset, the component's block as the scalar offset; counted by the compiler)
    [[maybe_unused]] __amdgpu_buffer_rsrc_t iprs;
    [[maybe_unused]] unsigned ipx[3] = {0, 0, 0};
    if constexpr (DOT) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int f = 64 * k + 2 * du + h, fc = f < npairs ? f : 0, r = tri_row_small(fc);
                wm |= (f < npairs ? 0x10000u << (8 * h + k) : 0u) | (fc == r * (r + 3) / 2 ? 1u << (8 * h + k) : 0u);
            }
        const unsigned xb = 8u * (unsigned)(n * n * npairs);
        iprs = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(dt.ip1 + g * dt.sip1), 0, (int)(3u * xb), 0x00020000);
#pragma unroll
        for (int x = 0; x < 3; ++x) ipx[x] = __builtin_amdgcn_readfirstlane(xb * (unsigned)x);
#pragma unroll
        for (int j = 0; j < 6; ++j) acc[j] = 0.0;
        if (blockIdx.x == 0 && dt.nchunk > n) {   // the slots behind the n partners, once per geometry
            double *tp = dt.t2part + g * dt.st2;
            const int pad = dt.nchunk - n;
            for (int idx = threadIdx.x; idx < 3 * n * pad; idx += 256) tp[(int64_t)(idx / pad) * dt.nchunk + n + idx % pad] = 0.0;
        }
    }
    // The two halves of a step of the dot: the six sums take register set c with the weighted stage values of pass k
    // (rows beyond the last pair: zero, whatever the stage holds there); the set takes the loads of pass k of the tile
    // bo belongs to.  A load stays inside its row: it starts at most at the last pair but one, and the thread whose
    // first row is the last pair finds that pair in the second element.  The sums of a tile over the lanes of its pair,
    // into the LDS buffer `par`; the 48 entries of tile jt out of it.
    [[maybe_unused]] auto dot_fma = [&](int c, int k, d2 stage) {
        const unsigned wk = opaque(wm) >> k;   // (opaque: the compiler otherwise keeps the weights of all passes in registers)
        const bool ok0 = wk >> 16 & 1u, ok1 = wk >> 24 & 1u;
        const double g0 = ok0 ? stage[0] * ((wk & 1u) ? 1.0 : 2.0) : 0.0, g1 = ok1 ? stage[1] * ((wk >> 8 & 1u) ? 1.0 : 2.0) : 0.0;
        const double ga = (ok0 && !ok1) ? 0.0 : g0, gb = (ok0 && !ok1) ? g0 : g1;
#pragma unroll
        for (int j = 0; j < 6; ++j) acc[j] = fma(qb[c][j][1], gb, fma(qb[c][j][0], ga, acc[j]));
    };
    [[maybe_unused]] auto dot_load = [&](int c, int k) {
        const unsigned f8 = opaque(du16) + 512u * (unsigned)k, l8 = 8u * (unsigned)(npairs - 2), fo = f8 < l8 ? f8 : l8;
#pragma unroll
        for (int j = 0; j < 6; ++j)
            qb[c][j] = __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(iprs, (int)(bo[j / 3] + fo), (int)ipx[j % 3], 0));
    };
    [[maybe_unused]] auto dot_reduce = [&](unsigned par) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double v = acc[j];
            v += dpp_move<0xB1>(v);
            v += dpp_move<0x4E>(v);
            v += dpp_move<0x141>(v);
            v += dpp_move<0x140>(v);
            v += __shfl_xor(v, 16);
            if ((lane & 31) == 0) lds_st(kPdRed + par * kPdRedB + 8u * (unsigned)((2 * wave + (lane >> 5)) * 6 + j), v);
            acc[j] = 0.0;
        }
    };
    [[maybe_unused]] auto dot_flush = [&](int jt, unsigned par) {
        if (threadIdx.x < 48) {
            const int t = threadIdx.x, j = t % 6, x = j % 3;
            const double sum = lds_ld(kPdRed + par * kPdRedB + 8u * (unsigned)t);
            const int e = 8 * (t_begin + jt) + t / 6;
            if (e < npairs) {
                const int hi = tri_row_small(e), lo = e - hi * (hi + 1) / 2;
                double *tp = dt.t2part + g * dt.st2;
                if (j < 3) tp[((int64_t)hi * 3 + x) * dt.nchunk + lo] = sum;
                else if (hi != lo) tp[((int64_t)lo * 3 + x) * dt.nchunk + hi] = sum;
            }
        }
    };
    // the H square of the wave: written as the accumulator holds it (row 4 reg + l4 of a tile, column l15), read as
    // A fragments (row l15, column 4 kk + l4)
    // (a base per 2 KB: the compiler pairs these accesses into ds_write2 / ds_read2, whose offsets reach that far, and
    //  otherwise forms the bases with vector adds inside the loop)
    [[maybe_unused]] unsigned sqw[4] = {0, 0, 0, 0}, sqr[2] = {0, 0};
    if constexpr (Y2) {
        const unsigned sq = kPdSq + (unsigned)wave * kPdSqB;
#pragma unroll
        for (int b = 0; b < 4; ++b) sqw[b] = opaque(sq + 8u * (unsigned)((l4 + 8 * b) * (int)kPdSqP + l15));
#pragma unroll
        for (int b = 0; b < 2; ++b) sqr[b] = opaque(sq + 8u * (unsigned)((l15 + 16 * b) * (int)kPdSqP + l4));
    }
    [[maybe_unused]] double mb[NT][KS], ha[NT][KS];   // fragments of M1_e (B operand) and of H (A operand)
    [[maybe_unused]] d4 yy[NT][NT];   // sum_e (mult(e) / 2) H_e M1_e
    // (p, q) of the wave's pair, advanced by 4 per matrix with scalar arithmetic: on the diagonal <=> q == p
    [[maybe_unused]] int pp = 0, qq = 0;
    if constexpr (Y2) {
        pp = __builtin_amdgcn_readfirstlane(tri_row_small(e0 < npairs ? e0 : 0));
        qq = (e0 < npairs ? e0 : 0) - pp * (pp + 1) / 2;
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int ta = 0; ta < NT; ++ta) yy[ti][ta] = (d4){0.0, 0.0, 0.0, 0.0};
    }
    // ... WITH TWO ROWS IN FLIGHT.  The SB row: `younger` and the M1 row requested behind the last Y phase (none before the first)
    [[maybe_unused]] auto y2_wait_sb_row = [&](int i, int K) { wait_vm_dyn8(i == 0 ? 0 : K + npieces); };
    // The M1 row of this matrix (requested behind the Y phase of the last one): younger than it are this phase's SB row
    // and its stores so far (passes c = 0..2, `stores` their bits); then its first fragments
    [[maybe_unused]] auto y2_wait_m1_row = [&](int stores) {
        wait_vm_dyn8(npieces + __builtin_popcount((unsigned)stores & 7u));
        mb[0][0] = lds_ld(fa[0][0] + kRowM);
        mb[1][0] = lds_ld(fa[1][0] + kRowM);
    };

    double mf[NT][KS];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int rt = 0; rt < NT; ++rt)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) mf[rt][kk] = lds_ld(fa[rt][kk]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    dma_row(e0 + 4);

    d4 nnA[NT][NT], nnB[NT][NT];
#pragma unroll
    for (int it = 0; it < NT; ++it)
#pragma unroll
        for (int st = 0; st < NT; ++st) nnA[it][st] = nnB[it][st] = (d4){0.0, 0.0, 0.0, 0.0};
    const d4 zero = {0.0, 0.0, 0.0, 0.0};

    // One iteration = one matrix (phase PH = i & 3: matrix parity ODD, tile parity TP).  COMPUTE: the main loop;
    // without: the two drain-only iterations behind it.
    auto iteration = [&](auto compute_tag, auto ph_tag, const int i, d4 (&nnp)[NT][NT], d4 (&nn)[NT][NT]) {
        constexpr bool COMPUTE = decltype(compute_tag)::value;
        constexpr int PH = decltype(ph_tag)::value;
        constexpr bool ODD = (PH & 1) != 0;
        constexpr unsigned TP = PH >> 1;
        // ---------------------------------------------------------------- H = M X  (+ stage writes of matrix i-1)
        d4 h[NT][NT];
        if constexpr (COMPUTE || !ODD) {
            // matrix i-1: second half of its tile (slot wave + 4) when i is even; its tile's buffer
            constexpr unsigned simm = ODD ? 0u : 4u * kPdP, sbuf = ODD ? TP : (TP ^ 1u);
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
#pragma unroll
                for (int m = 0; m < NT * NT; ++m) {
                    if constexpr (COMPUTE) {
                        // (s_setprio: a wave issuing MFMAs back to back keeps the port from its SIMD mate's loads, mfma_f64_coissue.txt)
                        const int rt = m / NT, st = m % NT;
                        __builtin_amdgcn_s_setprio(0);
                        h[rt][st] = mfma_f64(mf[rt][kk], xf[kk][st], kk == 0 ? zero : h[rt][st]);
                        __builtin_amdgcn_s_setprio(1);
                    }
                    const int f = kk * 2 + m;
                    if (m < 2 && f < 12) {
                        const int tile = f / 4, reg = f % 4;
                        const int it = tile == 0 ? 0 : 1, st2 = tile == 2 ? 1 : 0;
                        lds_st(sa[sbuf][f] + simm, nnp[it][st2][reg]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        if (!ODD && i >= 2) lds_barrier();
        if constexpr (DOT) {   // the sums of tile (i - 4) / 2 were complete before this barrier
            if (!ODD && i >= 4) dot_flush((i - 4) >> 1, TP);
        }
        // ---------------------------------------------------------------- N = X^T H  (+ everything else)
        {
            // tile jt (relative to t_begin) is complete after this barrier: written out in the N phases of iterations
            // 2 jt + 2 (passes 0..3) and 2 jt + 3 (passes 4..7); its buffer has the other parity than this matrix's tile
            int act = (ODD ? i >= 3 : i >= 2) ? vmask : 0;   // passes this wave writes in this phase (bit k)
            const int jt = (ODD ? i - 3 : i - 2) >> 1;
            constexpr unsigned bimm = (TP ^ 1u) * 8u * kPdP;
            char *ob = outg + (int64_t)(8 * (t_begin + jt)) * 8;
            const int K = younger(ODD, i);
            if constexpr (DOT) {
                // the int2e_ip1 rows (hi, lo) and (lo, hi) of the thread's pair of the tile whose passes 0..3 this phase
                // requests and 4..7 the next one (idle slots: pair 0, not written)
                if (ODD) {
                    const int e = 8 * (t_begin + jt + 1) + dslot, ec = e < npairs ? e : 0;
                    const int hi = tri_row_small(ec), lo = ec - hi * (hi + 1) / 2;
                    bo[0] = 8u * (unsigned)((hi * n + lo) * npairs);
                    bo[1] = 8u * (unsigned)((lo * n + hi) * npairs);
                }
            }
            d2 dv[4];
            [[maybe_unused]] int kd = 0;       // MODE 1: the pass that holds the diagonal u == v of this tile's columns
            [[maybe_unused]] d2 cf = {1.0, 1.0};   // MODE 1: multiplicities of the thread's two columns
            if constexpr (MODE == 1) {
                const int tg = t_begin + (jt < 0 ? 0 : jt);
                kd = tg >> 3;
                act &= ~((1 << kd) - 1);
                ob = outg + (int64_t)(8 * tg) * 8;
                const f2 c2 = *(lds_f2 *)(uintptr_t)(kPdTab + 4u * (unsigned)(8 * tg + wl));
                cf = (d2){(double)c2[0], (double)c2[1]};
            }
            asm volatile("" : "+s"(act));   // (kept a scalar: bit tests at the uses, no lane-mask copies)
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                if ((kk & 1) == 0) {
                    const int c = kk / 2, k = (ODD ? 4 : 0) + c;
                    if (act >> k & 1) {
                        if constexpr (DOT) {
                            dv[c] = lds_ld2(wod + 512u * k + bimm);
                        } else {
                            dv[c][0] = lds_ld(wo + 512u * k + bimm);
                            dv[c][1] = lds_ld(wo + 512u * k + bimm + kPdP);
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    if constexpr (COMPUTE) {
                        const int it = m == 0 ? 0 : 1, st = m == 2 ? 1 : 0;
                        __builtin_amdgcn_s_setprio(0);
                        nn[it][st] = mfma_f64(xf[kk][it], h[kk / 4][st][kk % 4], kk == 0 ? zero : nn[it][st]);
                        __builtin_amdgcn_s_setprio(1);
                        if (m == 0) {
                            // the operand row of matrix i+1 (requested one iteration ago) has landed -> fragments;
                            // then the row of matrix i+2 is requested into the same LDS row
                            if (kk == 0) {
                                if constexpr (Y2) y2_wait_sb_row(i, K);
                                else wait_vm_dyn(K);
                            }
                            if (kk < 2) {
#pragma unroll
                                for (int k2 = 0; k2 < KS; ++k2)
                                    mf[kk][k2] = lds_ld(fa[kk][k2]);
                            }
                            if (kk == 2) {
                                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                                dma_row(e0 + 4 * (i + 2));
                            }
                        }
                    }
                    if constexpr (COMPUTE && Y2) {
                        if (m == 1) {
                            if (kk < 4) {   // tile kk of H into the square
#pragma unroll
                                for (int reg = 0; reg < 4; ++reg)
                                    lds_st(sqw[2 * (kk / 2) + reg / 2] + 8u * (4u * (reg % 2) * kPdSqP + 16u * (kk % 2)), h[kk / 2][kk % 2][reg]);
                            } else {        // and back: the A fragments of row tile kk & 1, four k-steps
                                const int rt = kk & 1, k0 = kk < 6 ? 0 : 4;
#pragma unroll
                                for (int k2 = k0; k2 < k0 + 4; ++k2)
                                    ha[rt][k2] = lds_ld(sqr[rt] + 8u * 4u * k2);
                            }
                        }
                        if (m == 0 && kk == 7) y2_wait_m1_row(act >> (ODD ? 4 : 0));
                    }
                    if (m == 2 && (kk & 1) == 1) {
                        const int c = kk / 2, k = (ODD ? 4 : 0) + c;
                        if constexpr (DOT) {
                            // pass k into the sums; its register set takes pass k + 4 of this tile (odd iterations: pass
                            // k - 4 of the next tile, if the workgroup has one); behind pass 7 the tile's sums are complete
                            if (act >> k & 1) dot_fma(c, k, dv[c]);
                            const int kn = ODD ? c : 4 + c;
                            if ((vmask >> kn & 1) && (ODD ? jt + 1 < t_end - t_begin : i >= 2)) dot_load(c, kn);
                            if (c == 3 && ODD && i >= 3) dot_reduce(TP ^ 1u);
                        } else if (act >> k & 1) {
                            store_pass(k, dv[c], ob, kd, cf, jt);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        // ---------------------------------------------------------------- Y += mult(e) H M1_e
        // The B fragments of M1_e are read one k-step ahead; the pair's multiplicity, halved, is 1 for all but the n
        // diagonal pairs, whose fragments are halved as they arrive (the only vector arithmetic of the kernel's loop,
        // in 1 iteration of about 16); the sum is doubled at the end.  The next M1 row is requested behind the last read.
        if constexpr (COMPUTE && Y2) {
            auto yphase = [&](auto live_tag, auto diag_tag) {
                constexpr bool LIVE = decltype(live_tag)::value, DIAG = decltype(diag_tag)::value;
                if constexpr (DIAG) {
                    mb[0][0] *= 0.5;
                    mb[1][0] *= 0.5;
                }
#pragma unroll
                for (int kk = 0; kk < KS; ++kk)
#pragma unroll
                    for (int m = 0; m < NT * NT; ++m) {
                        const int ti = m / NT, ta = m % NT;
                        if constexpr (LIVE) {
                            __builtin_amdgcn_s_setprio(0);
                            yy[ti][ta] = mfma_f64(ha[ti][kk], mb[ta][kk], yy[ti][ta]);
                            __builtin_amdgcn_s_setprio(1);
                            if (m == 0 && kk < KS - 1) {
                                mb[0][kk + 1] = lds_ld(fa[0][kk + 1] + kRowM);
                                mb[1][kk + 1] = lds_ld(fa[1][kk + 1] + kRowM);
                            }
                            if constexpr (DIAG) {
                                if (m == 3 && kk < KS - 1) {
                                    mb[0][kk + 1] *= 0.5;
                                    mb[1][kk + 1] *= 0.5;
                                }
                            }
                        }
                        if (m == 1 && kk == KS - 1) {
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                            dma_mrow(e0 + 4 * (i + 1));
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
            };
            using Tt = std::true_type;
            using Ff = std::false_type;
            if (e0 + 4 * i >= npairs) yphase(Ff{}, Ff{});   // (idle slots of the last tile add nothing)
            else if (qq == pp) yphase(Tt{}, Tt{});
            else yphase(Tt{}, Ff{});
            qq += 4;
            while (qq > pp) {
                qq -= pp + 1;
                ++pp;
            }
        }
    };
    using T = std::true_type;
    using F = std::false_type;
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    using P2 = std::integral_constant<int, 2>;
    using P3 = std::integral_constant<int, 3>;
    int i = 0;
    for (; i + 4 <= niter; i += 4) {
        iteration(T{}, P0{}, i, nnB, nnA);
        iteration(T{}, P1{}, i + 1, nnA, nnB);
        iteration(T{}, P2{}, i + 2, nnB, nnA);
        iteration(T{}, P3{}, i + 3, nnA, nnB);
    }
    if (i < niter) {   // (niter = 2 mod 4)
        iteration(T{}, P0{}, i, nnB, nnA);
        iteration(T{}, P1{}, i + 1, nnA, nnB);
        iteration(F{}, P2{}, i + 2, nnB, nnA);
        iteration(F{}, P3{}, i + 3, nnA, nnB);
    } else {
        iteration(F{}, P0{}, i, nnB, nnA);
        iteration(F{}, P1{}, i + 1, nnA, nnB);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the rows requested beyond the last matrix)
    if constexpr (DOT) {
        // the last tile: no barrier of the loop came behind its sums
        const int ntl = t_end - t_begin;
        __syncthreads();
        dot_flush(ntl - 1, (unsigned)(ntl - 1) & 1u);
    }
    if constexpr (Y2) {
        // cross-wave sum of Y = Yd + 2 Yo over the rows and the stage, once every wave is done with them
        constexpr int NPAD = 32;
        __syncthreads();
        double *red = reinterpret_cast<double *>(lds);   // [4][NPAD][NPAD + 1]
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int ta = 0; ta < NT; ++ta)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    red[(wave * NPAD + ti * 16 + l4 + 4 * r) * (NPAD + 1) + ta * 16 + l15] = 2.0 * yy[ti][ta][r];
        __syncthreads();
        double *dst = y.partial + g * y.sws + (int64_t)blockIdx.x * n * n;
        for (int idx = threadIdx.x; idx < n * n; idx += 256) {
            const int ii = idx / n, aa = idx % n;
            const int o = ii * (NPAD + 1) + aa;
            constexpr int WS = NPAD * (NPAD + 1);
            dst[idx] = (red[o] + red[WS + o]) + (red[2 * WS + o] + red[3 * WS + o]);
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(256, 2) void ptd_kernel(PairTransformArgs a) {
    ptd_body<MODE, false>(a, Y2dArgs{});
}
// ... and with the int2e_ip1 dot in the place of the write-out (DOT = 1: a second template, the names of the kernels above stay)
template <int MODE, int DOT>
__global__ __launch_bounds__(256, 1) void ptd_kernel(PairTransformArgs a, PairDotArgs dt) {
    ptd_body<MODE, false, DOT != 0>(a, Y2dArgs{}, dt);
}

// y2d_kernel<PS>: one name, two kernels with a body each (explicit specialisations; why not two functions: DESIGN.md 4.5).
// PS = 1: the first gradient-side pair step with Y2 inside (R = X^T T_v X written as ptd_kernel<0> writes it); one
// workgroup per CU for its LDS.
template <int PS>
__global__ void y2d_kernel(Y2dArgs ya, PairTransformArgs pa);
template <>
__global__ __launch_bounds__(256, 1) void y2d_kernel<1>(Y2dArgs ya, PairTransformArgs pa) {
    ptd_body<0, true>(pa, ya);
}

// ---------------------------------------------------------------------------------- Y2 with LDS-DMA operand rows
// PS = 0 (pa is a dummy): y2_fused_kernel (y2.hip) with the machinery above: per pair v one wave computes H^T = X^T M1_v (32 MFMAs) and
// Y += mult(v) T_v H^T (32 MFMAs), M1_v = row v of the first pair step's intermediate, T_v = row v of SB, both dense
// (pair, pair) forms at the pitch pair_ld(n).  The two rows come by LDS-DMA into two wave-private LDS rows; the T
// fragments are read during the H phase and the next T row requested, the next M fragments during the Y phase and
// the M row after that requested -- each DMA has a whole iteration to land and the wait in front of either read is the
// constant "one row younger" vmcnt.  No barrier, no store, no vector instruction in the loop: the multiplicity of the
// pair (1 on the diagonal i == j, else 2) selects one of two accumulator sets (wave-uniform branch), Y = Yd + 2 Yo at
// the end.
template <>
__global__ __launch_bounds__(256, 2) void y2d_kernel<0>(Y2dArgs ya, PairTransformArgs) {
    const double *__restrict__ SB = ya.SB, *__restrict__ M1 = ya.M1, *__restrict__ X = ya.X;
    double *__restrict__ partial = ya.partial;
    const int64_t sX = ya.sX, sws = ya.sws;
    const int n = ya.n, tiles_per_wg = ya.tiles_per_wg, ppt = ya.ppt;
    constexpr int KS = 8, NT = 2;
    extern __shared__ __align__(16) char lds[];
    const int npairs = n * (n + 1) / 2, ld = pair_ld(n);
    const int64_t g = blockIdx.y;
    SB += g * sws;
    M1 += g * sws;
    X += g * sX;
    partial += g * sws;
    const int ntiles = (npairs + ppt - 1) / ppt;
    const int t_begin = blockIdx.x * tiles_per_wg, t_end = min(ntiles, t_begin + tiles_per_wg);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    d4 yD[NT][NT], yO[NT][NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int ta = 0; ta < NT; ++ta) yD[ti][ta] = yO[ti][ta] = (d4){0.0, 0.0, 0.0, 0.0};
    if (t_begin < t_end) {
        const int niter = (ppt / 4) * (t_end - t_begin);
        const unsigned rowM = (unsigned)wave * 2u * kPdRB, rowT = rowM + kPdRB;
        unsigned fa[NT][KS];   // LDS address of fragment (rt, kk) in the M row (T row: + kPdRB)
#pragma unroll
        for (int rt = 0; rt < NT; ++rt)
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                const int r = rt * 16 + l15, s = 4 * kk + l4;
                const int hi = s > r ? s : r, lo = s > r ? r : s;
                fa[rt][kk] = opaque((r < n && s < n) ? rowM + 8u * (unsigned)(hi * (hi + 1) / 2 + lo) : rowM + kPdRaw * 1024);
            }
        if (lane < 8) {
            *reinterpret_cast<double *>(lds + rowM + kPdRaw * 1024 + 8 * lane) = 0.0;
            *reinterpret_cast<double *>(lds + rowT + kPdRaw * 1024 + 8 * lane) = 0.0;
        }
        const RowDma dma((unsigned)((npairs * 8 + 15) & ~15), lane);   // (rows start on 128-byte lines)
        const int npieces = dma.npieces;
        auto dma_row = [&](const double *base, int e, unsigned dst) {
            dma.request(reinterpret_cast<const char *>(base + (int64_t)(e < npairs ? e : wave) * ld), dst);
        };
        // "everything but the youngest row has landed": npieces DMA instructions may stay in flight
        auto wait_older = [&]() {
            if (npieces >= 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else if (npieces == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
            else if (npieces == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
        };
        const int e0 = ppt * t_begin + wave;   // this wave's pair of iteration i: e0 + 4 i
        dma_row(M1, e0, rowM);
        dma_row(SB, e0, rowT);
        double xf[KS][NT];
#pragma unroll
        for (int kk = 0; kk < KS; ++kk)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int d = 4 * kk + l4, c = t * 16 + l15;
                const bool ok = d < n && c < n;
                const double v = X[ok ? d * n + c : 0];
                xf[kk][t] = ok ? v : 0.0;
            }
        double mf[NT][KS], tf[NT][KS];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int rt = 0; rt < NT; ++rt)
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) mf[rt][kk] = lds_ld(fa[rt][kk]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        dma_row(M1, e0 + 4, rowM);
        // (p, q) of the pair e, advanced by 4 per iteration with scalar arithmetic: on the diagonal <=> q == p
        int pp = __builtin_amdgcn_readfirstlane(tri_row_small(e0 < npairs ? e0 : 0)), qq = (e0 < npairs ? e0 : 0) - pp * (pp + 1) / 2;
        const d4 zero = {0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < niter; ++i) {
            const int e = e0 + 4 * i;
            const bool live = e < npairs, diag = qq == pp;
            // ------------------------------------------------------------ H^T = X^T M_e  (+ T fragments of pair e)
            d4 hT[NT][NT];
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
#pragma unroll
                for (int m = 0; m < NT * NT; ++m) {
                    const int it = m / NT, st = m % NT;
                    hT[it][st] = mfma_f64(xf[kk][it], mf[st][kk], kk == 0 ? zero : hT[it][st]);
                    if (m == 0) {
                        if (kk == 0) wait_older();   // the T row of this pair (the M row of the next one may be in flight)
                        if (kk < 2) {
#pragma unroll
                            for (int k2 = 0; k2 < KS; ++k2) tf[kk][k2] = lds_ld(fa[kk][k2] + kPdRB);
                        }
                        if (kk == 2) {
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                            dma_row(SB, e + 4, rowT);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // ------------------------------------------------------------ Y += mult(e) T_e H^T  (+ M fragments of pair e + 4)
            // (one wave-uniform branch per phase selects the accumulator set; idle slots of the last tile move data only)
            auto yphase = [&](auto live_tag, d4 (&y)[NT][NT]) {
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) {
#pragma unroll
                    for (int m = 0; m < NT * NT; ++m) {
                        const int ti = m / NT, ta = m % NT;
                        if constexpr (decltype(live_tag)::value)
                            y[ti][ta] = mfma_f64(tf[ti][kk], hT[kk / 4][ta][kk % 4], y[ti][ta]);
                        if (m == 0) {
                            if (kk == 0) wait_older();   // the M row of the next pair
                            if (kk < 2) {
#pragma unroll
                                for (int k2 = 0; k2 < KS; ++k2) mf[kk][k2] = lds_ld(fa[kk][k2]);
                            }
                            if (kk == 2) {
                                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                                dma_row(M1, e + 8, rowM);
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            };
            if (!live) yphase(std::false_type{}, yD);
            else if (diag) yphase(std::true_type{}, yD);
            else yphase(std::true_type{}, yO);
            qq += 4;
            while (qq > pp) {
                qq -= pp + 1;
                ++pp;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // cross-wave sum of Y = Yd + 2 Yo over the rows (every workgroup writes its slab, workgroups without tiles a zero one)
    constexpr int NPAD = 32;
    __syncthreads();
    double *red = reinterpret_cast<double *>(lds);   // [4][NPAD][NPAD + 1], over the rows once they are done with
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int ta = 0; ta < NT; ++ta)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                red[(wave * NPAD + ti * 16 + l4 + 4 * r) * (NPAD + 1) + ta * 16 + l15] = yD[ti][ta][r] + 2.0 * yO[ti][ta][r];
    __syncthreads();
    double *dst = partial + (int64_t)blockIdx.x * n * n;
    for (int idx = threadIdx.x; idx < n * n; idx += 256) {
        const int i = idx / n, aa = idx % n;
        const int o = i * (NPAD + 1) + aa;
        constexpr int WS = NPAD * (NPAD + 1);
        dst[idx] = (red[o] + red[WS + o]) + (red[2 * WS + o] + red[3 * WS + o]);
    }
}

int launch_y2_dma(const Y2Plan &p, const double *SB, const double *M1, const double *X, int64_t sX, int n, double *partial,
                  int64_t sws, int count, hipStream_t st) {
    Y2dArgs ya{SB, M1, X, partial, sX, sws, n, p.tiles_per_wg, p.ppt};
    hipLaunchKernelGGL((y2d_kernel<0>), dim3((unsigned)p.slabs, (unsigned)count), dim3(256), p.lds, st, ya, PairTransformArgs{});
    EVC_LAUNCH_CHECK("y2_dma");
    return 0;
}

int launch_y2_pairstep(const Y2Plan &p, const PairTransformArgs &a_in, const double *M1, double *partial, int64_t sws,
                       int count, hipStream_t st) {
    PairTransformArgs a = a_in;
    a.tiles_per_wg = p.tiles_per_wg;
    Y2dArgs ya{a.in, M1, a.C, partial, a.sC, sws, a.n, p.tiles_per_wg, p.ppt};
    static LdsAttr attr;
    if (int rc = allow_dynamic_lds(y2d_kernel<1>, attr, 160 * 1024, "y2_pairstep")) return rc;
    hipLaunchKernelGGL((y2d_kernel<1>), dim3((unsigned)p.slabs, (unsigned)count), dim3(256), p.lds, st, ya, a);
    note_kernel(EVC_PROF_Y2, "%s", y2_plan_name(p));
    EVC_LAUNCH_CHECK("y2_pairstep");
    return 0;
}

int launch_pair_transform_dot(const PairPlan &p, const PairTransformArgs &a_in, const PairDotArgs &dt, int count,
                              hipStream_t st) {
    PairTransformArgs a = a_in;
    a.tiles_per_wg = p.tiles_per_wg;
    static LdsAttr attr;
    if (int rc = allow_dynamic_lds(ptd_kernel<0, 1>, attr, 160 * 1024, "pair_transform_dot")) return rc;
    hipLaunchKernelGGL((ptd_kernel<0, 1>), dim3(p.grid_x, (unsigned)count), dim3(256), p.lds, st, a, dt);
    note_kernel(EVC_PROF_PAIR_TRANSFORM, "%s", pair_plan_name(p));
    EVC_LAUNCH_CHECK("pair_transform_dot");
    return 0;
}

// (a: tiles_per_wg filled from the plan, launch_pair_transform)
int launch_pair_transform_dma(const PairPlan &p, const PairTransformArgs &a, int count, hipStream_t st) {
    const dim3 grid(p.grid_x, (unsigned)count);
    if (p.t[0]) {
        static LdsAttr attr1;
        if (int rc = allow_dynamic_lds(ptd_kernel<1>, attr1, 160 * 1024, "pair_transform_dma")) return rc;
        hipLaunchKernelGGL((ptd_kernel<1>), grid, dim3(256), p.lds, st, a);
    } else {
        static LdsAttr attr;
        if (int rc = allow_dynamic_lds(ptd_kernel<0>, attr, 160 * 1024, "pair_transform_dma")) return rc;
        hipLaunchKernelGGL((ptd_kernel<0>), grid, dim3(256), p.lds, st, a);
    }
    note_kernel(EVC_PROF_PAIR_TRANSFORM, "%s", pair_plan_name(p));
    EVC_LAUNCH_CHECK("pair_transform_dma");
    return 0;
}

}  // namespace evc
