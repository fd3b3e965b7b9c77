// The software-pipelined forms of the symmetric pair step (pt_pipe_kernel, pt_pipe4_kernel): every N <= 32 the LDS-DMA
// kernel of pair_dma.hip does not take.  The arithmetic is pt_kernel's (pair_transform.hip, which also holds the switch
// that calls launch_pair_transform_pipe below).  blockIdx.y = geometry of the batch (kernels.hpp).
#include "common.hpp"
#include "pair_plan.hpp"
#include "pair_rows.hpp"
#include "pt_stamps.hpp"
#include <type_traits>

namespace evc {

// ------------------------------------------------------------------ software-pipelined pair transform
// pt_kernel alternates, per tile of eight leading pairs, a matrix-core phase (two matrices per wave) with a
// write-out phase, and every workgroup of the launch does so at the same moments: phase stamps (tools/micro/
// pt_stamps.py) show the 56 MFMAs of a matrix issue in 1.8 us of the 3.5 us a wave spends per matrix (the rest: index
// arithmetic, the operand row's round trip through LDS, the stage writes), and the write-out of a tile takes 2.5-2.9 us
// because the whole chip stores at once (15 MB per phase) and then not at all.  This kernel is the same arithmetic for
// the fully symmetric case (dense (pair, pair) operand, q <= p, lower-triangle results) as ONE software pipeline per
// wave: everything that is not an MFMA is cut into small pieces that are issued between the MFMA groups of the
// CURRENT matrix --
//   * H phase of matrix i (KS groups of NT*NT MFMAs): the stage writes of matrix i-1's result (kept in registers);
//   * N phase: the operand row of matrix i+1 goes from registers to the wave's LDS row and comes back as MFMA
//     fragments (the registers of matrix i's fragments are free after its H phase), the global fetch of matrix i+2's
//     row is issued, half of the write-out passes of an EARLIER tile --
// with a double-buffered stage (8 doubles per result row and buffer, the slot XOR-swizzled by the row against bank
// conflicts of the accumulator layout) and ONE workgroup barrier per tile: barrier(j) sits after the H phase of
// the first matrix of tile j+1 (which wrote the last results of tile j); tile j is then written out during the
// following two N phases, before barrier(j+1), after which its buffer is written again.  The stores of the launch
// are spread evenly over its duration.  (vmcnt counts loads and stores in order on gfx9: the wait for an operand row
// also waits for every store issued before it, so the write-out sits in the N phases only and the row is awaited at
// the start of the next one, an H phase later.)
// MODE 0: dense (pair, pair) result out[tri(r',s')][tri(p,q)];
// MODE 1: the 8-fold compressed packed vector.
template <int NPAD, int MODE>
__global__ __launch_bounds__(256) void pt_pipe_kernel(PairTransformArgs a) {
    constexpr int KS = NPAD / 4;
    constexpr int NT = NPAD / 16;
    constexpr int NPASS_MAX = (NPAD * (NPAD + 1) / 2 + 63) / 64;   // write-out passes of a tile (64 result rows each)
    constexpr int PH2 = (NPASS_MAX + 1) / 2;                       // ... per N phase
    constexpr int NRES = NT * (NT + 1) / 2 * 4;                    // result registers (doubles) of a matrix per lane
    constexpr int SPG = (NRES + KS - 1) / KS;                      // stage writes per MFMA group
    constexpr int FPG = (NT * KS + (KS - 2) - 1) / (KS - 2);       // fragment reads per MFMA group (groups 2..KS-1)
    constexpr int PPG = (PH2 + KS - 1) / KS;                       // write-out passes per MFMA group (N phase)
    constexpr int RAWN = (NPAD * (NPAD + 1) / 2 + 1 + 127) / 128;  // 16-byte loads per lane that cover a row
    extern __shared__ __align__(16) double sm[];
    const int n = a.n;
    const int npairs = n * (n + 1) / 2;
    const int64_t g = blockIdx.y;
    const double *__restrict__ in = a.in + g * a.sin;
    const double *__restrict__ C = a.C + g * a.sC;
    const int ild = a.in_ld ? a.in_ld : npairs, old_ = a.out_ld ? a.out_ld : npairs;   // pitch of the dense (pair, pair) forms
    const int ntiles = (npairs + 7) / 8;
    const int t_begin = blockIdx.x * a.tiles_per_wg, t_end = min(ntiles, t_begin + a.tiles_per_wg);
    if (t_begin >= t_end) return;
    EVC_PT_WG(0);
    EVC_PT_STAMP(0);
    const int niter = 2 * (t_end - t_begin);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    double *mrow = sm + wave * kPtRowLen;   // the wave's operand row
    // the stage: result row u = tri(r',s') of buffer b (tile parity), slot s (pair of the tile) at
    //   u * 16 + b * 8 + (s ^ f(u)),  f(u) = 2 ((u >> 1) & 3)
    // (f is even: the slots 2t, 2t+1 of a row stay an aligned 16-byte pair, which the write-out reads with one
    //  ds_read_b128; 16 consecutive rows of one slot fall on 8 bank pairs, a 2-way conflict on the 12 stage writes of
    //  a matrix; f(u + 64) = f(u))
    double *stage = sm + 4 * kPtRowLen;     // (behind the npairs rows: one dump row of 16 doubles)
    char *__restrict__ outb = nullptr;
    if constexpr (MODE == 0) outb = reinterpret_cast<char *>(a.out + g * a.sout);
    else outb = reinterpret_cast<char *>(a.packed + g * a.spacked);

    int foff[NT][KS];   // fragment (rt, kk) of the symmetric n x n matrix in its packed row
#pragma unroll
    for (int rt = 0; rt < NT; ++rt)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const int r = rt * 16 + l15, s = 4 * kk + l4;
            const int hi = s > r ? s : r, lo = s > r ? r : s;
            foff[rt][kk] = (r < n && s < n) ? hi * (hi + 1) / 2 + lo : kPtRawMax * 128;   // else: a zero slot
        }
    // stage index of result register (it, st <= it, reg) for slot `wave` of buffer 0 (registers that hold no result
    // go to a dump row behind the last one); the slot of the second matrix of a tile and the buffer are XORed in:
    // (slot + 4) ^ f = (slot ^ f) ^ 4 for slot < 4
    int sa[NT][NT][4];
#pragma unroll
    for (int it = 0; it < NT; ++it)
#pragma unroll
        for (int st = 0; st <= it; ++st)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int r2 = it * 16 + l4 + 4 * reg, s2 = st * 16 + l15;
                const int u = r2 * (r2 + 1) / 2 + s2;
                sa[it][st][reg] = (r2 < n && s2 <= r2) ? u * 16 + (wave ^ (((u >> 1) & 3) << 1)) : npairs * 16 + wave;
            }
    [[maybe_unused]] const int dq = l15 - l4;   // result register reg of a diagonal tile is r' == s'  <=>  dq == 4 reg
    if (lane < 4) mrow[kPtRawMax * 128 + lane] = 0.0;

    d2 raw[RAWN];
    // row e of the operand (e clamped: idle slots fetch row 0 and their result is never written out)
    auto fetch = [&](int e) -> int { return fetch_packed_row(in + (int64_t)(e < npairs ? e : 0) * ild, npairs, lane, raw); };
    auto park = [&]() { park_packed_row(mrow, lane, raw); };

    const int e0 = 8 * t_begin + wave;   // this wave's leading pair of iteration i: e0 + 4 i
    int d_rd = fetch(e0);
    // the X fragments straight from global memory (every wave its own copy: 16 rows of 128 bytes per load instruction,
    // one latency together with the first operand row; no LDS staging, no barrier)
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
    if constexpr (MODE == 1) {
        if (blockIdx.x == 0)   // zero the padding [M, packed_len) once per geometry
            zero_packed_tail(a.packed + g * a.spacked, (int64_t)npairs * (npairs + 1) / 2, a.packed_len);
    }
    EVC_PT_STAMP(1);
    double mf[NT][KS];
    park();
#pragma unroll
    for (int rt = 0; rt < NT; ++rt)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) mf[rt][kk] = mrow[foff[rt][kk] + d_rd];
    int d_next = fetch(e0 + 4);
    EVC_PT_STAMP(2);

    // write-out: 4 lanes cover the pair run of one result row, two pairs (16 bytes) each; thread (wl, ur) takes the
    // columns wl, wl + 1 (wl even) of rows u0 + 64 k
    const int wl = 2 * (threadIdx.x & 3), ur = threadIdx.x >> 2;
    [[maybe_unused]] const unsigned stride_b = 64u * (unsigned)old_ * 8u;     // MODE 0: bytes between two passes

    // the result of a matrix stays in registers until it is staged during the next matrix's H phase: two register
    // sets, alternating (the loop body is instantiated for even and odd i)
    d4 nnA[NT][NT], nnB[NT][NT];
#pragma unroll
    for (int it = 0; it < NT; ++it)
#pragma unroll
        for (int st = 0; st < NT; ++st) nnA[it][st] = nnB[it][st] = (d4){0.0, 0.0, 0.0, 0.0};

    // One iteration = one matrix.  COMPUTE: the main loop (idle slots of the last tile compute on row 0, their result is
    // never written out); without: the two drain-only iterations behind it.  Everything that is not an MFMA sits
    // BETWEEN two MFMAs in program order (sched_barrier pins it there), a few instructions at a time: the LDS and
    // memory operations are spread evenly and their latencies end behind MFMAs, not behind each other.
    auto iteration = [&](auto compute_tag, auto odd_tag, const int i, d4 (&nnp)[NT][NT], d4 (&nn)[NT][NT]) {
        constexpr bool COMPUTE = decltype(compute_tag)::value, ODD = decltype(odd_tag)::value;
        const int ei = e0 + 4 * i;
        EVC_PT_STAMP(3 + 3 * i);
        // ---------------------------------------------------------------- H = M X  (+ stage writes of matrix i-1)
        d4 h[NT][NT];
#pragma unroll
        for (int rt = 0; rt < NT; ++rt)
#pragma unroll
            for (int st = 0; st < NT; ++st) h[rt][st] = (d4){0.0, 0.0, 0.0, 0.0};
        if constexpr (COMPUTE || !ODD) {
            // results of matrix i-1: slot wave + 4 ((i-1) & 1) of the buffer of ITS tile (iteration 0 and idle slots
            // write values nobody reads)
            const int xm = ((((i - 1) >> 1) & 1) << 3) | (ODD ? 0 : 4);
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
#pragma unroll
                for (int m = 0; m < NT * NT; ++m) {
                    if constexpr (COMPUTE) {
                        const int rt = m / NT, st = m % NT;
                        // (equal priorities let a wave that issues MFMAs back to back keep the issue port: the SIMD mate's
                        // loads, stores and LDS operations go first, tools/micro/mfma_coissue.hip)
                        __builtin_amdgcn_s_setprio(0);
                        h[rt][st] = mfma_f64(mf[rt][kk], xf[kk][st], h[rt][st]);
                        __builtin_amdgcn_s_setprio(1);
                    }
                    const int f = kk * SPG + m;   // the stage write that follows this MFMA
                    if (m < SPG && f < NRES) {
                        const int tile = f / 4, reg = f % 4;
                        const int it = tile == 0 ? 0 : 1, st2 = tile == 2 ? 1 : 0;   // tiles (0,0), (1,0), (1,1)
                        double v = nnp[it][st2][reg];
                        // MODE 1: the write-out doubles every element, r' == s' has multiplicity 1
                        if (MODE == 1 && it == st2) v *= (dq == 4 * reg) ? 0.5 : 1.0;
                        stage[sa[it][st2][reg] ^ xm] = v;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        EVC_PT_STAMP(4 + 3 * i);
        if (!ODD && i >= 2 && i <= niter) lds_barrier();
        EVC_PT_STAMP(5 + 3 * i);
        // ---------------------------------------------------------------- N = X^T H
#pragma unroll
        for (int it = 0; it < NT; ++it)
#pragma unroll
            for (int st = 0; st < NT; ++st) nn[it][st] = (d4){0.0, 0.0, 0.0, 0.0};
        {
            // write-out: tile j's result is complete after barrier(j) (H phase of iteration 2j+2); it is written out in
            // the N phases of iterations 2j+2 (passes 0 .. PH2 - 1) and 2j+3 (the rest), PPG passes per MFMA group
            const int jn = ODD ? (i - 3) / 2 : (i - 2) / 2;
            constexpr int kn = ODD ? PH2 : 0;
            const bool dn = (ODD ? i >= 3 : i >= 2) && 2 * jn < niter;
            // per tile and thread: LDS index of pass 0, byte offset of its store, rows left, the factors of its two columns
            const int ew = 8 * (t_begin + jn) + wl;            // the first pair (column) this thread writes
            const int u0 = (MODE == 0 ? 0 : ew) + ur;          // MODE 1: rows u >= v = ew only
            const int rem = (dn && ew < npairs) ? npairs - u0 : 0;   // pass k is valid  <=>  64 k < rem
            const bool two = ew + 1 < npairs;                  // (the last pair of an odd count stands alone)
            const d2 *dsrc = reinterpret_cast<const d2 *>(stage + (u0 * 16 + ((jn & 1) << 3) + (wl ^ (((u0 >> 1) & 3) << 1))));
            d2 fac = {1.0, 1.0};
            [[maybe_unused]] d2 fac0 = {1.0, 1.0};
            unsigned off0 = 0;
            [[maybe_unused]] unsigned offA = 0;
            if (dn) {
                if constexpr (MODE == 0) {
                    off0 = (unsigned)(u0 * old_ + ew) * 8u;
                } else {
                    fac[0] = tri_is_diag(ew) ? 2.0 : 4.0;          // multiplicity of (p,q) x 2 (see the stage writes)
                    fac[1] = tri_is_diag(ew + 1) ? 2.0 : 4.0;
                    // pass 0: the thread with u == v takes diag_mult; row u = ew has no column ew + 1 (u < v)
                    fac0[0] = ur == 0 ? fac[0] * a.diag_mult : fac[0];
                    fac0[1] = ur == 1 ? fac[1] * a.diag_mult : fac[1];
                    off0 = (unsigned)(u0 * (u0 + 1) / 2 + ew) * 8u;
                    offA = (unsigned)(64 * u0) * 8u;               // tri(u0 + 64 k) = tri(u0) + k (64 u0) + 2048 k^2 + 32 k
                }
            }
            constexpr int NM = NT * (NT + 1) / 2;   // MFMAs of a group: tiles (0,0), (1,0), (1,1)
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                d2 dv[PPG];
#pragma unroll
                for (int c = 0; c < PPG; ++c) {
                    const int k = kk * PPG + c;   // pass kn + k
                    dv[c] = (k < PH2 && 64 * (kn + k) < rem) ? dsrc[512 * (kn + k)] : (d2){0.0, 0.0};
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    if constexpr (COMPUTE) {
                        const int it = m == 0 ? 0 : 1, st = m == 2 ? 1 : 0;
                        __builtin_amdgcn_s_setprio(0);
                        nn[it][st] = mfma_f64(xf[kk][it], h[kk / 4][st][kk % 4], nn[it][st]);
                        __builtin_amdgcn_s_setprio(1);
                    }
                    if (COMPUTE && m == 0) {
                        // the operand row of matrix i+1 (fetched one iteration ago) -> the wave's LDS row -> fragments;
                        // the row of matrix i+2 is requested (behind the last matrix: row 0, unused)
                        if (kk == 0) {
                            park();
                            d_rd = d_next;
                        }
                        if (kk == 1) d_next = fetch(ei + 8);
                        if (kk >= 2) {
#pragma unroll
                            for (int rt = 0; rt < NT; ++rt)
#pragma unroll
                                for (int k2 = 0; k2 < KS; ++k2)
                                    if ((rt * KS + k2) / FPG == kk - 2) mf[rt][k2] = mrow[foff[rt][k2] + d_rd];
                        }
                    }
                    if (m == NM - 1) {
#pragma unroll
                        for (int c = 0; c < PPG; ++c) {
                            const int k = kk * PPG + c;
                            if (k < PH2 && 64 * (kn + k) < rem) {
                                const unsigned kq = (unsigned)(kn + k);
                                unsigned off;
                                d2 v;
                                bool second = two;
                                if constexpr (MODE == 0) {
                                    off = off0 + kq * stride_b;
                                    v = dv[c];
                                } else {
                                    off = off0 + kq * offA + (2048u * kq * kq + 32u * kq) * 8u;
                                    v = dv[c] * (kq == 0 ? fac0 : fac);
                                    if (kq == 0) second = two && ur >= 1;   // row u = ew: column ew + 1 is above the diagonal
                                }
                                if (second) *reinterpret_cast<d2 *>(outb + off) = v;
                                else *reinterpret_cast<double *>(outb + off) = v[0];
                            }
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (i == 3) EVC_PT_STAMP(40 + kk);
            }
        }
    };
    for (int i = 0; i < niter; i += 2) {   // (niter is even)
        iteration(std::true_type{}, std::false_type{}, i, nnB, nnA);
        iteration(std::true_type{}, std::true_type{}, i + 1, nnA, nnB);
    }
    iteration(std::false_type{}, std::false_type{}, niter, nnB, nnA);
    iteration(std::false_type{}, std::true_type{}, niter + 1, nnA, nnB);
    EVC_PT_STAMP(3 + 3 * (niter + 2));
    EVC_PT_WG(1);
}

// ------------------------------------------------------------------ the same for a few geometries: tiles of 4 pairs
// With one or two geometries per launch pt_pipe_kernel has 59 workgroups of two matrices per wave and spends more
// time in its prologue and drain-only tail than in between.  Here a tile is 4 leading pairs -- ONE matrix per wave --
// so there are twice as many workgroups of half the length (the write-out runs are 32 bytes, which does not matter at
// this size).  Same pipeline with period one: matrix i's result is staged during the H phase of matrix i+1, barrier,
// and the tile is written out during that matrix's N phase; stage = 4 doubles per result row and buffer.  No K3.
template <int NPAD, int MODE>
__global__ __launch_bounds__(256) void pt_pipe4_kernel(PairTransformArgs a) {
    constexpr int KS = NPAD / 4;
    constexpr int NT = NPAD / 16;
    constexpr int NPASS = (NPAD * (NPAD + 1) / 2 + 127) / 128;     // write-out passes of a tile (128 result rows each)
    constexpr int NRES = NT * (NT + 1) / 2 * 4;
    constexpr int SPG = (NRES + KS - 1) / KS;
    constexpr int FPG = (NT * KS + (KS - 2) - 1) / (KS - 2);
    constexpr int PPG = (NPASS + KS - 1) / KS;
    constexpr int RAWN = (NPAD * (NPAD + 1) / 2 + 1 + 127) / 128;
    extern __shared__ __align__(16) double sm[];
    const int n = a.n;
    const int npairs = n * (n + 1) / 2;
    const int64_t g = blockIdx.y;
    const double *__restrict__ in = a.in + g * a.sin;
    const double *__restrict__ C = a.C + g * a.sC;
    const int ild = a.in_ld ? a.in_ld : npairs, old_ = a.out_ld ? a.out_ld : npairs;   // pitch of the dense (pair, pair) forms
    const int ntiles = (npairs + 3) / 4;
    const int t_begin = blockIdx.x * a.tiles_per_wg, t_end = min(ntiles, t_begin + a.tiles_per_wg);
    if (t_begin >= t_end) return;
    const int niter = t_end - t_begin;   // one matrix per wave and tile
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    double *mrow = sm + wave * kPtRowLen;
    // stage: row u, buffer b, slot s at u * 8 + b * 4 + (s ^ f(u)), f(u) = 2 ((u >> 1) & 1); one dump row behind
    double *stage = sm + 4 * kPtRowLen;
    char *__restrict__ outb = nullptr;
    if constexpr (MODE == 0) outb = reinterpret_cast<char *>(a.out + g * a.sout);
    else outb = reinterpret_cast<char *>(a.packed + g * a.spacked);

    int foff[NT][KS];
#pragma unroll
    for (int rt = 0; rt < NT; ++rt)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const int r = rt * 16 + l15, s = 4 * kk + l4;
            const int hi = s > r ? s : r, lo = s > r ? r : s;
            foff[rt][kk] = (r < n && s < n) ? hi * (hi + 1) / 2 + lo : kPtRawMax * 128;
        }
    int sa[NT][NT][4];
#pragma unroll
    for (int it = 0; it < NT; ++it)
#pragma unroll
        for (int st = 0; st <= it; ++st)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int r2 = it * 16 + l4 + 4 * reg, s2 = st * 16 + l15;
                const int u = r2 * (r2 + 1) / 2 + s2;
                sa[it][st][reg] = (r2 < n && s2 <= r2) ? u * 8 + (wave ^ (((u >> 1) & 1) << 1)) : npairs * 8 + wave;
            }
    [[maybe_unused]] const int dq = l15 - l4;
    if (lane < 4) mrow[kPtRawMax * 128 + lane] = 0.0;

    d2 raw[RAWN];
    auto fetch = [&](int e) -> int { return fetch_packed_row(in + (int64_t)(e < npairs ? e : 0) * ild, npairs, lane, raw); };
    auto park = [&]() { park_packed_row(mrow, lane, raw); };

    const int e0 = 4 * t_begin + wave;   // this wave's leading pair of iteration i: e0 + 4 i
    int d_rd = fetch(e0);
    double xf[KS][NT];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int d = 4 * kk + l4, c = t * 16 + l15;
            const bool ok = d < n && c < n;
            const double v = C[ok ? (a.ct ? c * n + d : d * n + c) : 0];
            xf[kk][t] = ok ? v : 0.0;
        }
    if constexpr (MODE == 1) {
        if (blockIdx.x == 0) zero_packed_tail(a.packed + g * a.spacked, (int64_t)npairs * (npairs + 1) / 2, a.packed_len);
    }
    double mf[NT][KS];
    park();
#pragma unroll
    for (int rt = 0; rt < NT; ++rt)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) mf[rt][kk] = mrow[foff[rt][kk] + d_rd];
    int d_next = fetch(e0 + 4);

    // write-out: 2 lanes cover the 4 pairs of one result row (16 bytes each); thread (wl, ur): columns wl, wl + 1 of
    // rows u0 + 128 k
    const int wl = 2 * (threadIdx.x & 1), ur = threadIdx.x >> 1;
    [[maybe_unused]] const unsigned stride_b = 128u * (unsigned)old_ * 8u;

    d4 nnp[NT][NT];
#pragma unroll
    for (int it = 0; it < NT; ++it)
#pragma unroll
        for (int st = 0; st < NT; ++st) nnp[it][st] = (d4){0.0, 0.0, 0.0, 0.0};

    auto iteration = [&](auto compute_tag, const int i) {
        constexpr bool COMPUTE = decltype(compute_tag)::value;
        const int ei = e0 + 4 * i;
        // ---------------------------------------------------------------- H = M X  (+ stage writes of matrix i-1)
        d4 h[NT][NT];
#pragma unroll
        for (int rt = 0; rt < NT; ++rt)
#pragma unroll
            for (int st = 0; st < NT; ++st) h[rt][st] = (d4){0.0, 0.0, 0.0, 0.0};
        {
            const int xm = ((i - 1) & 1) << 2;   // buffer of tile i-1
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
#pragma unroll
                for (int m = 0; m < NT * NT; ++m) {
                    if constexpr (COMPUTE) {
                        const int rt = m / NT, st = m % NT;
                        __builtin_amdgcn_s_setprio(0);
                        h[rt][st] = mfma_f64(mf[rt][kk], xf[kk][st], h[rt][st]);
                        __builtin_amdgcn_s_setprio(1);
                    }
                    const int f = kk * SPG + m;
                    if (m < SPG && f < NRES) {
                        const int tile = f / 4, reg = f % 4;
                        const int it = tile == 0 ? 0 : 1, st2 = tile == 2 ? 1 : 0;
                        double v = nnp[it][st2][reg];
                        if (MODE == 1 && it == st2) v *= (dq == 4 * reg) ? 0.5 : 1.0;
                        stage[sa[it][st2][reg] ^ xm] = v;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        if (i >= 1) lds_barrier();   // tile i-1 is complete (and tile i-2 written out by everybody)
        // ---------------------------------------------------------------- N = X^T H
        d4 nn[NT][NT];
#pragma unroll
        for (int it = 0; it < NT; ++it)
#pragma unroll
            for (int st = 0; st < NT; ++st) nn[it][st] = (d4){0.0, 0.0, 0.0, 0.0};
        {
            const int jn = i - 1;                              // the tile written out now
            const bool dn = jn >= 0;
            const int ew = 4 * (t_begin + jn) + wl;
            const int u0 = (MODE == 0 ? 0 : ew) + ur;
            const int rem = (dn && ew < npairs) ? npairs - u0 : 0;   // pass k is valid  <=>  128 k < rem
            const bool two = ew + 1 < npairs;
            const d2 *dsrc = reinterpret_cast<const d2 *>(stage + (u0 * 8 + ((jn & 1) << 2) + (wl ^ (((u0 >> 1) & 1) << 1))));
            d2 fac = {1.0, 1.0};
            [[maybe_unused]] d2 fac0 = {1.0, 1.0};
            unsigned off0 = 0;
            [[maybe_unused]] unsigned offA = 0;
            if (dn) {
                if constexpr (MODE == 0) {
                    off0 = (unsigned)(u0 * old_ + ew) * 8u;
                } else {
                    fac[0] = tri_is_diag(ew) ? 2.0 : 4.0;
                    fac[1] = tri_is_diag(ew + 1) ? 2.0 : 4.0;
                    fac0[0] = ur == 0 ? fac[0] * a.diag_mult : fac[0];
                    fac0[1] = ur == 1 ? fac[1] * a.diag_mult : fac[1];
                    off0 = (unsigned)(u0 * (u0 + 1) / 2 + ew) * 8u;
                    offA = (unsigned)(128 * u0) * 8u;   // tri(u0 + 128 k) = tri(u0) + k (128 u0) + 8192 k^2 + 64 k
                }
            }
            constexpr int NM = NT * (NT + 1) / 2;
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                d2 dv[PPG];
#pragma unroll
                for (int c = 0; c < PPG; ++c) {
                    const int k = kk * PPG + c;
                    dv[c] = (k < NPASS && 128 * k < rem) ? dsrc[512 * k] : (d2){0.0, 0.0};
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    if constexpr (COMPUTE) {
                        const int it = m == 0 ? 0 : 1, st = m == 2 ? 1 : 0;
                        __builtin_amdgcn_s_setprio(0);
                        nn[it][st] = mfma_f64(xf[kk][it], h[kk / 4][st][kk % 4], nn[it][st]);
                        __builtin_amdgcn_s_setprio(1);
                    }
                    if (COMPUTE && m == 0) {
                        if (kk == 0) {
                            park();
                            d_rd = d_next;
                        }
                        if (kk == 1) d_next = fetch(ei + 8);
                        if (kk >= 2) {
#pragma unroll
                            for (int rt = 0; rt < NT; ++rt)
#pragma unroll
                                for (int k2 = 0; k2 < KS; ++k2)
                                    if ((rt * KS + k2) / FPG == kk - 2) mf[rt][k2] = mrow[foff[rt][k2] + d_rd];
                        }
                    }
                    if (m == NM - 1) {
#pragma unroll
                        for (int c = 0; c < PPG; ++c) {
                            const int k = kk * PPG + c;
                            if (k < NPASS && 128 * k < rem) {
                                const unsigned kq = (unsigned)k;
                                unsigned off;
                                d2 v;
                                bool second = two;
                                if constexpr (MODE == 0) {
                                    off = off0 + kq * stride_b;
                                    v = dv[c];
                                } else {
                                    off = off0 + kq * offA + (8192u * kq * kq + 64u * kq) * 8u;
                                    v = dv[c] * (kq == 0 ? fac0 : fac);
                                    if (kq == 0) second = two && ur >= 1;
                                }
                                if (second) *reinterpret_cast<d2 *>(outb + off) = v;
                                else *reinterpret_cast<double *>(outb + off) = v[0];
                            }
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
#pragma unroll
        for (int it = 0; it < NT; ++it)
#pragma unroll
            for (int st = 0; st <= it; ++st) nnp[it][st] = nn[it][st];
    };
    for (int i = 0; i < niter; ++i) iteration(std::true_type{}, i);
    iteration(std::false_type{}, niter);
}

// One function (and LdsAttr) per instantiation; pt_pipe4_kernel stays within the 64 KB of dynamic LDS a kernel gets unasked.
template <int NPAD, int MODE>
static int launch_pt_pipe(const PairPlan &p, const PairTransformArgs &a, dim3 grid, hipStream_t st) {
    static LdsAttr attr;
    if (int rc = allow_dynamic_lds(pt_pipe_kernel<NPAD, MODE>, attr, 160 * 1024, "pair_transform")) return rc;
    hipLaunchKernelGGL((pt_pipe_kernel<NPAD, MODE>), grid, dim3(256), p.lds, st, a);
    EVC_LAUNCH_CHECK("pair_transform_pipe");
    return 0;
}
template <int NPAD, int MODE>
static int launch_pt_pipe4(const PairPlan &p, const PairTransformArgs &a, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL((pt_pipe4_kernel<NPAD, MODE>), grid, dim3(256), p.lds, st, a);
    EVC_LAUNCH_CHECK("pair_transform_pipe4");
    return 0;
}

int launch_pair_transform_pipe(const PairPlan &p, const PairTransformArgs &a, dim3 grid, hipStream_t st) {
    using PtLauncher = int(const PairPlan &p, const PairTransformArgs &a, dim3 grid, hipStream_t st);
#define EVC_PT_FAMILY(launcher_) {{launcher_<16, 0>, launcher_<16, 1>}, {launcher_<32, 0>, launcher_<32, 1>}}
    static PtLauncher *const launcher[2][2][2] = {EVC_PT_FAMILY(launch_pt_pipe), EVC_PT_FAMILY(launch_pt_pipe4)};
#undef EVC_PT_FAMILY
    return launcher[p.kernel == kPtPipe4][p.t[0] == 32][p.t[1]](p, a, grid, st);
}

}  // namespace evc

// (the stamps of the last pt_pipe_kernel launch: what tools/micro/pt_stamps.py reads by default)
EVC_PT_STAMP_READERS(evc_debug_read_pt, evc_debug_read_pt_wg)
