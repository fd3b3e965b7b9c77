// The fused pair step of the four-index rotations (two quarter steps in one kernel, n <= 32): pt_kernel, the
// phase-alternating kernel that takes EVERY form of the step, and the switch over the kernel families of a plan
// (pair_plan.hpp): the pipelined forms of the symmetric step live in pair_pipe.hip, the LDS-DMA kernels in pair_dma.hip,
// 32 < n <= 64 in pair64.hip.
// blockIdx.y = geometry of the batch (kernels.hpp).
#include "common.hpp"
#include "pair_plan.hpp"
#include "pair_rows.hpp"
#include "pt_stamps.hpp"

namespace evc {

// ------------------------------------------------------------------ fused pair transform (two quarter steps)
// For every leading index pair (p,q) the n x n block M = in[p][q][:,:] is rotated on both sides,
//     H = M X            (half result, optionally stored as K3[s'][p][q][r] = H[r][s'])
//     N = X^T H          stored as out[r'][s'][p][q]  (= two quarter steps of the rotation scheme)
// or, for the final step of the AO->OAO integral rotation, directly into the packed lower triangle
// (row (r',s') >= column (p,q), diagonal x diag_mult; electron_integral_utils.py:38-66).
// One wave per matrix: the D tiles of H = M X sit in exactly the lanes/registers the B operand of
// X^T H needs (row 4*kk + (l>>4) of H lives in register kk%4 of row-tile kk/4), so the second product
// consumes the accumulators of the first without any data movement; the X fragments serve as B
// operand of the first and A operand of the second product.  A workgroup works through tiles of 8
// leading pairs (2 matrices per wave) and stages N in LDS so that the output leaves as 64-byte runs.
// Symmetric operands (the compressed layout's pipeline) are exploited through three
// independent flags: lead_sym (in[p][q] = in[q][p]: only the n(n+1)/2 pairs q <= p are computed), in_lower
// (M = M^T: only its lower triangle is read) and rs_lower (only N[r'][s'], s' <= r', is wanted: 3 of 4
// result tiles, half the stage, half the output rows / the 8-fold compressed packed vector).
// ROWBUF (operand = dense (pair, pair) matrix, in_pairs): a leading pair's matrix is ONE contiguous row of n(n+1)/2
// doubles.  The wave fetches it with coalesced 16-byte loads (4-5 instructions of 1 KiB instead of 16 eight-byte
// gathers that touch 64 cache lines each), parks it in a wave-private LDS row and reads its MFMA fragments from there
// at lane-constant offsets tri(max(r,s), min(r,s)): triangular numbers of 16 consecutive r fall on 16 different banks.
template <int NPAD, bool ROWBUF>
__global__ __launch_bounds__(256) void pt_kernel(PairTransformArgs a) {
    constexpr int LDX = (NPAD % 32 == 0) ? NPAD + 16 : NPAD;
    constexpr int KS = NPAD / 4;
    constexpr int NT = NPAD / 16;
    constexpr int QT = 8, QP = QT + 1;
    extern __shared__ __align__(16) double sm[];
    double *Xs = sm;                  // NPAD * LDX
    double *stage = Xs + NPAD * LDX;  // n*n*QP, or n(n+1)/2*QP with rs_lower
    const int n = a.n;
    const int64_t n2 = (int64_t)n * n;
    const int64_t g = blockIdx.y;
    const double *__restrict__ in = a.in + g * a.sin;
    const double *__restrict__ C = a.C + g * a.sC;
    // The leading pairs (p,q) are handled in tiles of 8 (one 64-byte run of the output per (r',s')); a workgroup
    // owns `tpw` consecutive tiles: the stores of a tile drain while the next one is loaded and multiplied, and
    // X is staged once.
    //   plain:    tile t = (p, 8-wide q tile), pairs with q >= n are idle;
    //   lead_sym: in[p][q] = in[q][p] and the consumer reads out[..][p][q] only for q <= p (in_lower of the next
    //             step): the tiles run over the n(n+1)/2 pairs q <= p in row-major triangle order.
    const bool sym = a.lead_sym != 0;
    const int ntq = (n + QT - 1) / QT;
    const int npairs = n * (n + 1) / 2;
    const int ild = a.in_ld ? a.in_ld : npairs, old_ = a.out_ld ? a.out_ld : npairs;   // pitch of the dense (pair, pair) forms
    const int ntiles = sym ? (npairs + QT - 1) / QT : n * ntq;
    const int t_begin = blockIdx.x * a.tiles_per_wg, t_end = min(ntiles, t_begin + a.tiles_per_wg);
    if (t_begin >= t_end) return;
    EVC_PT_STAMP(0);
    EVC_PT_WG(0);
    const bool lower = a.in_lower != 0;  // the n x n matrices are symmetric and valid for r >= s only
    // rs_lower: the consumer needs the result N[r'][s'] for s' <= r' only: upper tiles of X^T H are not computed,
    // the stage holds the lower triangle (row index tri(r',s')) and only those rows of `out` are written
    const bool rsl = a.rs_lower != 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    // pair `ql` of tile t -> (p, q); false if the slot is idle
    auto pair_of = [&](int t, int ql, int &p, int &q) -> bool {
        if (sym) {
            const int e = t * QT + ql;
            if (e >= npairs) return false;
            p = (int)tri_row(e);
            q = e - p * (p + 1) / 2;
            return true;
        }
        p = t / ntq;
        q = (t - p * ntq) * QT + ql;
        return q < n;
    };
    // in_pairs: the operand is the dense (pair, pair) matrix in[tri(p,q)][tri(r,s)] (out_pairs of the previous step)
    const bool inp = a.in_pairs != 0;
    auto load_matrix = [&](double (&m)[NT][KS], bool ok, int p, int q) {
        const double *Mb = inp ? in + (int64_t)(ok ? p * (p + 1) / 2 + q : 0) * ild
                               : in + ((int64_t)(ok ? p : 0) * n + (ok ? q : 0)) * n2;
#pragma unroll
        for (int rt = 0; rt < NT; ++rt)
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                const int r = rt * 16 + l15, s = 4 * kk + l4;
                const int hi = s > r ? s : r, lo = s > r ? r : s;
                const int off = inp ? hi * (hi + 1) / 2 + lo : ((lower && s > r) ? s * n + r : r * n + s);
                m[rt][kk] = (ok && r < n && s < n) ? Mb[off] : 0.0;
            }
    };

    // ROWBUF: wave-private LDS row behind the stage; raw[] = the row in flight (lane i holds doubles 128 u + 2 i, +1 of
    // the 16-byte aligned window that starts `dlt` doubles before the row)
    const int stage_rows = rsl ? npairs : n * n;
    double *mrow = stage + (((int64_t)stage_rows * QP + 1) & ~(int64_t)1) + wave * kPtRowLen;
    const int nraw = ROWBUF ? (npairs + 1 + 127) / 128 : 0;   // wave-uniform
    double2 raw[ROWBUF ? kPtRawMax : 1];
    int dlt = 0, dlt_next = 0;
    int foff[ROWBUF ? NT : 1][ROWBUF ? KS : 1];
    if constexpr (ROWBUF) {
#pragma unroll
        for (int rt = 0; rt < NT; ++rt)
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                const int r = rt * 16 + l15, s = 4 * kk + l4;
                const int hi = s > r ? s : r, lo = s > r ? r : s;
                foff[rt][kk] = (r < n && s < n) ? hi * (hi + 1) / 2 + lo : kPtRawMax * 128;   // else: a zero slot
            }
        if (lane < 4) mrow[kPtRawMax * 128 + lane] = 0.0;
    }
    auto fetch_row = [&](bool ok, int p_, int q_, int &d_) {
        if constexpr (ROWBUF) {
            const double *row = in + (int64_t)(ok ? p_ * (p_ + 1) / 2 + q_ : 0) * ild;
            d_ = (int)((reinterpret_cast<uintptr_t>(row) >> 3) & 1);
            const double *w0 = row - d_;          // 16-byte aligned window
            const int lim = npairs + d_;          // valid doubles of the window
#pragma unroll
            for (int u = 0; u < kPtRawMax; ++u) {
                if (u < nraw) {
                    const int j = 128 * u + 2 * lane;
                    double2 v = make_double2(0.0, 0.0);
                    if (ok) {
                        if (j + 1 < lim) v = *reinterpret_cast<const double2 *>(w0 + j);
                        else if (j < lim) v.x = w0[j];
                    }
                    raw[u] = v;
                }
            }
        }
    };
    auto row_to_fragments = [&](double (&m)[NT][KS], int d_) {
        if constexpr (ROWBUF) {
#pragma unroll
            for (int u = 0; u < kPtRawMax; ++u)
                if (u < nraw) *reinterpret_cast<double2 *>(mrow + 128 * u + 2 * lane) = raw[u];
#pragma unroll
            for (int rt = 0; rt < NT; ++rt)
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) m[rt][kk] = mrow[foff[rt][kk] + d_];
        }
    };

    // first matrix of this wave: operand loads issued before the LDS fill of X
    double mf[NT][KS];
    int p = 0, q = 0;
    bool have = pair_of(t_begin, wave, p, q);
    if constexpr (ROWBUF) fetch_row(have, p, q, dlt);
    else load_matrix(mf, have, p, q);
    for (int idx = threadIdx.x; idx < NPAD * NPAD; idx += 256) {
        const int d = idx / NPAD, c = idx % NPAD;
        double v = 0.0;
        if (d < n && c < n) v = a.ct ? C[c * n + d] : C[d * n + c];
        Xs[d * LDX + c] = v;
    }
    lds_barrier();
    EVC_PT_STAMP(1);
    double xf[KS][NT];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
#pragma unroll
        for (int t = 0; t < NT; ++t) xf[kk][t] = Xs[(4 * kk + l4) * LDX + t * 16 + l15];
    if constexpr (ROWBUF) row_to_fragments(mf, dlt);
    EVC_PT_STAMP(2);

    for (int t = t_begin; t < t_end; ++t) {
        [[maybe_unused]] const int sb = 3 + 8 * (t - t_begin);
        for (int ql = wave; ql < QT; ql += 4) {
            // prefetch the wave's next matrix: slot ql + 4 of this tile, else its first slot of the next tile
            double mn[ROWBUF ? 1 : NT][ROWBUF ? 1 : KS];
            int pn = 0, qn = 0;
            const bool have_next = (ql + 4 < QT) ? pair_of(t, ql + 4, pn, qn) : (t + 1 < t_end && pair_of(t + 1, wave, pn, qn));
            [[maybe_unused]] const int fb = (t == t_begin + 1) ? 44 + (ql >= 4 ? 5 : 0) : 64;
            EVC_PT_STAMP(fb);
            if constexpr (ROWBUF) fetch_row(have_next, pn, qn, dlt_next);
            else load_matrix(mn, have_next, pn, qn);
            EVC_PT_STAMP(fb + 1);
            if (have) {  // wave-uniform
                // H = M X
                // (a dependent f64 MFMA costs ~3x the issue interval: the NT*NT tile chains are interleaved)
                d4 h[NT][NT];
#pragma unroll
                for (int rt = 0; rt < NT; ++rt)
#pragma unroll
                    for (int st = 0; st < NT; ++st) h[rt][st] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int kk = 0; kk < KS; ++kk)
#pragma unroll
                    for (int rt = 0; rt < NT; ++rt)
#pragma unroll
                        for (int st = 0; st < NT; ++st) h[rt][st] = mfma_f64(mf[rt][kk], xf[kk][st], h[rt][st]);
                EVC_PT_STAMP(fb + 2);
                if (a.k3) {
                    // lead_sym: only K3[s'][p][q][:] with q <= p is written (its consumer folds the p <-> q symmetry),
                    // as K3[s'][tri(p,q)][:] times the multiplicity of (p,q)
                    double *K3 = a.k3 + g * a.sk3;
                    const double km = (sym && p != q) ? 2.0 : 1.0;
                    const int64_t kcol = sym ? (int64_t)(p * (p + 1) / 2 + q) * n : (int64_t)p * n2 + (int64_t)q * n;
                    const int64_t krow = sym ? (int64_t)npairs * n : (int64_t)n * n2;
#pragma unroll
                    for (int rt = 0; rt < NT; ++rt)
#pragma unroll
                        for (int st = 0; st < NT; ++st)
#pragma unroll
                            for (int reg = 0; reg < 4; ++reg) {
                                const int r = rt * 16 + l4 + 4 * reg, s2 = st * 16 + l15;
                                if (r < n && s2 < n) K3[s2 * krow + kcol + r] = h[rt][st][reg] * km;
                            }
                }
                // N = X^T H : B operand of k-step kk is register kk%4 of H's row tile kk/4
                d4 nn[NT][NT];
#pragma unroll
                for (int it = 0; it < NT; ++it)
#pragma unroll
                    for (int st = 0; st < NT; ++st) nn[it][st] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int kk = 0; kk < KS; ++kk)
#pragma unroll
                    for (int it = 0; it < NT; ++it)
#pragma unroll
                        for (int st = 0; st < NT; ++st)
                            if (!(rsl && st > it)) nn[it][st] = mfma_f64(xf[kk][it], h[kk / 4][st][kk % 4], nn[it][st]);
                EVC_PT_STAMP(fb + 3);
#pragma unroll
                for (int it = 0; it < NT; ++it)
#pragma unroll
                    for (int st = 0; st < NT; ++st)
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) {
                            const int r2 = it * 16 + l4 + 4 * reg, s2 = st * 16 + l15;
                            if (r2 < n && s2 < n) {
                                if (!rsl) stage[(r2 * n + s2) * QP + ql] = nn[it][st][reg];
                                else if (s2 <= r2) stage[(r2 * (r2 + 1) / 2 + s2) * QP + ql] = nn[it][st][reg];
                            }
                        }
                EVC_PT_STAMP(fb + 4);
            }
            EVC_PT_STAMP(sb + (ql >= 4 ? 2 : 0));
            if constexpr (ROWBUF) {
                row_to_fragments(mf, dlt_next);   // (the fragments of the current matrix are consumed: same wave, in order)
            } else {
#pragma unroll
                for (int rt = 0; rt < NT; ++rt)
#pragma unroll
                    for (int kk = 0; kk < KS; ++kk) mf[rt][kk] = mn[rt][kk];
            }
            have = have_next;
            p = pn;
            q = qn;
            EVC_PT_STAMP(sb + (ql >= 4 ? 3 : 1));
        }
        lds_barrier();
        EVC_PT_STAMP(sb + 4);
        // write-out: 8 lanes cover the pair run of one (r',s')
        const int wl = threadIdx.x & 7;
        int wp = 0, wq = 0;
        const bool wok = pair_of(t, wl, wp, wq);
        const int64_t Cc = (int64_t)wp * n + wq;
        if (a.out && wok) {
            double *out = a.out + g * a.sout;
            if (!rsl) {
                for (int rs = threadIdx.x >> 3; rs < n * n; rs += 32) out[(int64_t)rs * n2 + Cc] = stage[rs * QP + wl];
            } else if (a.out_pairs) {
                // dense (pair, pair) result: row tri(r',s'), column = the leading pair's own triangle index
                const int e = t * QT + wl;
                for (int u = threadIdx.x >> 3; u < npairs; u += 32) out[(int64_t)u * old_ + e] = stage[u * QP + wl];
            } else {
                // (r', s') of stage row u, advanced incrementally: u += 32
                int r2 = (int)tri_row(threadIdx.x >> 3), s2 = (threadIdx.x >> 3) - r2 * (r2 + 1) / 2;
                for (int u = threadIdx.x >> 3; u < npairs; u += 32) {
                    out[((int64_t)r2 * n + s2) * n2 + Cc] = stage[u * QP + wl];
                    s2 += 32;
                    while (s2 > r2) {
                        s2 -= r2 + 1;
                        ++r2;
                    }
                }
            }
        }
        if (a.packed && !a.sym8) {
            double *pk = a.packed + g * a.spacked;
            if (wok)
                for (int rs = threadIdx.x >> 3; rs < n * n; rs += 32) {
                    const int64_t R = rs;
                    if (R >= Cc) pk[tri_index(R, Cc)] = stage[rs * QP + wl] * (R == Cc ? a.diag_mult : 1.0);
                }
            // zero the padding [M, packed_len) once per geometry
            if (blockIdx.x == 0 && t == t_begin) zero_packed_tail(pk, n2 * (n2 + 1) / 2, a.packed_len);
        }
        if (a.packed && a.sym8) {
            // 8-fold compressed vector: only r' >= s', p >= q, (r's') >= (pq) is kept, with its multiplicity
            double *pk = a.packed + g * a.spacked;
            if (wok && wp >= wq) {
                const int64_t v = tri_index(wp, wq);
                const double mq = (wp != wq) ? 2.0 : 1.0;
                if (rsl) {
                    // the stage row index IS u = tri(r',s'); r' == s' <=> u + 1 is a triangular number's end
                    const int u0 = (int)v + (threadIdx.x >> 3);
                    int r2 = (int)tri_row(u0), s2 = u0 - r2 * (r2 + 1) / 2;
                    for (int u = u0; u < npairs; u += 32) {
                        pk[tri_index(u, v)] =
                            stage[u * QP + wl] * ((u == v ? a.diag_mult : 1.0) * mq * (s2 == r2 ? 1.0 : 2.0));
                        s2 += 32;
                        while (s2 > r2) {
                            s2 -= r2 + 1;
                            ++r2;
                        }
                    }
                } else {
                    for (int rs = threadIdx.x >> 3; rs < n * n; rs += 32) {
                        const int r2 = rs / n, s2 = rs - r2 * n;
                        const int64_t u = tri_index(r2, s2);
                        if (r2 >= s2 && u >= v)
                            pk[tri_index(u, v)] =
                                stage[rs * QP + wl] * ((u == v ? a.diag_mult : 1.0) * mq * (r2 != s2 ? 2.0 : 1.0));
                    }
                }
            }
            if (blockIdx.x == 0 && t == t_begin) {
                const int64_t mm = (int64_t)n * (n + 1) / 2;
                zero_packed_tail(pk, mm * (mm + 1) / 2, a.packed_len);
            }
        }
        EVC_PT_STAMP(sb + 5);
        lds_barrier();  // the stage is free again; the stores above drain while the next tile is computed
        EVC_PT_STAMP(sb + 6);
    }
    EVC_PT_WG(1);
}

// One function (and LdsAttr) per instantiation; pt_kernel<16> stays within the 64 KB of dynamic LDS a kernel gets unasked.
template <int NPAD, int ROWBUF>
static int launch_pt(const PairPlan &p, const PairTransformArgs &a, dim3 grid, hipStream_t st) {
    static LdsAttr attr;
    if (NPAD == 32)
        if (int rc = allow_dynamic_lds(pt_kernel<NPAD, ROWBUF != 0>, attr, 160 * 1024, "pair_transform")) return rc;
    hipLaunchKernelGGL((pt_kernel<NPAD, ROWBUF != 0>), grid, dim3(256), p.lds, st, a);
    EVC_LAUNCH_CHECK("pair_transform");
    return 0;
}

// The family switch of a plan: this unit's own kernel, else the launcher of the family's unit.
int launch_pair_transform(const PairPlan &p, PairTransformArgs a, int count, hipStream_t st) {
    using PtLauncher = int(const PairPlan &p, const PairTransformArgs &a, dim3 grid, hipStream_t st);
    static PtLauncher *const launcher[2][2] = {{launch_pt<16, 0>, launch_pt<16, 1>}, {launch_pt<32, 0>, launch_pt<32, 1>}};
    a.tiles_per_wg = p.tiles_per_wg;
    const dim3 grid(p.grid_x, (unsigned)count);
    switch (p.kernel) {
        case kPt: EVC_TRY(launcher[p.t[0] == 32][p.t[1]](p, a, grid, st)); break;
        case kPtPipe: case kPtPipe4: EVC_TRY(launch_pair_transform_pipe(p, a, grid, st)); break;
        case kPtd: return launch_pair_transform_dma(p, a, count, st);
        case kPt64: return launch_pair_transform64(p, a, count, st);
        default:   // no kernel takes the step (beyond 32 orbitals the symmetric step alone exists: pair64.hip)
            if (a.n > kPairTransformMaxN)
                set_error("pair transform: n=%d beyond %d needs the symmetric dense-pair form", a.n, kPairTransformMaxN);
            else
                set_error("pair_transform: n=%d not supported (1..32)", a.n);
            return -1;
    }
    note_kernel(EVC_PROF_PAIR_TRANSFORM, "%s", pair_plan_name(p));
    return 0;
}

}  // namespace evc

EVC_PT_STAMP_READERS(evc_debug_read_pt_phase, evc_debug_read_pt_wg_phase)
