// Which kernel runs a pair step or the Y2 contraction, and with what launch: the plan is a value --
// plan_pair_step, plan_y2 and, for the gradient side of the symmetric pipeline, plan_grad_pairs, pure functions of the
// launch arguments, the batch size and the knobs.  It names ONE kernel instantiation, its tiling, grid and dynamic LDS;
// the launchers (pair_transform.hip, pair_pipe.hip, pair_dma.hip, pair64.hip, y2.hip) launch exactly that and decide nothing.  The plans are
// host code; the LDS layout constants kPd* and p64_rowlen below are shared with the kernels of pair_dma.hip and
// pair64.hip, which lay out the LDS the plans size.
#pragma once
#include <stdlib.h>

#include "kernels.hpp"

namespace evc {

struct PairKnobs {       // read once per process (pair_knobs); all default 1
    bool pt_dma;         // EVC_PT_DMA: the LDS-DMA kernels of pair_dma.hip (ptd_kernel, y2d_kernel), 16 < n <= 30
    bool pt_pipe;        // EVC_PT_PIPE: the software-pipelined pt_pipe_kernel / pt_pipe4_kernel (0: the phase-alternating pt_kernel)
    bool y2_pairstep;    // EVC_Y2_PAIRSTEP: Y2 inside the first gradient-side pair step (0: y2d_kernel<0>, then ptd_kernel<0>)
    bool ip1_pairstep;   // EVC_IP1_PAIRSTEP: the int2e_ip1 dot inside the second (0: it writes the AO-basis 2-RDM and
                         // ip1_dh_kernel's pair blocks contract it)
};
inline const PairKnobs &pair_knobs() {
    static const PairKnobs knobs = [] {
        auto on = [](const char *name) { return !(getenv(name) && atoi(getenv(name)) == 0); };
        return PairKnobs{on("EVC_PT_DMA"), on("EVC_PT_PIPE"), on("EVC_Y2_PAIRSTEP"), on("EVC_IP1_PAIRSTEP")};
    }();
    return knobs;
}

// ---- LDS layouts of the kernels whose launches the plans size (pair_dma.hip, pair64.hip)
constexpr int kPdMaxN = 30;
constexpr unsigned kPdRaw = 4;                    // 1 KiB pieces per operand row (465 + 1 doubles at most)
constexpr unsigned kPdRB = kPdRaw * 1024 + 64;    // bytes per wave: the row and a zero slot behind it
constexpr unsigned kPdStage = 4 * kPdRB;          // byte offset of the stage (a multiple of 256)
constexpr unsigned kPdP = 3872;                   // slot pitch of the stage: >= 8 (465 + 16) bytes, = 32 mod 128
constexpr unsigned kPdTab = kPdStage + 16 * kPdP;   // MODE 1: multiplicity of pair u (1 on the diagonal i == j, else 2), 512 floats
constexpr unsigned kPdLds = kPdTab, kPdLds1 = kPdTab + 512 * 4;
// DOT: per tile parity the 48 sums of a tile (8 pairs x 2 orders of the pair x 3 components), behind the stage
constexpr unsigned kPdRed = kPdTab, kPdRedB = 48 * 8, kPdLdsDot = kPdRed + 2 * kPdRedB;
// The pair step that also contracts Y2 (y2d_kernel<1>): the M1 rows of the four waves behind their SB rows, the stage
// behind those, and per wave a 32 x 32 square (pitch 34 doubles: its fragment reads are conflict free) through which
// H goes from its accumulator form to the A-operand form.  130 KB: one workgroup per CU.
constexpr unsigned kPdStageY = 8 * kPdRB;
constexpr unsigned kPdSqP = 34, kPdSqB = 32 * kPdSqP * 8;
constexpr unsigned kPdSq = kPdStageY + 16 * kPdP;
constexpr unsigned kPdLdsY = kPdSq + 4 * kPdSqB;
// pair64.hip: doubles of one wave's row / stage buffer: the row, two zero slots behind it (fragments outside the matrix; two
// because of the 16-byte window below), a length = 8 mod 32 (the four buffers then sit on disjoint quarter-banks for the
// write-out, which reads slot-fastest)
__host__ __device__ inline int p64_rowlen(int npairs) {
    int r = npairs + 4;
    r += (8 - (r & 31) + 32) & 31;
    return r;
}
// ... and the LDS of pt64_kernel and y2_64_kernel: C, the fragment table, four such buffers
inline size_t pair64_lds_bytes(int n) { return sizeof(double) * (4096 + 2048 + (size_t)4 * p64_rowlen(n * (n + 1) / 2)); }

// ---- one pair step
enum PairKernel {
    kPairUnsupported,   // no kernel takes the shape: the launcher's error
    kPt,                // pt_kernel<NPAD, ROWBUF>       phase-alternating, every form of the step, n <= 32
    kPtPipe,            // pt_pipe_kernel<NPAD, MODE>    the symmetric step, software-pipelined, two workgroups per CU
    kPtPipe4,           // pt_pipe4_kernel<NPAD, MODE>   ... tiles of 4 pairs, a few geometries
    kPtd,               // ptd_kernel<MODE>              ... operand rows by LDS-DMA, 16 < n <= 30, two workgroups per CU
    kPtdDot,            // ptd_kernel<0, 1>              ... the int2e_ip1 dot in the place of the write-out
    kPt64,              // pt64_kernel                   the symmetric step, 32 < n <= 64 (t[0]: MODE, a run-time branch)
};
struct PairPlan {
    PairKernel kernel;
    int t[2];           // the kernel's template arguments, in the order above
    int tiles_per_wg;   // -> PairTransformArgs::tiles_per_wg
    unsigned grid_x;    // (grid.y = geometries, 256 threads)
    size_t lds;         // dynamic LDS bytes
};
// The kernel name of a plan as the stage record keeps it.  A thread's ONE buffer, valid until its next call: two calls in
// one expression return the same pointer (comparing two names needs a copy of the first).
inline const char *pair_plan_name(const PairPlan &p) {
    static thread_local char buf[48];
    static const char *const fmt[] = {"", "pt_kernel<%d,%d>", "pt_pipe_kernel<%d,%d>", "pt_pipe4_kernel<%d,%d>", "ptd_kernel<%d>",
                                      "ptd_kernel<0> +ip1", "pt64_kernel<%d>"};
    snprintf(buf, sizeof(buf), fmt[p.kernel], p.t[0], p.t[1]);
    return buf;
}

// The fully symmetric step of the compressed layout's pipeline (dense (pair, pair) operand, lower triangles only) ...
inline bool pair_step_symmetric(const PairTransformArgs &a) { return a.lead_sym && a.in_lower && a.rs_lower && a.in_pairs; }
// ... and what it writes: 0 = the dense (pair, pair) result, 1 = the 8-fold compressed packed vector, -1 = another form
inline int pair_step_mode(const PairTransformArgs &a) {
    return a.k3 ? -1 : (a.out && a.out_pairs && !a.packed) ? 0 : (a.packed && a.sym8 && !a.out) ? 1 : -1;
}
// 8-pair tiles per workgroup of the kernels that put ONE workgroup on a CU (y2d_kernel<1>, ptd_kernel<0, 1>): a batch that
// fills the chip takes 8 (N = 30, 32 geometries: 256 workgroups), smaller ones fewer for more workgroups
inline int pairstep_tiles(int count) { return count >= 32 ? 8 : count >= 8 ? 4 : 2; }

inline PairPlan plan_pair_step(const PairTransformArgs &a, int count, const PairKnobs &knobs) {
    const int n = a.n, npairs = n * (n + 1) / 2, npad = (n + 15) / 16 * 16, ntq = (n + 7) / 8;
    const int mode = pair_step_symmetric(a) ? pair_step_mode(a) : -1;   // >= 0: the symmetric kernels take the step
    PairPlan p{kPairUnsupported, {0, 0}, 0, 0, 0};
    auto take = [&p](PairKernel kernel, int t0, int t1, int tiles_per_wg, int ntiles, size_t lds) {
        p = PairPlan{kernel, {t0, t1}, tiles_per_wg, (unsigned)((ntiles + tiles_per_wg - 1) / tiles_per_wg), lds};
        return p;
    };
    if (n < 1 || n > 64) return p;
    if (n > kPairTransformMaxN) {   // 32 < n <= 64: the symmetric step alone exists
        if (mode < 0) return p;
        // tiles of 4 pairs, one resident round of the chip (one workgroup per CU)
        const int ntiles = (npairs + 3) / 4, tpw = (int)ceil_div((int64_t)ntiles * count, (int64_t)250);
        return take(kPt64, mode, 0, tpw < 1 ? 1 : tpw, ntiles, pair64_lds_bytes(n));
    }
    // tiles of 8: 4 per workgroup (2/3/5/8 measured slower, with pt_pipe_kernel and again with ptd_kernel); a few
    // geometries: one, so that there are enough workgroups for the chip
    const int tpw = count < 4 ? 1 : (ntq < 4 ? ntq : 4), ntiles_sym = (npairs + 7) / 8;
    if (knobs.pt_dma && n > 16 && n <= kPdMaxN && count >= 4 && mode >= 0 && (a.in_ld == 0 || a.in_ld >= npairs) &&
        (mode == 1 || (a.out_ld >= 8 * ntiles_sym && a.out_ld % 2 == 0)))
        return take(kPtd, mode, 0, tpw, ntiles_sym, mode ? kPdLds1 : kPdLds);
    if (knobs.pt_pipe && mode >= 0) {
        if (count < 4 && npairs >= 8)   // tiles of 4 pairs, one per workgroup (twice the workgroups, half the length)
            return take(kPtPipe4, npad, mode, 1, (npairs + 3) / 4, sizeof(double) * ((size_t)4 * kPtRowLen + npairs * 8 + 8));
        const size_t lds = sizeof(double) * ((size_t)4 * kPtRowLen + (size_t)npairs * 16 + 16);
        if (lds <= 80 * 1024) return take(kPtPipe, npad, mode, tpw, ntiles_sym, lds);   // two workgroups fit a CU: n <= 30
    }
    // dense (pair, pair) operand: coalesced row fetch through a wave-private LDS row (ROWBUF), else a gather
    const size_t stage_rows = a.rs_lower ? (size_t)npairs : (size_t)n * n, rowbuf = a.in_pairs ? (size_t)4 * kPtRowLen + 2 : 0;
    return take(kPt, npad, a.in_pairs ? 1 : 0, tpw, a.lead_sym ? ntiles_sym : n * ntq,
                sizeof(double) * ((npad == 16 ? (size_t)16 * 16 : (size_t)32 * 48) + stage_rows * 9 + rowbuf));
}
// the second gradient-side step (a plan of ptd_kernel<0>) with the int2e_ip1 dot: one workgroup per CU
inline PairPlan plan_pair_step_dot(int n, int count) {
    const int tiles = pairstep_tiles(count), ntiles = (n * (n + 1) / 2 + 7) / 8;
    return PairPlan{kPtdDot, {0, 1}, tiles, (unsigned)((ntiles + tiles - 1) / tiles), kPdLdsDot};
}

// ---- the Y2 contraction
// slabs the partial buffer of the pipeline is sized for (carve): the pair kernels use up to that many workgroups;
// beyond 32 orbitals y2_64_kernel deals the pairs of ONE geometry to a full round of the chip
inline int y2_slab_capacity(int n) { return n > kPairTransformMaxN ? 256 : 128; }

enum Y2Kernel {
    kY2Unsupported,
    kY2GsT,        // y2_kernel<NT>           GsT (n^3, n) and K3
    kY2Sb,         // y2_sb_kernel<NT>        the row-major SB and K3
    kY2Fused,      // y2_fused_kernel<NPAD>   the dense (pair, pair) SB and M1, n <= 32
    kY2d,          // y2d_kernel<0>           ... both rows by LDS-DMA, 16 < n <= 30
    kY2dPairstep,  // y2d_kernel<1>           ... inside the first gradient-side pair step
    kY2Wide,       // y2_64_kernel            ... 32 < n <= 64
};
enum Y2Operands { kY2FromGsT, kY2FromSb, kY2FromPairs };
struct Y2Plan {
    Y2Kernel kernel;
    int t;               // the template argument
    int slabs;           // = grid.x: partial (n, n) matrices per geometry, what the gradient tail sums (Ip1Args::nslab)
    unsigned grid_z;     // (grid.y = geometries, 256 threads)
    int tiles_per_wg;    // pair kernels: tiles per workgroup ...
    int ppt;             // ... of this many pairs (y2_64_kernel: pairs per workgroup)
    size_t lds;          // dynamic LDS bytes
};
// (a thread's one buffer, as pair_plan_name)
inline const char *y2_plan_name(const Y2Plan &p) {
    static thread_local char buf[48];
    static const char *const fmt[] = {"", "y2_kernel<%d>", "y2_sb_kernel<%d>", "y2_fused_kernel<%d>", "y2d_kernel",
                                      "y2d_kernel<1> pairstep", "y2_64_kernel"};
    snprintf(buf, sizeof(buf), fmt[p.kernel], p.t);
    return buf;
}
inline Y2Plan plan_y2(Y2Operands from, int n, int count, const PairKnobs &knobs) {
    const int nt = (n + 15) / 16, npairs = n * (n + 1) / 2, cap = y2_slab_capacity(n);
    if (from != kY2FromPairs) {   // n > 64: four 64 x 64 quadrants
        if (nt < 1 || nt > 8) return Y2Plan{kY2Unsupported, 0, 0, 0, 0, 0, 0};
        return Y2Plan{from == kY2FromGsT ? kY2GsT : kY2Sb, nt > 4 ? 4 : nt, kY2Slabs, nt > 4 ? 4u : 1u, 0, 0, 0};
    }
    if (n < 1 || n > 64) return Y2Plan{kY2Unsupported, 0, 0, 0, 0, 0, 0};
    if (n > kPairTransformMaxN) {
        // one resident round of the chip, never more slabs than the partial buffer holds
        int wgs = count >= 250 ? 1 : 250 / count;
        if (wgs > cap) wgs = cap;
        if (wgs > npairs) wgs = npairs;
        const int ppw = (npairs + wgs - 1) / wgs, slabs = (npairs + ppw - 1) / ppw;
        return Y2Plan{kY2Wide, 0, slabs, 1, 1, (npairs + slabs - 1) / slabs, pair64_lds_bytes(n)};
    }
    // tiles of 8 pairs, 4 per workgroup, for batches (as the pair transform); tiles of 4 (one matrix per wave), one per
    // workgroup, for a few geometries (enough workgroups for the chip); never more workgroups than the buffer has slabs
    const int ppt = count < 4 ? 4 : 8, ntiles = (npairs + ppt - 1) / ppt;
    int t = count < 4 ? 1 : 4;
    while ((ntiles + t - 1) / t > cap) ++t;
    const int slabs = (ntiles + t - 1) / t, npad = nt * 16;
    constexpr size_t red32 = sizeof(double) * 4 * 32 * 33, rows = sizeof(double) * (size_t)8 * kPtRowLen;
    if (knobs.pt_dma && n > 16 && n <= kPdMaxN) return Y2Plan{kY2d, 0, slabs, 1, t, ppt, 8 * kPdRB > red32 ? 8 * kPdRB : red32};
    const size_t red = sizeof(double) * 4 * npad * (npad + 1);
    return Y2Plan{kY2Fused, npad, slabs, 1, t, ppt, rows > red ? rows : red};
}
inline Y2Plan plan_y2_pairstep(int n, int count) {
    const int tiles = pairstep_tiles(count), ntiles = (n * (n + 1) / 2 + 7) / 8;
    return Y2Plan{kY2dPairstep, 1, (ntiles + tiles - 1) / tiles, 1, tiles, 8, kPdLdsY};
}

// ---- the gradient side of the symmetric pipeline: Y2, then two pair steps B1 -> B2 -> B1
// the second step's arguments from the first's: it reads what the first wrote and writes `out`
// (it keeps rs_lower as well: G^AO[m,b,c,d] = G^AO[b,m,c,d], fold_cd reads b <= m; the result is only valid for d <= c)
inline PairTransformArgs grad_second_args(PairTransformArgs pa, double *out, int out_pairs) {
    pa.in = pa.out;
    pa.out = out;
    pa.in_pairs = pa.out_pairs;
    pa.out_pairs = out_pairs;
    return pa;
}
struct GradPairPlan {
    bool y2_in_first;     // y2d_kernel<1> is the Y2 contraction AND the first step: `first` is not launched
    bool dot_in_second;   // ptd_kernel<0, 1>: the pair blocks of the packed int2e_ip1 contraction in the place of the second
                          // step's write-out (nothing but that dot reads B1 behind the step, so B1 stays unwritten)
    Y2Plan y2;
    PairPlan first, second;
    PairTransformArgs first_args, second_args;   // what the two steps are launched with (tiles_per_wg: the launchers)
    int nslab() const { return y2.slabs; }   // slabs of y2part the launched Y2 kernel writes
};
// first: the first step on the dense (pair, pair) SB (in_pairs = 1); with G and n <= 32 it is launched on the N^4-addressed
// SB instead (first_args).  second_out: where the second step writes.  M1 (geometry stride sM1, pitch first.in_ld): the energy phase's intermediate the Y2 kernels read.  one_slot:
// one slot per geometry (the multi-slot roots form reads the int2e_ip1 rows once for several slots: ip1_dh_kernel keeps it).
inline GradPairPlan plan_grad_pairs(const PairTransformArgs &first, double *second_out, const double *M1, int64_t sM1,
                                    int count, bool want_G, bool wide, int ip1_s2kl, bool one_slot, const PairKnobs &knobs) {
    GradPairPlan g;
    const int n = first.n;
    const PairPlan dense = plan_pair_step(first, count, knobs);
    const Y2Plan ps = plan_y2_pairstep(n, count);
    // (both rows of a pair share one DMA window: rows on 16-byte granules, same pitch)
    const bool aligned = ((reinterpret_cast<uintptr_t>(first.in) | reinterpret_cast<uintptr_t>(M1)) & 15) == 0 &&
                         first.in_ld >= n * (n + 1) / 2 && first.in_ld % 2 == 0 && first.sin % 2 == 0 && sM1 % 2 == 0;
    g.y2_in_first = knobs.y2_pairstep && dense.kernel == kPtd && dense.t[0] == 0 && first.ct == 1 && aligned &&
                    first.in != first.out && ps.slabs <= y2_slab_capacity(n);
    g.y2 = g.y2_in_first ? ps : plan_y2(kY2FromPairs, n, count, knobs);
    g.first_args = first;
    g.first_args.in_pairs = (!want_G || wide) ? 1 : 0;
    g.first = plan_pair_step(g.first_args, count, knobs);
    g.second_args = grad_second_args(g.first_args, second_out, ip1_s2kl ? 1 : 0);
    g.second = plan_pair_step(g.second_args, count, knobs);
    g.dot_in_second = ip1_s2kl && !want_G && !wide && one_slot && knobs.ip1_pairstep && g.second.kernel == kPtd && g.second.t[0] == 0;
    if (g.dot_in_second) g.second = plan_pair_step_dot(n, count);
    return g;
}

// ---- the launchers: exactly the instantiation of the plan
int launch_pair_transform(const PairPlan &p, PairTransformArgs a, int count, hipStream_t st);
// (callers with no reason to look at the plan)
inline int launch_pair_transform(const PairTransformArgs &a, int count, hipStream_t st) {
    return launch_pair_transform(plan_pair_step(a, count, pair_knobs()), a, count, st);
}
int launch_pair_transform_pipe(const PairPlan &p, const PairTransformArgs &a, dim3 grid, hipStream_t st);   // pair_pipe.hip
int launch_pair_transform_dma(const PairPlan &p, const PairTransformArgs &a, int count, hipStream_t st);   // pair_dma.hip
int launch_pair_transform64(const PairPlan &p, const PairTransformArgs &a, int count, hipStream_t st);     // pair64.hip
// the dense step does not write `out` but contracts its result with the packed int2e_ip1 as the pair blocks of
// ip1_dh_kernel do (Ip1Args, ip1_s2kl)
int launch_pair_transform_dot(const PairPlan &p, const PairTransformArgs &a, const PairDotArgs &dt, int count, hipStream_t st);
// Y2 without K3 (symmetric pipeline): the half-transformed integrals are recomputed from the dense (pair, pair)
// intermediate `M1` of the first pair step (kept by the energy phase) inside the contraction,
//   Y2[i][a] = sum_v mult(v) sum_j SB[v][tri(i,j)] (M1_v X)[a][j];
// writes p.slabs partial (n, n) matrices per geometry; SB and M1 at the pitch pair_ld(n)
int launch_y2_fused(const Y2Plan &p, const double *SB, const double *M1, const double *X, int64_t sX, int n, double *partial,
                    int64_t sws, int count, hipStream_t st);
// ... the launchers of its kernel families in pair_dma.hip (y2d_kernel<0>) and pair64.hip (y2_64_kernel)
int launch_y2_dma(const Y2Plan &p, const double *SB, const double *M1, const double *X, int64_t sX, int n, double *partial,
                  int64_t sws, int count, hipStream_t st);
int launch_y2_64(const Y2Plan &p, const double *SB, const double *M1, const double *X, int64_t sX, int n, double *partial,
                 int64_t sws, int count, hipStream_t st);
// Y2 inside the first gradient-side pair step (y2d_kernel<1>): the launch `a` describes (dense (pair, pair) SB in, ct = 1,
// R out as ptd_kernel<0> writes it) and, from the H = SB_v X it forms, Y2 with M1 (pitch a.in_ld, geometry stride sws)
int launch_y2_pairstep(const Y2Plan &p, const PairTransformArgs &a, const double *M1, double *partial, int64_t sws, int count,
                       hipStream_t st);

}  // namespace evc
