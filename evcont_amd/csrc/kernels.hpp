// Internal launch interfaces shared by the translation units of libevcont_hip.so.
//
// Batching: every kernel of the per-geometry pipeline carries a batch index (blockIdx.y for the
// multi-workgroup kernels, blockIdx.x for the single-workgroup ones).  A pointer `p` that belongs
// to geometry 0 is paired with a stride `sp` in doubles; geometry g uses p + g*sp.  Workspace
// buffers all share one stride (the per-geometry workspace size), inputs/outputs have their own.
#pragma once
#include <vector>

#include "common.hpp"
#include "route.hpp"

namespace evc {

constexpr int kMaxOrbitals = 96;   // N of the fused pipeline (quarter transforms: 16-wide tiles up to 96 padded columns)
constexpr int kMaxBatchG = 32;  // geometries contracted per pass of the streaming kernels (matrix-core variants)

// ---- fci.hip, fci_solve.hip, fci_pack.hip ----------------------------------------------------------
constexpr int kFciMaxOrb = 16;
constexpr int kFciMinRows = 256;     // determinants per split-K block, at least
constexpr int kFciMaxBlocks = 256;   // split-K blocks (= partial tiles per ket), at most
// The split of the determinants into blocks depends on the determinant count alone -- not on the workspace, not on the
// number of kets or vectors -- so a row call and its single-pair calls, and a dot product in any grouping, sum the same
// partials in the same order.
inline int64_t fci_rows_per_block(int64_t dim) {
    const int64_t r = (int64_t)align_up((size_t)ceil_div(dim, kFciMaxBlocks), 64);
    return r < kFciMinRows ? kFciMinRows : r;
}

// fci_pack.hip: the dense dm2 (norb^4) of one ket -> one row of the evaluator's (pairs, ld) matrix in EVC_LAYOUT_PACK2 or
// EVC_LAYOUT_SYM8 (fci_row_pack_cols columns, the rest of the row up to ld zero); note_fci_row_pack: the stage record
int64_t fci_row_pack_cols(int layout, int norb);
int launch_fci_row_pack(int layout, int norb, const double *dm2, double *row, int64_t ld, hipStream_t st);
void note_fci_row_pack(int layout, int norb, int nrows, int64_t ld);

// ---- K5 / K8, the streaming t-RDM contractions: kernels in gemv_stream.hip (VALU), gemv_mfma.hip (matrix cores,
//      fragment-shaped loads), gemv_lds.hip / gemv_cols_lds.hip (matrix cores, K5 / K8 LDS-staged); gemv_dispatch.hip
//      plans the passes of a call
struct RowProblem {
    const double *A;   // (rows, ld)                       shared by the batch
    const double *v;   // (cols)            + g*vstride
    double *partial;   // (nspans, rows)    + g*pstride
    int64_t rows, cols, ld, vstride, pstride;
    int nspans, nblocks;   // nblocks: != 0 = the launch carries this problem (the VALU launchers put their block count here)
    int64_t span_cols;  // columns per span (a multiple of 32; the last span may be shorter): span s = [s, s+1) * span_cols
    int reserved;       // (the kernels take two of these by value: the size of the struct is part of their argument layout)
};
struct GemvRowsLaunch {
    RowProblem p[2];
    int nblk0;
    int nblk1;  // matrix-core variant: blocks of p[1] (padded to a multiple of 8), dispatched first
    // matrix-core variant: the 16-row tiles of p[k] are dealt to nrg[k] balanced row groups, the first
    // trem[k] of which have tpg[k] + 1 tiles and the others tpg[k]
    int tpg[2], trem[2], nrg[2];
};
struct ColProblem {
    const double *A;  // (rows, ld)                        shared by the batch
    const double *w;  // (rows)             + g*wstride
    const double *wt; // (rows, kMaxBatchG) + (g - g % kMaxBatchG)*wstride: the same weights of a group of geometries,
                      // transposed (geometry g in column g % kMaxBatchG), or NULL
    double *out;      // (cols)             + g*ostride
    int64_t rows, cols, ld, wstride, ostride;
    double *part;     // (kColSlabs, ld) + g*pstride or NULL: scratch for the row-slab form of a NARROW problem with many
    int64_t pstride;  // rows (the one-body t-RDM of a large training set: T^2 rows of N^2 columns)
};
constexpr int kColSlabs = 64;   // row slabs of that form
struct GemvColsLaunch {
    ColProblem p[2];
    int nblk0;
};

// One pass over the matrices: geometries [g0, g0 + G) through one kernel instantiation.
enum GemvKernel {
    kRowsValu,       // gemv_rows_kernel<RB, G>                          lane-private accumulators, G = 1, 2
    kRowsWaveRows,   // gemv_rows_wr_kernel<RBW, G, SUB>                 a wave per row set, G = 4, 8
    kRowsMfma,       // gemv_rows_mfma_pipe_kernel<GS, MAXT, MINW, PIPE> fragment-shaped loads, G = 12 .. 32
    kRowsLds,        // gemv_rows_lds_kernel<GS, NT, NCH>                LDS-staged, G = 12 .. 64
    kColsValu,       // gemv_cols_kernel<G>                              column tiles, G = 1, 2, 4, 8
    kColsValuRs,     // gemv_cols_rs_kernel<G>                           ... the rows split over the waves (narrow matrices)
    kColsSlab,       // gemv_cols_slab_kernel + its reduce               the small problem in row slabs, all geometries
    kColsMfma,       // gemv_cols_mfma_kernel<CT, KSN, MINW, GS>         G = 12 .. 32
    kColsMfmaRs,     // gemv_cols_mfma_rs_kernel<KSN, MINW, GS>          ... narrow matrices
    kColsLds,        // gemv_cols_lds_kernel<GS, D0, D1, NW>             LDS-staged, all weights in LDS, G = 17 .. 32
    kColsLdsSlab,    // gemv_cols_lds_slab_kernel<GS, NTW>               ... tall matrices, the weights in slabs
};
struct GemvPass {
    int g0, G;
    GemvKernel kernel;
    int t[4];      // the kernel's template parameters, in the order above
    int slot[2];   // the problem (0: large / two-body, 1: small / one-body) in slot k of the launch, -1: empty.  A tall
                   // one-body problem in a launch of its own is a second pass with the same g0 and G.
};
// The kernel name of a pass as the stage record keeps it (evc_profile_kernel) and evc_trdm_plan_describe prints it
// (a thread's buffer: valid until its next call).
const char *gemv_pass_name(const GemvPass &ps);

struct GemvShape {
    int64_t rows, cols, ld;   // rows <= 0: the call has no such problem
};
inline GemvShape gemv_shape(const RowProblem &P) { return {P.rows, P.cols, P.ld}; }
struct GemvKnobs {       // read once per process (gemv_knobs)
    bool rows_lds;         // EVC_ROWS_LDS (default 1): the LDS-staged K5 kernel
    bool cols_lds;         // EVC_COLS_LDS (default 1): the LDS-staged K8 kernels
    int rows_lds_nt;       // EVC_ROWS_LDS_NT: forces the K5 kernel's tiles per row group (14, 7, 4, 2)
    int64_t lds_min_cols;  // EVC_ROWS_LDS_MINCOLS (default 4096): narrower matrices stay with the fragment-shaped kernels
                           // (nothing to stream); 1 sends the small shapes of the parity tests through the LDS kernels
};
const GemvKnobs &gemv_knobs();
// CUs of the current device (0: unknown), the one place that asks HIP.  The LDS-staged kernels put one workgroup on a CU
// and size their grids for a whole MI355X, kLdsBlocks + kLdsBlocksSmall workgroups in one round: a device (or partition)
// with fewer CUs keeps the kernels of gemv_mfma.hip.
int lds_device_cus();
constexpr int kLdsBlocks = 242;      // workgroups of the large problem: one per CU (the images fill the LDS), one round
constexpr int kLdsBlocksSmall = 8;   // ... of the small (one-body) problem
constexpr int kLdsChunkCols = 16;    // columns per wave chunk of the LDS-staged K5 kernel (a span: a multiple of 4 chunks)
constexpr int kMfmaMinG = 12;        // groups of >= this many geometries use the matrix cores

// The K5 plan of a call: pure functions of the shapes, the batch size, the CU count and the knobs.
struct GemvSpans {
    int64_t span_cols;
    int nspans;
};
struct RowsPlan {
    GemvSpans spans[2];   // span decomposition of the two problems (-> layout of the partials)
    std::vector<GemvPass> passes;
    void apply(RowProblem &p0, RowProblem &p1) const;   // span_cols, nspans; nblocks != 0 iff the call has the problem
};
RowsPlan plan_gemv_rows(const GemvShape &p0, const GemvShape &p1, int count, int device_cus, const GemvKnobs &knobs);
// ... and the K8 plan; wt / part: the call brings the transposed weights / the slab scratch of the small problem
std::vector<GemvPass> plan_gemv_cols(const GemvShape &p0, const GemvShape &p1, int count, bool wt, bool part,
                                     int device_cus, const GemvKnobs &knobs);
// most spans any plan makes of a problem, on any device with any knobs (the partial buffers are carved for it)
int rows_max_spans(const GemvShape &P, bool small);
size_t rows_ws_doubles(int64_t rows, int64_t cols);
// `count` geometries in the passes of the plan.  PRECONDITION of launch_gemv_rows: span_cols / nspans of p0, p1 are those
// of plan_gemv_rows for the same shapes and `count` on this device (RowsPlan::apply: workspace.hip setup, evc_gemv_rows)
// -- the kernels write, and the consumer sums, the spans the caller names; a problem with nblocks == 0 is left out.
int launch_gemv_rows(RowProblem p0, RowProblem p1, int count, hipStream_t st);
int launch_gemv_cols(ColProblem p0, ColProblem p1, int count, hipStream_t st);
// One launcher per kernel family, in the order of GemvKernel: exactly the instantiation ps.t for the geometries of the
// pass (the plan names only instantiations that exist).
using RowsLauncher = int(GemvRowsLaunch L, const GemvPass &ps, hipStream_t st);
using ColsLauncher = int(GemvColsLaunch L, const GemvPass &ps, hipStream_t st);
RowsLauncher launch_rows_valu, launch_rows_wave_rows, launch_rows_mfma, launch_rows_lds;
ColsLauncher launch_cols_valu, launch_cols_valu_rs, launch_cols_slab, launch_cols_mfma, launch_cols_mfma_rs, launch_cols_lds,
    launch_cols_lds_slab;
int launch_rows_reduce(const double *partial, int64_t rows, int nspans, double alpha, double *y, hipStream_t st);

// ---- quarter.hip, pair_transform.hip, pack.hip, y2.hip, ip1.hip ----------------------
int launch_quarter_transform(const double *in, int64_t sin, const double *C, int64_t sC, int c_transposed, int n,
                             double *out, int64_t sout, int count, hipStream_t st);
// Two quarter steps fused (n <= 32): out[r'][s'][p][q] = sum_rs in[p][q][r][s] C[r][r'] C[s][s'].
struct PairTransformArgs {
    const double *in;   // (n^4)   + g*sin
    const double *C;    // (n,n)   + g*sC
    double *out;        // (n^4) full result or NULL                          + g*sout
    double *packed;     // packed lower triangle (diag * diag_mult) or NULL   + g*spacked
    double *k3;         // half result K3[s'][p][q][r] = sum_s in[p][q][r][s] C[s][s'] or NULL  + g*sk3
    int64_t sin, sC, sout, spacked, sk3, packed_len;
    double diag_mult;
    int ct, n;
    int tiles_per_wg;   // set by the launchers from the plan (pair_plan.hpp): consecutive 8-wide q tiles per workgroup
    int sym8;           // `packed` is the 8-fold compressed vector (EVC_LAYOUT_SYM8), multiplicities folded in
    int lead_sym;       // in[p][q][..] = in[q][p][..]: only q <= p (whole 8-wide q tiles) is computed and stored
    int in_lower;       // in[p][q][r][s] = in[p][q][s][r] and only r >= s is valid (output of a lead_sym step)
    int rs_lower;       // only the rows (r',s'), s' <= r', of the result are needed (out rows / packed sym8 vector)
    int out_pairs;      // (with lead_sym and rs_lower) `out` is the dense (pair, pair) matrix out[tri(r',s')][tri(p,q)]
                        // instead of rows of an N^4 tensor (multiplicities are the consumers' business)
    int in_pairs;       // (with lead_sym) `in` is such a matrix: in[tri(p,q)][tri(r,s)]
    int in_ld, out_ld;  // row pitch (doubles) of the dense (pair, pair) operand / result; 0: n(n+1)/2 (the caller's s4 `int2e`);
                        // the pipeline's own intermediates use pair_ld(n): rows start on 128-byte lines
};
// what ptd_kernel<0, 1> contracts its result with (launch_pair_transform_dot, pair_plan.hpp)
struct PairDotArgs {
    const double *ip1;  // (3,n,n,n(n+1)/2)  + g*sip1
    double *t2part;     // (n,3,nchunk)      + g*st2
    int64_t sip1, st2;
    int nchunk;
};
// (pair_ld(n), the row pitch of the pipeline's dense (pair, pair) intermediates, and kPairTransformMaxN: route.hpp)
// one packed operand row of the pair kernels in LDS (pair_transform.hip pt_kernel, pair_pipe.hip, y2.hip y2_fused_kernel)
constexpr int kPtRawMax = (kPairTransformMaxN * (kPairTransformMaxN + 1) / 2 + 1 + 127) / 128;   // double2 per lane: 5
constexpr int kPtRowLen = kPtRawMax * 128 + 4;   // + two zero slots (padding fragments), 16-byte multiple
// (the plans of the pair steps and of Y2, and the launchers that take them: pair_plan.hpp)
int launch_pack(const double *h2, int64_t sh2, int n, double diag_mult, double *out, int64_t sout, int64_t out_len,
                int count, hipStream_t st);
// 8-fold compressed vector of a tensor with the index symmetries of real two-electron integrals:
//   out[tri(u,v)] = h2[i,j,k,l] * (u == v ? diag_mult : 1) * (i != j ? 2 : 1) * (k != l ? 2 : 1),
//   u = tri(i,j) (i >= j), v = tri(k,l) (k >= l), u >= v
int launch_pack_sym8(const double *h2, int64_t sh2, int n, double diag_mult, double *out, int64_t sout,
                     int64_t out_len, int count, hipStream_t st);
int launch_unpack(const double *packed, int64_t sp, int n, double *out, int64_t sout, int count, hipStream_t st);
// Gs^T[jkl][i] = G[i,j,k,l] + G[j,i,k,l] + G[l,k,j,i] + G[k,l,i,j]   (gradients_loewdin.py:213-215)
int launch_sym_oao_t(const double *G, int64_t sG, int n, double *out, int64_t sout, int count, hipStream_t st);
// Packed fast path: from the packed predicted 2-RDM p (pair symmetric by construction) write in one pass
//   GsT[jkl][i] = 2 p(ij,kl) + p(ji,kl) + p(ji,lk)        (= the OAO symmetrisation above, transposed)
//   SB[i,j,k,l] = 2 (p(ij,kl) + p(ji,lk))                  (= AO-type symmetrisation, gradients_loewdin.py:238-240,
//                                                             applied BEFORE the OAO->AO rotation, with which it commutes)
//   G[i,j,k,l]  = p(ij,kl)                                 (optional: the unpacked 2-RDM, eiu:69-88)
int launch_unpack_sym(const double *packed, int64_t sp, int n, double *GsT, double *SB, int64_t sws, double *G,
                      int64_t sG, int count, hipStream_t st);
// EVC_LAYOUT_SYM8: `packed` is the 8-fold compressed vector p8 of a fully symmetric 2-RDM:
//   SB[i,j,k,l] = 4 p8(ijkl) (only for i >= j, l <= k when lead_half = 1, which needs G; lead_half = 2: the dense
//   (pair, pair) matrix SB[tri(i,j)][tri(k,l)] instead), G[i,j,k,l] = p8(ijkl) (optional)
int launch_unpack8(const double *packed, int64_t sp, int n, double *SB, int64_t sws, double *G, int64_t sG, int count,
                   int lead_half, hipStream_t st);
// partial[b][i][a] = sum_{k in slab b} SB[i][k] * K3[k][a]: the Y2 contraction with the row-major operand
int launch_y2_sb(const double *SB, const double *K3, int n, double *partial, int64_t sws, int count, hipStream_t st);
// partial[b][i][a] = sum_{k in slab b} GsT[k][i] * K3[k][a]   (k = jkl)
constexpr int kY2Slabs = 64;   // K slabs of these two = partial results per geometry
inline int y2_slabs(int) { return kY2Slabs; }
int launch_y2(const double *GsT, const double *K3, int n, double *partial, int64_t sws, int count, hipStream_t st);
// ip1 contraction with on-the-fly AO symmetrisation (gradients_loewdin.py:234-252), dhcore:P_ao dots
// and the fixed-order sum of the Y2 slabs (three block families of one launch)
int ip1_chunks(int n);
// Geometry of slot g of a gradient launch: geo_period = 0 -> g (one slot per geometry); otherwise g % geo_period (the
// root-pair-major slots s = p * count + g of evc_phase_gradient_roots_batch, geo_period = count).  Applies to the
// caller's per-geometry inputs only (hcore, int2e_ip1, dhcore, ipovlp); the workspace is per slot.
__host__ __device__ inline int64_t geo_of(int64_t g, int geo_period) { return geo_period > 0 ? g % geo_period : g; }
struct Ip1Args {
    const double *ip1;     // (3,n^4)      + geo_of(g)*sip1
    const double *Gao;     // (n^4)        + g*sws
    double *t2part;        // (n,3,nchunk) + g*sws
    const double *dh;      // (A,3,n,n)    + geo_of(g)*sdh      (may be NULL with natm = 0)
    const double *Pao;     // (n,n)        + g*sws
    double *term3;         // (A*3)        + g*sws
    const double *y2part;  // (nslab,n,n)  + g*sws
    double *y2;            // (n,n)        + g*sws
    int64_t sip1, sdh, sws;
    int n, natm, nslab, nchunk;
    int presym;            // Gao already carries the 4-fold AO symmetrisation (packed fast path)
    int fold_cd;           // (with presym) Gao[m,b,c,d] is symmetric in c <-> d and in m <-> b and only valid for
                           // d <= c, b <= m
    int ip1_s2kl;          // (with fold_cd) ip1 is (3,n,n,n(n+1)/2): packed in its last two indices, c >= d
                           // (EVC_FLAG_IP1_S2KL); sip1 is the packed size and Gao the dense (pair, pair) matrix
                           // Gao[tri(m,b)][tri(c,d)] at the pitch pair_ld(n), WITHOUT the multiplicity of (c,d): the
                           // dot weighs it (2 for c != d)
    int geo_period;        // geo_of (0: slot g reads geometry g)
    int slots;             // (pair-block route, geo_period > 0) root-pair slots per geometry: the launch has
                           // geo_period * slots slots, and one block reads the int2e_ip1 rows of a geometry once for up
                           // to kIp1MaxSlots of its slots (launch_ip1_dh); 0 or 1: one slot per block
    int pairs_done;        // (pair-block route, one slot per block) the second gradient-side pair step has written the
                           // pair blocks' entries of t2part (ptd_kernel<0, 1>): the grid has none
};
constexpr int kIp1MaxSlots = 8;
int launch_ip1_dh(const Ip1Args &a, int count, hipStream_t st);

// ---- loewdin.hip (loewdin.hpp: the kernel body subspace_small.hip shares) -----------------------------
struct LoewdinArgs {
    const double *S, *h;   // + g*sS, + g*sh   (h may be NULL)
    double *X, *U, *s, *h1;  // + g*sws        (h1 may be NULL)
    int64_t sS, sh, sws;
    int n;
    int warm;  // U holds the eigenvectors of a previous, nearby S: start the Jacobi sweeps from them
    int fast;  // set by launch_loewdin: FP32 Jacobi + FP64 refinement for n <= 32 (EVC_EIGH_F32=0: FP64 Jacobi)
    double *scratch;   // n > 64: 2 Tp^2 doubles (Tp = n rounded up to 16) + g*sscratch for two of the three work matrices
    int64_t sscratch;  // (NULL: the LDS-only kernels, n <= 80)
    double *flag;      // + g*sws: one word per geometry (32 < n <= 64, part != 0): 1 = the Newton-Schulz launch wrote X, h1
    int part;          // 0: X, h1, U, s.  loewdin_split_available(n) only: 1 = X and h1 alone (Newton-Schulz on the matrix
                       // cores, no eigensolver; U and s are not touched), 2 = U and s alone (X, h1 are not touched) -- the
                       // two halves of a step whose gradient tail alone needs the eigendecomposition (side_stream.hip);
                       // 3 (internal, 32 < n <= 64): X and h1 by the eigensolver for the geometries whose flag is 0
};
int launch_loewdin(const LoewdinArgs &a, int count, hipStream_t st);
bool loewdin_split_available(int n);
// loewdin_big.hip: 32 < n <= 64 in LDS alone, 64 < n <= kMaxOrbitals with a.scratch
int launch_loewdin_big(const LoewdinArgs &a, int count, hipStream_t st);
// Host-side knobs, read once per process (loewdin.hip).  EVC_EIGH_F32: 0 = FP64 Jacobi, 1 = FP32 Jacobi + refinement,
// 2 (default) = FP32 tridiagonal start + refinement.  EVC_SUBSPACE_FEW (default 1): a few lowest roots through the
// tridiagonal route, in both subspace kernels.
int eigh_fast_enabled();
int subspace_few_enabled();

// ---- subspace_small.hip (T <= kSubspaceSmallT), subspace_big.hip (beyond; big_block.hpp, big_few_roots.hpp) ---
struct SolveArgs {
    const double *h1part;  // (nsp1, T*T) partial sums of the one-body rows      + g*sh1
    int nsp1;
    double alpha1;
    const double *h2part;  // (nsp2, rows2_total) partial sums of two-body rows  + g*sh2
    int nsp2;
    double alpha2;
    const double *S;  // (T,T) + g*sS  (sS = 0: one overlap matrix shared by the batch)
    int64_t sS;
    int T, layout, nroots;
    double e_shift;             // used when e_shift_dev == NULL
    const double *e_shift_dev;  // [count] or NULL
    double *evals, *evecs, *Hout;  // + g*sev, + g*svec, + g*sH  (Hout may be NULL)
    double *w2, *w1;               // + g*sw
    double *w2t;                   // (w2_count, kMaxBatchG) or NULL: w2 of the geometries of a group of kMaxBatchG,
                                   // transposed, in the workspace of the group's first geometry (+ (g - g%32)*sw)
    double *w1t;                   // (T*T, kMaxBatchG) or NULL: the same for w1
    int64_t sh1, sh2, sev, svec, sH, sw;
    int64_t w2_offset, w2_count;  // slice of the global weight vector to write (multi-GPU)
    double *vstd;                 // (m,m), m = T rounded up to even: standard-form eigenvectors, kept in the
                                  // workspace from call to call (+ g*sw); may be NULL
    int warm;                     // start the Jacobi sweeps from vstd
    int fast;                     // set by launch_subspace_solve: FP32 Jacobi + FP64 refinement for T <= 32
    double *bcache;               // (2, T, T) + g*sw or NULL: the lower triangle of the overlap matrix the cached
                                  // B = L^-1 (second block) was computed from -- S_train does not depend on the
                                  // geometry, so every call after the first finds its factorisation here
                                  // (T > kSubspaceSmallT: two blocks of Tp^2, Tp = T rounded up to 16, B at pitch Tp)
    int few;                      // set by launch_subspace_big: nroots <= 4 through the tridiagonal route (EVC_SUBSPACE_FEW)
    double *scratch;              // T > kSubspaceSmallT: subspace_big_scratch_doubles(T) doubles + g*sscratch
    int64_t sscratch;
};
constexpr int kSubspaceSmallT = 32;   // up to here: the register / 32 x 32-tile kernel of subspace_small.hip
constexpr int kSubspaceMaxT = 512;    // beyond kSubspaceSmallT: subspace_big.hip (LDS-resident up to 128, then global)
// subspace solve + the eigendecomposition half of the Loewdin step (part 2) in one launch (subspace_small.hip)
int launch_subspace_loewdin(const SolveArgs &s, const LoewdinArgs &l, int count, hipStream_t st);
int launch_subspace_solve(const SolveArgs &a, int count, hipStream_t st);
// subspace_big.hip: T > kSubspaceSmallT (vstd, when given, holds Tp^2 doubles: the eigenvectors as ROWS at pitch Tp)
size_t subspace_big_scratch_doubles(int T);
int launch_subspace_big(const SolveArgs &a, int count, hipStream_t st);

// ---- grad_tail.hip -------------------------------------------------------------------------------------
// The layout's two-body rows are the pairs a >= b of training states (T(T+1)/2 of them) instead of all T^2.
__host__ __device__ inline bool layout_pairs(int layout) {
    return layout == EVC_LAYOUT_PAIR5 || layout == EVC_LAYOUT_PACK2 || layout == EVC_LAYOUT_SYM8;
}
// Weights of the t-RDM rows for the predicted RDMs of a GIVEN coefficient vector c[T] (gradients_loewdin.py:343-356):
// w1[a*T+b] = c_a c_b; w2 = the slice [w2_offset, +w2_count) of the two-body row weights (pairs: 2 c_a c_b, c_a^2 on
// the diagonal; otherwise c_a c_b).
int launch_pair_weights(const double *c, int T, int layout, double *w1, double *w2, int64_t w2_offset,
                        int64_t w2_count, hipStream_t st);
// The same for the slots of the root pairs (evc_phase_gradient_roots*): slot s = p * geo_period + g (geo_period > 0;
// geo_period = 0: slot s = pair p = s) gets the weights of the symmetric weighting W = (c_k c_l^T + c_l c_k^T) / 2
// of the rows k = pairs[2p], l = pairs[2p+1] of the (nvec, T) block c + geo_of(s, geo_period) * sc -- c_k c_k^T for
// k == l --, w1 / w2 at + s*sw and, if w1t / w2t are given, the transposed group copies the batched K8 reads.
int launch_pair_weights_geo(const double *c, int64_t sc, int geo_period, int T, int layout, const int32_t *pairs,
                            int npairs, double *w1, double *w2, double *w1t, double *w2t, int64_t sw, int64_t w2_offset,
                            int64_t w2_count, hipStream_t st);
constexpr int kPairWeightsSlots = 256;   // slots per launch (their (k, l) travel in the kernel arguments)
struct PairWeightsArgs {
    const double *c;          // (nvec, T) rows  + geo_of(g, geo_period)*sc
    double *w1, *w2;          // + g*sw, g = slot0 + blockIdx.y
    double *w1t, *w2t;        // (rows, kMaxBatchG) + (g - g % kMaxBatchG)*sw, or NULL
    int64_t sw, w2_offset, w2_count, sc;
    int T, pairs, slot0, geo_period;
    int16_t k[kPairWeightsSlots], l[kPairWeightsSlots];
};
struct GradPrepArgs {
    int n;
    const double *X;      // + g*sws
    const double *hcore;  // + geo_of(g)*sh
    const double *D;      // predicted 1-RDM (n,n)  + g*sD
    double *Pao;          // X D X^T                + g*sws
    double *Y1;           // hcore X (D + D^T)      + g*sws
    int64_t sws, sh, sD;
    double scale1;        // 1 on the rank that owns the one-body part, else 0
    int geo_period;       // geo_of
};
int launch_grad_prep(const GradPrepArgs &a, int count, hipStream_t st);
// grad_prep and the unpack of the packed predicted 2-RDM into the dense (pair, pair) SB in ONE launch
int launch_unpack8_prep(const GradPrepArgs &a, const double *packed, int64_t sp, double *SB, int64_t sws, int count,
                        hipStream_t st);
struct GradFinalArgs {
    int n, natm;
    const double *U, *s;          // eigen-decomposition of S_AO   + g*sws
    const double *Y1;             // (n,n) [a][i]                  + g*sws
    const double *y2;             // (n,n) [i][a]                  + g*sws
    const double *ipovlp;         // (3,n,n)                       + geo_of(g)*sip
    const int64_t *aoslices;      // (A,2) shared
    const double *t2part;         // (n,3,nchunk)                  + g*sws
    int nchunk;
    const double *term3;          // (A*3)                         + g*sws
    const double *gnuc;           // (A,3) or NULL                 + g*sgn
    double scale1;                // 1: include term3 + gnuc
    double *grad;                 // (A,3)                         + g*sgrad
    int64_t sws, sip, sgn, sgrad;
    int geo_period;               // geo_of (gnuc is per slot)
};
int launch_grad_final(const GradFinalArgs &a, int count, hipStream_t st);

}  // namespace evc
