// What the files of the per-geometry orchestration share: the views of a call's inputs, outputs and workspace, the
// per-call state, the profiler hooks, the side-stream calls and the gradient chain.
//   profile.hip      error string, ABI version, stage records, event profiler, evc_profile_*
//   workspace.hip    set / geometry checks, the constructors of Geo / Out, carve, setup, the workspace byte counts
//   side_stream.hip  the Loewdin step in two halves: side stream, join, evc_release_workspace, loewdin_split_mode
//   pipeline.hip     the three phases, the gradient routes, the single / batch entry points
//   roots.hip        the multi-root gradient
//   standalone.hip   evc_subspace_solve[_batch], evc_integrals_oao_batch, evc_grad_elec_oao
#pragma once
#include <string.h>

#include "pair_plan.hpp"

namespace evc {

// ---- profile.hip ---------------------------------------------------------------------------------------------------
constexpr int kProfStages = 14;  // EVC_PROF_* of include/evcont_hip.h
// Entry points clear the records of the stages they can launch, so that a stage the call did not run reports "".
constexpr unsigned kStagesAll = (1u << kProfStages) - 1u;
constexpr unsigned kStagesHamiltonian =
    (1u << EVC_PROF_LOEWDIN) | (1u << EVC_PROF_PAIR_TRANSFORM) | (1u << EVC_PROF_ROWS) | (1u << EVC_PROF_UNPACK);
constexpr unsigned kStagesGradient = (1u << EVC_PROF_COLS) | (1u << EVC_PROF_UNPACK) | (1u << EVC_PROF_Y2) |
                                     (1u << EVC_PROF_PAIR_TRANSFORM) | (1u << EVC_PROF_IP1);
void clear_kernels(unsigned mask);
constexpr int kKernelRanLen = 96;
const char *kernel_ran(int stage);   // the stage's record (note_kernel)
// start of a timed launch: returns the record index or -1 (stage < 0: not timed)
int prof_start(int stage, hipStream_t st);
void prof_stop(int i, hipStream_t st);
// a launch timed as `stage`; its error returns from the calling function
#define EVC_TIMED(stage, st, call)                \
    do {                                          \
        const int pr_ = prof_start(stage, st);    \
        if (int rc_ = (call)) return rc_;         \
        prof_stop(pr_, st);                       \
    } while (0)

// ---- workspace.hip -------------------------------------------------------------------------------------------------
// Internal batch view of the geometry inputs / outputs (strides in doubles; 0 for a single geometry).
struct Geo {
    int natm, count;
    const double *S, *hcore, *eri, *ipovlp, *dhcore, *eri_ip1, *gnuc;
    const int64_t *aoslices;
    int64_t sS, sh, seri, sip, sdh, sip1, sgn;
    double enuc;             // used when enuc_dev == NULL
    const double *enuc_dev;  // [count]
    int batch;               // built by geo_batch: enuc and gnuc are device arrays, both required (check_geometry)
    int eri_s4;              // eri is the dense (pair, pair) matrix (EVC_FLAG_ERI_S4); set from the call's flags (setup)
    int geo_period;          // gradient chain: slot g reads geometry geo_of(g, geo_period) (kernels.hpp; 0: g)
};
struct Out {
    double *energy, *coeffs, *grad, *d_pred, *g_pred, *hmat;
    int64_t se, sc, sg, sd, sG, sH;
};

// The carving of one geometry slot: a pure function of the set, natm and the base pointer (carve).
struct Ws {
    // N^2-sized
    double *X, *U, *s, *h1, *Dpred, *Pao, *Y1;
    double *lflag;   // one word: the Newton-Schulz launch of a split Loewdin step delivered (32 < n <= 64)
    // N^4-sized
    double *B1, *B2, *K3, *G;
    double *vec2;  // ld2-long vector: packed h2 (phase A) / packed predicted 2-RDM (phase C)
    // t-RDM contraction
    double *h2part, *h1part, *h2rows, *w2, *w1, *w2t, *w1t;
    double *d1part;   // row-slab partials of the predicted 1-RDM (large training sets: gemv_cols_slab_kernel)
    // gradient partials
    double *y2part, *y2, *t2part, *term3;
    // scratch outputs when the caller passes NULL
    double *evals, *evecs;
    // eigenvectors kept from call to call for EVC_FLAG_WARM_START (U above serves the Loewdin step)
    double *vstd;
    double *bcache;   // (2, T, T): overlap matrix (lower triangle) and the inverse Cholesky factor computed from it
    double *sbig;     // T > kSubspaceSmallT: scratch of the large-T subspace kernel (subspace_big.hip)
    void *base;       // the caller's workspace pointer (key of its side stream, side_of)
    size_t bytes;     // of ONE geometry
    int64_t stride;   // the same in doubles
};
Ws carve(const evc_trdm_set *t, int natm, char *base);

// The state of one call (setup): the workspace, the flags that configure it, the span plan and the routes.
struct Call {
    Ws w;
    bool warm;
    bool loewdin_done;   // X, U, s, h1 are already in the workspace (EVC_FLAG_LOEWDIN_DONE)
    int split;           // Loewdin step of this call: 0 = one kernel; 1 = X, h1 by Newton-Schulz on the call's stream and
                         // U, s by the eigensolver on the device's side stream, joined in front of launch_grad_final;
                         // 3 = the same with the eigensolver riding in the launch of the subspace solve (la_ride)
    LoewdinArgs la_ride; // split == 3: the eigensolver launch phase_solve still owes
    RowProblem rp2, rp1; // shapes and the span plan of this call (never more spans than the buffers were carved for)
    Route eri, ip1;      // route of the energy phase (EVC_FLAG_ERI_S4) and of the gradient phase (EVC_FLAG_IP1_S2KL)
};

int check_set(const evc_trdm_set *t);
// A batch needs enuc and gnuc as device arrays; one geometry takes enuc by value and gnuc is optional (NULL: no
// nuclear term).
int check_geometry(const char *who, const Geo &g, bool need_grad);
// The two constructors of Geo.  One geometry: count = 1, every stride 0, enuc by value, geo_period 0 (to the chain the
// slot is a geometry of its own).  They and those of Out are called before any check: a NULL descriptor gives
// count = 0, which check_geometry reports (a NULL set: check_set).
Geo geo_single(const evc_geometry *g);
// count geometries of t->n orbitals, each at its own stride (geo_period 0: slot g reads geometry g), enuc on the device
Geo geo_batch(const evc_trdm_set *t, const evc_geometry_batch *gb);
// The two constructors of Out: one geometry (strides 0), count geometries each at its own stride.
Out out_single(const evc_outputs *o);
Out out_batch(const evc_trdm_set *t, const evc_geometry_batch *gb, const evc_outputs_batch *ob);
// The set-up every entry point that works in a caller's workspace of `slots` geometry slots goes through (t checked by
// the caller, check_set): the workspace checks, its carving, the span plan and the routes of the call, and the call's
// flags that configure the two views -- each decoded here and nowhere else.
int setup(const char *who, const evc_trdm_set *t, Geo &g, int flags, void *ws, size_t ws_bytes, int slots, Call &c);
// The Loewdin step of the geometries g into the workspace slots (part 0: everything in one launch).
LoewdinArgs loewdin_args(int n, const Geo &g, const Call &c);

// ---- side_stream.hip -----------------------------------------------------------------------------------------------
// The eigensolver half of a split Loewdin step (la.part = 2) on the device's side stream, forked from st; the workspace's
// next side_join waits for it.
int side_launch_loewdin(void *ws, const LoewdinArgs &la, int count, hipStream_t st);
// The join: whoever reads U and s of a workspace next (launch_grad_final -- in the same call or, after an energy-only
// call, in a later evc_phase_gradient, evc_phase_loewdin_batch or Loewdin launch on the same workspace) waits for the
// eigensolver launch that writes them.
int side_join(void *ws, hipStream_t st);
// which form the Loewdin step of a FULL call (evc_energy_with_grad[_batch]) takes
int loewdin_split_mode(int n, int ntrain, int count, bool loewdin_done, bool warm, hipStream_t st);

// ---- pipeline.hip --------------------------------------------------------------------------------------------------
// The plain four-index rotation with C (ct: over its second index): in -> ping -> pong as two fused pair steps
// (Steps::Pair), in -> ping -> pong -> ping -> pong as four quarter steps.  The result is in pong.
int rotate_four_index(Steps steps, const double *in, int64_t sin, const double *C, int64_t sC, int ct, int n, double *ping,
                      int64_t sping, double *pong, int64_t spong, int count, hipStream_t st);
// What a gradient route works on: the views and the state of the call, the predicted 1-RDM, where the gradient goes.
struct GradCall {
    int n;
    const Geo &g;
    const Call &c;
    hipStream_t st;
    const double *D;   // predicted 1-RDM
    int64_t sD;
    double scale1;     // 0 drops everything that is not linear in G (multi-GPU partial ranks)
    bool add_gnuc;
    double *grad;
    int64_t sgrad;
};
// Gradient of the energy functional defined by (D, G), G unpacked (N^4), given X, U, s, K3 in the workspace (layouts
// 6 / 5 and evc_grad_elec_oao).
int gradient_unpacked(const GradCall &x, const double *G, int64_t sG);
// Phase C: the predicted RDMs of the weights in the workspace, then the gradient chain on the call's route.
int phase_gradient(const evc_trdm_set *t, const Geo &g_in, const Out &out, int flags, const Call &c, hipStream_t st);

}  // namespace evc
