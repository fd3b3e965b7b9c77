// Per-geometry orchestration: enqueues the whole energy(+force) DAG on one HIP stream.
// Mirrors get_energy_with_grad (gradients_loewdin.py:308-379) and approximate_*_OAO
// (evcont.py:178-250).  Two generalisations over the reference:
//   * BATCH: `count` independent geometries go through every launch together (batch index =
//     blockIdx.y / blockIdx.x) and share ONE pass over the t-RDM in the two streaming kernels;
//   * PHASES: split in three so a pair-sharded multi-GPU host can put its two small collectives
//     (all-gather of the H rows, all-reduce of the gradient) between them.
// This file: the three phases, the gradient routes and the single / batch entry points (the rest: pipeline.hpp).
#include "pipeline.hpp"

namespace evc {

// Many spans: sum the partials in a multi-workgroup launch instead of inside the eigensolver kernel.
static bool reduce_in_own_launch(const Call &c) { return c.rp2.nspans > 64; }

// y[g][r] = alpha * sum_k partial[g][k][r]: the fixed-order sum of the span partials, done here (many
// workgroups) rather than inside the single-workgroup eigensolver when there are many spans.
// Block = 64 rows x 4 span groups; blockIdx.y = geometry.
__global__ __launch_bounds__(256) void rows_reduce_kernel(const double *partial, int64_t spart, int64_t rows,
                                                          int nspans, double alpha, double *y, int64_t sy) {
    __shared__ double part[16][17];
    partial += (int64_t)blockIdx.y * spart;
    y += (int64_t)blockIdx.y * sy;
    const int rl = threadIdx.x & 15, grp = threadIdx.x >> 4;   // 16 rows x 16 span lanes
    const int64_t r = (int64_t)blockIdx.x * 16 + rl;
    double s0 = 0.0, s1 = 0.0;
    if (r < rows) {
        int k = grp;
        for (; k + 16 < nspans; k += 32) {
            s0 += partial[(int64_t)k * rows + r];
            s1 += partial[(int64_t)(k + 16) * rows + r];
        }
        if (k < nspans) s0 += partial[(int64_t)k * rows + r];
    }
    part[grp][rl] = s0 + s1;
    __syncthreads();
    if (grp == 0 && r < rows) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) s += part[k][rl];   // fixed order
        y[r] = alpha * s;
    }
}

int rotate_four_index(Steps steps, const double *in, int64_t sin, const double *C, int64_t sC, int ct, int n, double *ping,
                      int64_t sping, double *pong, int64_t spong, int count, hipStream_t st) {
    if (steps == Steps::Pair) {
        PairTransformArgs pa;
        memset(&pa, 0, sizeof(pa));
        pa.C = C;
        pa.sC = sC;
        pa.ct = ct;
        pa.n = n;
        pa.in = in;
        pa.sin = sin;
        pa.out = ping;
        pa.sout = sping;
        EVC_TRY(launch_pair_transform(pa, count, st));
        pa.in = ping;
        pa.sin = sping;
        pa.out = pong;
        pa.sout = spong;
        return launch_pair_transform(pa, count, st);
    }
    EVC_TRY(launch_quarter_transform(in, sin, C, sC, ct, n, ping, sping, count, st));
    EVC_TRY(launch_quarter_transform(ping, sping, C, sC, ct, n, pong, spong, count, st));
    EVC_TRY(launch_quarter_transform(pong, spong, C, sC, ct, n, ping, sping, count, st));
    return launch_quarter_transform(ping, sping, C, sC, ct, n, pong, spong, count, st);
}

// rows_out != NULL: the scaled two-body rows go to rows_out[g*srows_out + r] (r local) instead of the workspace.
static int phase_hamiltonian(const evc_trdm_set *t, const Geo &g_in, Call &c, bool reduce_rows, hipStream_t st,
                             double *rows_out = nullptr, int64_t srows_out = 0) {
    const Ws &w = c.w;
    const Route &route = c.eri;
    const int n = t->n, cnt = g_in.count;
    Geo g = g_in;
    if (g.eri_s4) {
        EVC_REQUIRE(route.symmetric, "EVC_FLAG_ERI_S4 needs the compressed layout (EVC_LAYOUT_SYM8) and N <= 64");
        const int64_t npr = (int64_t)n * (n + 1) / 2;
        if (cnt > 1) g.seri = npr * npr;
    }
    const int64_t sw = w.stride;
    if (!c.loewdin_done) {
        // the Loewdin step in the form the call chose (Call::split, side_stream.hip)
        LoewdinArgs la = loewdin_args(n, g, c);
        if (c.split == 1) {
            // the eigendecomposition of S (U, s: read by launch_grad_final alone) on the side stream, forked here: the
            // inputs are ready, U of the previous call has been consumed
            la.part = 2;
            EVC_TRY(side_launch_loewdin(w.base, la, cnt, st));
        } else {
            // this launch reads (warm start) and writes U and s: an eigensolver launch of an earlier energy-only call
            // on the side stream may still be writing them
            EVC_TRY(side_join(w.base, st));
        }
        char side_ran[kKernelRanLen] = "";
        if (c.split == 1) snprintf(side_ran, sizeof(side_ran), "%s", kernel_ran(EVC_PROF_LOEWDIN));
        la.part = c.split ? 1 : 0;
        EVC_TIMED(EVC_PROF_LOEWDIN, st, launch_loewdin(la, cnt, st));
        if (c.split == 1) {
            char main_ran[kKernelRanLen];
            snprintf(main_ran, sizeof(main_ran), "%s", kernel_ran(EVC_PROF_LOEWDIN));
            note_kernel(EVC_PROF_LOEWDIN, "%s; side stream: %s", main_ran, side_ran);
        }
        if (c.split == 3) c.la_ride = la;
    }
    // (ab|cd) -> K3[jkl][a] -> h2[ijkl]
    const double *v2;
    if (route.pairs()) {
        // two fused pair steps; the second one emits K3 and writes h2 straight into the form the
        // streaming kernel consumes (packed with diag x 1/2, or full)
        // the whole batch per launch, here and in the gradient tail: chunks of 16 geometries keep the intermediates
        // (6.5 MB per geometry) closer to the 256 MB Infinity Cache and measured within noise
        v2 = is_packed(t->layout) ? w.vec2 : w.B2;
        const int sym = route.symmetric ? 1 : 0;
        PairTransformArgs pa;
        memset(&pa, 0, sizeof(pa));
        pa.in = g.eri;
        pa.sin = g.seri;
        pa.C = w.X;
        pa.sC = sw;
        pa.n = n;
        // the intermediate; in the K3 buffer where the gradient phase recomputes K3 from it (route.hpp)
        double *mid = route.k3_is_dense_mid() ? w.K3 : w.B1;
        pa.out = mid;
        pa.sout = sw;
        // compressed layout: the AO integrals are 8-fold symmetric by contract, the first step only
        // produces the q <= p half of its output and the second one reads the lower triangles
        // (in_lower: eri[p,q,r,s] = eri[p,q,s,r]; rs_lower: the next step's leading pairs are (r',s'), s' <= r')
        pa.lead_sym = pa.in_lower = pa.rs_lower = sym;
        pa.in_pairs = g.eri_s4;       // int2e handed over as the dense (pair, pair) matrix (EVC_FLAG_ERI_S4)
        pa.in_ld = 0;                 // ... at the caller's pitch n(n+1)/2
        pa.out_pairs = pa.lead_sym;   // the intermediate as a dense (pair, pair) matrix
        pa.out_ld = pair_ld(n);
        EVC_TIMED(EVC_PROF_PAIR_TRANSFORM, st, launch_pair_transform(pa, cnt, st));
        pa.in_pairs = pa.out_pairs;
        pa.in_ld = pa.out_ld;
        pa.out_pairs = 0;
        pa.out_ld = 0;
        // ... and the second step again only needs the q <= p half of ITS leading pair
        pa.in = mid;
        pa.sin = sw;
        pa.k3 = route.k3_is_dense_mid() ? nullptr : w.K3;
        pa.sk3 = sw;
        if (is_packed(t->layout)) {
            pa.out = nullptr;
            pa.packed = w.vec2;
            pa.spacked = sw;
            pa.packed_len = t->ld2;
            pa.diag_mult = 0.5;
            pa.sym8 = sym;
        } else {
            pa.out = w.B2;
        }
        EVC_TIMED(EVC_PROF_PAIR_TRANSFORM, st, launch_pair_transform(pa, cnt, st));
    } else {
        // (through three buffers, K3 among them: not rotate_four_index)
        EVC_TRY(launch_quarter_transform(g.eri, g.seri, w.X, sw, 0, n, w.B1, sw, cnt, st));
        EVC_TRY(launch_quarter_transform(w.B1, sw, w.X, sw, 0, n, w.B2, sw, cnt, st));
        EVC_TRY(launch_quarter_transform(w.B2, sw, w.X, sw, 0, n, w.K3, sw, cnt, st));
        EVC_TRY(launch_quarter_transform(w.K3, sw, w.X, sw, 0, n, w.B1, sw, cnt, st));
        v2 = w.B1;
        if (is_packed(t->layout)) {
            EVC_TRY(is_sym8(t->layout) ? launch_pack_sym8(w.B1, sw, n, 0.5, w.vec2, sw, t->ld2, cnt, st)
                                    : launch_pack(w.B1, sw, n, 0.5, w.vec2, sw, t->ld2, cnt, st));
            v2 = w.vec2;
        }
    }
    RowProblem p2 = c.rp2, p1 = c.rp1;
    p2.A = t->two_rdm;
    p2.v = v2;
    p2.partial = w.h2part;
    p2.vstride = p2.pstride = sw;
    if (t->rows2 == 0) p2.nblocks = 0;
    p1.A = t->one_rdm;
    p1.v = w.h1;
    p1.partial = w.h1part;
    p1.vstride = p1.pstride = sw;
    EVC_TIMED(EVC_PROF_ROWS, st, launch_gemv_rows(p2, p1, cnt, st));
    if ((reduce_rows || reduce_in_own_launch(c)) && t->rows2 > 0) {
        const double alpha2 = is_packed(t->layout) ? 1.0 : 0.5;
        hipLaunchKernelGGL(rows_reduce_kernel, dim3((unsigned)ceil_div(t->rows2, 16), (unsigned)cnt), dim3(256), 0,
                           st, w.h2part, sw, t->rows2, c.rp2.nspans, alpha2,
                           rows_out ? rows_out : w.h2rows + t->row_offset, rows_out ? srows_out : sw);
        EVC_LAUNCH_CHECK("rows_reduce");
    }
    return 0;
}

static int phase_solve(const evc_trdm_set *t, const Geo &g, const double *h2rows_all, int64_t sh2_all, const Out &out,
                       int nroots, const Call &c, hipStream_t st) {
    const Ws &w = c.w;
    SolveArgs a;
    memset(&a, 0, sizeof(a));
    const int64_t sw = w.stride;
    a.h1part = w.h1part;
    a.nsp1 = c.rp1.nspans;
    a.alpha1 = 1.0;
    a.sh1 = sw;
    if (h2rows_all || reduce_in_own_launch(c)) {
        // the complete rows: the caller's, or written by rows_reduce_kernel in phase A (complete t-RDM on this device)
        a.h2part = h2rows_all ? h2rows_all : w.h2rows;
        a.nsp2 = 1;
        a.alpha2 = 1.0;
        a.sh2 = h2rows_all ? sh2_all : sw;
    } else {
        a.h2part = w.h2part;
        a.nsp2 = c.rp2.nspans;
        a.alpha2 = is_packed(t->layout) ? 1.0 : 0.5;
        a.sh2 = sw;
    }
    a.S = t->s_train;
    a.T = t->ntrain;
    a.layout = t->layout;
    a.nroots = nroots;
    a.e_shift = g.enuc;
    a.e_shift_dev = g.enuc_dev;
    a.evals = out.energy ? out.energy : w.evals;   // (one geometry may leave them in the workspace)
    a.sev = out.energy ? out.se : sw;
    a.evecs = out.coeffs ? out.coeffs : w.evecs;
    a.svec = out.coeffs ? out.sc : sw;
    a.Hout = out.hmat;
    a.sH = out.sH;
    a.w2 = w.w2;
    a.w2t = g.count > 1 ? w.w2t : nullptr;
    a.w1t = g.count > 1 ? w.w1t : nullptr;
    a.w1 = w.w1;
    a.sw = sw;
    a.w2_offset = t->row_offset;
    a.w2_count = t->rows2;
    a.vstd = w.vstd;
    a.bcache = w.bcache;
    a.scratch = w.sbig;
    a.sscratch = sw;
    a.warm = c.warm ? 1 : 0;
    const int pr = prof_start(EVC_PROF_SUBSPACE, st);
    const int rc = c.split == 3 ? launch_subspace_loewdin(a, c.la_ride, g.count, st) : launch_subspace_solve(a, g.count, st);
    prof_stop(pr, st);
    return rc;
}

// ---- the gradient chain: one function per route, a shared head and tail ------------------------------------------------
// Gradient of the energy functional defined by (D, G) given X, U, s and the K3 buffer in the workspace.  The packed
// routes take both symmetrisations straight from the packed predicted 2-RDM (G is then only written when the caller
// wants it, G may be NULL).  Only the pair-step routes time their stages (timed).
static GradPrepArgs grad_prep_args(const GradCall &x) {
    const Ws &w = x.c.w;
    GradPrepArgs p;
    p.n = x.n;
    p.X = w.X;
    p.hcore = x.g.hcore;
    p.D = x.D;
    p.Pao = w.Pao;
    p.Y1 = w.Y1;
    p.sws = w.stride;
    p.sh = x.g.sh;
    p.sD = x.sD;
    p.scale1 = x.scale1;
    p.geo_period = x.g.geo_period;
    return p;
}
// the shared head
static int grad_head(const GradCall &x) { return launch_grad_prep(grad_prep_args(x), x.g.count, x.st); }

// The shared tail: the int2e_ip1 contraction with G^AO in the form (presym, fold_cd, ip1_s2kl: Ip1Args, kernels.hpp) and
// the sum of `nslab` Y2 slabs, the join of the side stream, the response term.
// ip1_prof: the timing bracket the second pair step opened when it did the pair blocks' dot (ip1_pairs_done): closed
// behind the residual launch here.
static int grad_tail(const GradCall &x, const double *gao, int presym, int fold_cd, int ip1_s2kl, int nslab, bool timed,
                     bool ip1_pairs_done = false, int ip1_prof = -1) {
    const Ws &w = x.c.w;
    const Geo &g = x.g;
    const int n = x.n, cnt = g.count;
    const int64_t sw = w.stride;
    Ip1Args ia;
    ia.ip1 = g.eri_ip1;
    ia.Gao = gao;
    ia.presym = presym;
    ia.fold_cd = fold_cd;
    ia.ip1_s2kl = ip1_s2kl;
    ia.t2part = w.t2part;
    ia.dh = g.dhcore;
    ia.Pao = w.Pao;
    ia.term3 = w.term3;
    ia.y2part = w.y2part;
    ia.y2 = w.y2;
    ia.sip1 = g.sip1;
    ia.sdh = g.sdh;
    ia.sws = sw;
    ia.n = n;
    ia.natm = g.natm;
    ia.nslab = nslab;
    ia.nchunk = ip1_chunks(n);
    ia.geo_period = g.geo_period;
    ia.slots = g.geo_period > 0 ? cnt / g.geo_period : 1;
    ia.pairs_done = ip1_pairs_done ? 1 : 0;
    if (ip1_pairs_done) {
        EVC_TRY(launch_ip1_dh(ia, cnt, x.st));
        prof_stop(ip1_prof, x.st);
    } else {
        EVC_TIMED(timed ? EVC_PROF_IP1 : -1, x.st, launch_ip1_dh(ia, cnt, x.st));
    }
    EVC_TRY(side_join(w.base, x.st));   // U and s may come from the side stream (phase_hamiltonian)
    GradFinalArgs f;
    f.n = n;
    f.natm = g.natm;
    f.U = w.U;
    f.s = w.s;
    f.Y1 = w.Y1;
    f.y2 = w.y2;
    f.ipovlp = g.ipovlp;
    f.aoslices = g.aoslices;
    f.t2part = w.t2part;
    f.nchunk = ip1_chunks(n);
    f.term3 = w.term3;
    f.gnuc = x.add_gnuc ? g.gnuc : nullptr;
    f.scale1 = x.scale1;
    f.grad = x.grad;
    f.sws = sw;
    f.sip = g.sip;
    f.sgn = g.sgn;
    f.sgrad = x.sgrad;
    f.geo_period = g.geo_period;
    return launch_grad_final(f, cnt, x.st);
}

// The first gradient-side pair step, B1 -> B2, G^AO = (X x X x X x X) G with the contraction over the SECOND index of X
// (gradients_loewdin.py:224-232); sym: SB is fully symmetric (the symmetric pipeline).
static PairTransformArgs grad_first_step(const Ws &w, int n, int sym) {
    PairTransformArgs a;
    memset(&a, 0, sizeof(a));
    a.C = w.X;
    a.sC = w.stride;
    a.ct = 1;
    a.n = n;
    a.in = w.B1;
    a.sin = w.stride;
    a.out = w.B2;
    a.sout = w.stride;
    a.lead_sym = a.in_lower = a.rs_lower = a.out_pairs = sym;
    a.in_ld = a.out_ld = pair_ld(n);   // (pitch of every dense (pair, pair) form of the pipeline)
    return a;
}
// (... and the second, B2 -> B1: grad_second_args, pair_plan.hpp)

// G unpacked, N^4 (layouts 6 / 5 and evc_grad_elec_oao): symmetrise -> Y2 -> rotate G itself -> IP1 symmetrises on the fly
int gradient_unpacked(const GradCall &x, const double *G, int64_t sG) {
    const Ws &w = x.c.w;
    const int n = x.n, cnt = x.g.count;
    const int64_t sw = w.stride;
    EVC_TRY(grad_head(x));
    EVC_TRY(launch_sym_oao_t(G, sG, n, w.B2, sw, cnt, x.st));
    EVC_TRY(launch_y2(w.B2, w.K3, n, w.y2part, sw, cnt, x.st));
    // (two pair steps end in B2, four quarter steps in B1: one more hop would cost a launch)
    const bool pairs = x.c.ip1.pairs();
    double *ping = pairs ? w.B1 : w.B2, *pong = pairs ? w.B2 : w.B1;
    EVC_TRY(rotate_four_index(x.c.ip1.steps, G, sG, w.X, sw, 1, n, ping, sw, pong, sw, cnt, x.st));
    return grad_tail(x, pong, 0, 0, 0, y2_slabs(n), false);
}

// Packed reference layouts (3 / 2): unpack + both symmetrisations (B2: OAO, transposed, for Y2; B1: AO-type) -> Y2 ->
// B1 -> B2 -> B1 (AO) as two pair steps, or B1 -> B2 -> B1 -> B2 -> B1 as four quarter steps
static int gradient_packed_ref(const GradCall &x, const double *packed, int64_t spacked, double *G, int64_t sG) {
    const Ws &w = x.c.w;
    const int n = x.n, cnt = x.g.count;
    const int64_t sw = w.stride;
    const bool pairs = x.c.ip1.pairs();
    EVC_TRY(grad_head(x));
    EVC_TIMED(pairs ? EVC_PROF_UNPACK : -1, x.st, launch_unpack_sym(packed, spacked, n, w.B2, w.B1, sw, G, sG, cnt, x.st));
    EVC_TIMED(pairs ? EVC_PROF_Y2 : -1, x.st, launch_y2(w.B2, w.K3, n, w.y2part, sw, cnt, x.st));
    if (pairs) {
        const PairTransformArgs pa = grad_first_step(w, n, 0);
        EVC_TIMED(EVC_PROF_PAIR_TRANSFORM, x.st, launch_pair_transform(pa, cnt, x.st));
        EVC_TIMED(EVC_PROF_PAIR_TRANSFORM, x.st, launch_pair_transform(grad_second_args(pa, w.B1, 0), cnt, x.st));
    } else if (int rc = rotate_four_index(Steps::Quarter, w.B1, sw, w.X, sw, 1, n, w.B2, sw, w.B1, sw, cnt, x.st)) {
        return rc;
    }
    return grad_tail(x, w.B1, 1, 0, 0, y2_slabs(n), pairs);
}

// Compressed layout on quarter steps (n > 32 with full int2e / int2e_ip1): unpack -> Y2 with the row-major SB ->
// B1 -> B2 -> B1 -> B2 -> B1 (AO)
static int gradient_sym8_quarter(const GradCall &x, const double *packed, int64_t spacked, double *G, int64_t sG) {
    const Ws &w = x.c.w;
    const int n = x.n, cnt = x.g.count;
    const int64_t sw = w.stride;
    EVC_TRY(grad_head(x));
    EVC_TRY(launch_unpack8(packed, spacked, n, w.B1, sw, G, sG, cnt, 0, x.st));
    EVC_TRY(launch_y2_sb(w.B1, w.K3, n, w.y2part, sw, cnt, x.st));
    EVC_TRY(rotate_four_index(Steps::Quarter, w.B1, sw, w.X, sw, 1, n, w.B2, sw, w.B1, sw, cnt, x.st));
    return grad_tail(x, w.B1, 1, 0, 0, y2_slabs(n), false);
}

// The symmetric pipeline (compressed layout on pair steps, n <= 32 and the 64-wide form): unpack into the dense
// (pair, pair) SB -> Y2 from the energy phase's intermediate in the K3 buffer (K3 was written for l <= k only) ->
// B1 -> B2 -> B1 (AO, dense where int2e_ip1 is packed: the packed-ip1 dot weighs the pairs itself).  The Y2 kernel does
// the first pair step as well where the plan says so (plan_grad_pairs), otherwise that is the first of two pair-transform
// launches.  With G the first unpack writes the N^4-addressed SB that comes with it:
//   n <= 32: the first pair step reads that; a second unpack writes the dense form for Y2, to B2, free until the next
//            step -- or over SB in B1 when the Y2 kernel is the first pair step as well and writes B2;
//   64-wide: it is not used -- it goes to B2, which the next step overwrites -- and a second unpack gives B1 the dense
//            form every step reads.
// Without G, grad_prep rides in the unpack launch, n <= 32 only: every block of the shared launch reserves grad_prep's
// LDS -- 52 KB there, 108 KB at n = 58, where the unpack blocks would run one per CU.
static int gradient_sym8_pairs(const GradCall &x, const double *packed, int64_t spacked, double *G, int64_t sG,
                               int ip1_s2kl) {
    const Ws &w = x.c.w;
    const int n = x.n, cnt = x.g.count;
    const int64_t sw = w.stride;
    hipStream_t st = x.st;
    const bool p64 = x.c.ip1.steps == Steps::Pair64, prep_rides = !G && !p64;
    if (!prep_rides) EVC_TRY(grad_head(x));
    int pr = prof_start(EVC_PROF_UNPACK, st);
    if (prep_rides)
        EVC_TRY(launch_unpack8_prep(grad_prep_args(x), packed, spacked, w.B1, sw, cnt, st));
    else
        EVC_TRY(launch_unpack8(packed, spacked, n, G && p64 ? w.B2 : w.B1, sw, G, sG, cnt, G ? 1 : 2, st));
    if (G && p64) EVC_TRY(launch_unpack8(packed, spacked, n, w.B1, sw, nullptr, 0, cnt, 2, st));
    prof_stop(pr, st);
    pr = prof_start(EVC_PROF_Y2, st);
    PairTransformArgs pa = grad_first_step(w, n, 1);
    pa.in_pairs = 1;   // (the dense form: what Y2 reads; the plan has the form each step is launched with)
    const Geo &g = x.g;
    const GradPairPlan plan = plan_grad_pairs(pa, w.B1, w.K3, sw, cnt, G != nullptr, p64, ip1_s2kl,
                                              g.geo_period <= 0 || cnt == g.geo_period, pair_knobs());
    const double *sbp = w.B1;
    if (G && !p64) {
        double *dense = plan.y2_in_first ? w.B1 : w.B2;
        EVC_TRY(launch_unpack8(packed, spacked, n, dense, sw, nullptr, 0, cnt, 2, st));
        sbp = dense;
    }
    if (plan.y2_in_first)
        EVC_TRY(launch_y2_pairstep(plan.y2, pa, w.K3, w.y2part, sw, cnt, st));
    else
        EVC_TRY(launch_y2_fused(plan.y2, sbp, w.K3, w.X, sw, n, w.y2part, sw, cnt, st));
    prof_stop(pr, st);
    if (!plan.y2_in_first)
        EVC_TIMED(EVC_PROF_PAIR_TRANSFORM, st, launch_pair_transform(plan.first, plan.first_args, cnt, st));
    if (plan.dot_in_second) {
        // the launch belongs to the int2e_ip1 stage's time: grad_tail closes the bracket behind the residual ip1_dh_kernel launch
        const PairDotArgs dt{g.eri_ip1, w.t2part, g.sip1, sw, ip1_chunks(n)};
        const int ip1_prof = prof_start(EVC_PROF_IP1, st);
        EVC_TRY(launch_pair_transform_dot(plan.second, plan.second_args, dt, cnt, st));
        return grad_tail(x, w.B1, 1, 1, ip1_s2kl, plan.nslab(), true, true, ip1_prof);
    }
    EVC_TIMED(EVC_PROF_PAIR_TRANSFORM, st, launch_pair_transform(plan.second, plan.second_args, cnt, st));
    return grad_tail(x, w.B1, 1, 1, ip1_s2kl, plan.nslab(), true);
}

int phase_gradient(const evc_trdm_set *t, const Geo &g_in, const Out &out, int flags, const Call &c, hipStream_t st) {
    const Ws &w = c.w;
    const int n = t->n, cnt = g_in.count;
    Geo g = g_in;
    const int s2kl = (flags & EVC_FLAG_IP1_S2KL) ? 1 : 0;
    if (s2kl) {
        EVC_REQUIRE(c.ip1.symmetric, "EVC_FLAG_IP1_S2KL needs the compressed layout (EVC_LAYOUT_SYM8) and N <= 64");
        if (cnt > 1 && g.sip1) g.sip1 = (int64_t)3 * n * n * (n * (n + 1) / 2);   // (0: one geometry shared by the slots)
    }
    const int64_t sw = w.stride;
    double *D = out.d_pred ? out.d_pred : w.Dpred;
    const int64_t sD = out.d_pred ? out.sd : sw;
    double *G = out.g_pred ? out.g_pred : w.G;
    const int64_t sG = out.g_pred ? out.sG : sw;
    ColProblem c2{}, c1{};
    c2.A = t->two_rdm;
    c2.w = w.w2;
    c2.wt = cnt > 1 ? w.w2t : nullptr;
    c2.wstride = sw;
    c2.rows = t->rows2;
    c2.cols = t->cols2;
    c2.ld = t->ld2;
    if (is_packed(t->layout)) {
        c2.out = w.vec2;
        c2.ostride = sw;
    } else {
        c2.out = G;
        c2.ostride = sG;
    }
    c1.A = t->one_rdm;
    c1.w = w.w1;
    c1.wt = cnt > 1 ? w.w1t : nullptr;
    c1.wstride = sw;
    c1.rows = (int64_t)t->ntrain * t->ntrain;
    c1.cols = (int64_t)n * n;
    c1.ld = t->ld1;
    c1.out = D;
    c1.ostride = sD;
    c1.part = (int64_t)t->ntrain * t->ntrain >= 1024 ? w.d1part : nullptr;
    c1.pstride = sw;
    EVC_TIMED(EVC_PROF_COLS, st, launch_gemv_cols(c2, c1, cnt, st));
    const bool partial = (flags & EVC_FLAG_PARTIAL_RANK) != 0;
    const GradCall x{n, g, c, st, D, sD, partial ? 0.0 : 1.0, !partial, out.grad, out.sg};
    if (!is_packed(t->layout)) return gradient_unpacked(x, G, sG);
    // the unpacked 2-RDM is only materialised when the caller asked for it
    if (!is_sym8(t->layout)) return gradient_packed_ref(x, w.vec2, sw, out.g_pred, out.sG);
    if (!c.ip1.pairs()) return gradient_sym8_quarter(x, w.vec2, sw, out.g_pred, out.sG);
    return gradient_sym8_pairs(x, w.vec2, sw, out.g_pred, out.sG, s2kl);
}

// ---- one body per operation: the full call and the phases A, B, C --------------------------------------------------
// Each takes the two views and serves the single-geometry entry point and its _batch twin alike.  Where the two differ
// on purpose it says so (Geo::batch): a batch is handed its rows, energies and coefficients in the caller's arrays, one
// geometry may leave them in the workspace.

// what the subspace solve needs of its caller (full call and phase B)
static int check_solve(const char *who, const evc_trdm_set *t, const Geo &g, const Out &o, int nroots) {
    EVC_REQUIRE(!g.batch || (o.energy && o.coeffs), "%s: batch outputs.energy/coeffs are required", who);
    EVC_REQUIRE(nroots >= 1 && nroots <= t->ntrain, "%s: nroots=%d out of range 1..%d", who, nroots, t->ntrain);
    return 0;
}

static int full_call(const char *who, const evc_trdm_set *t, Geo g, const Out &o, int nroots, int flags, void *ws,
                     size_t ws_bytes, void *stream) {
    const bool energy_only = (flags & EVC_FLAG_ENERGY_ONLY) != 0;
    if (check_set(t) || check_geometry(who, g, !energy_only)) return -1;
    EVC_REQUIRE(energy_only || o.grad, "%s: outputs.grad is required unless EVC_FLAG_ENERGY_ONLY", who);
    Call c;
    if (setup(who, t, g, flags, ws, ws_bytes, g.count, c) || check_solve(who, t, g, o, nroots)) return -1;
    EVC_REQUIRE(t->rows2 == t->rows2_total && t->row_offset == 0,
                "%s needs the complete t-RDM on this device (use the phase calls when sharded)", who);
    const int s2kl = flags & EVC_FLAG_IP1_S2KL;
    EVC_REQUIRE(energy_only || phases_agree(t->n, g.eri_s4 != 0, s2kl != 0),
                "%s: N > 32: EVC_FLAG_ERI_S4 and EVC_FLAG_IP1_S2KL go together (both packed inputs, or neither)", who);
    hipStream_t st = as_stream(stream);
    c.split = loewdin_split_mode(t->n, t->ntrain, g.count, c.loewdin_done, c.warm, st);
    EVC_TRY(phase_hamiltonian(t, g, c, false, st));
    EVC_TRY(phase_solve(t, g, nullptr, 0, o, nroots, c, st));
    if (energy_only) return 0;
    // (of the two bits the gradient phase reads, EVC_FLAG_PARTIAL_RANK belongs to the phase calls alone)
    return phase_gradient(t, g, o, s2kl, c, st);
}

// Phase A.  rows_out NULL (one geometry): the rows stay in the workspace, c.w tells the caller where.
static int hamiltonian_call(const char *who, const evc_trdm_set *t, Geo g, int flags, double *rows_out,
                            int64_t ld_rows_out, void *ws, size_t ws_bytes, void *stream, Call &c) {
    if (check_set(t) || check_geometry(who, g, false) || setup(who, t, g, flags, ws, ws_bytes, g.count, c)) return -1;
    EVC_REQUIRE(!g.batch || t->rows2 == 0 || (rows_out && ld_rows_out >= t->rows2),
                "%s: rows_out NULL or ld_rows_out=%lld < rows2=%lld", who, (long long)ld_rows_out, (long long)t->rows2);
    return phase_hamiltonian(t, g, c, true, as_stream(stream), rows_out, ld_rows_out);
}

// Phase B.  h2rows_all NULL (one geometry): the rows phase A left in the workspace.
static int solve_call(const char *who, const evc_trdm_set *t, Geo g, const double *h2rows_all, int64_t ld_rows_all,
                      const Out &o, int nroots, int flags, void *ws, size_t ws_bytes, void *stream) {
    Call c;
    if (check_set(t) || check_geometry(who, g, false) || setup(who, t, g, flags, ws, ws_bytes, g.count, c) ||
        check_solve(who, t, g, o, nroots))
        return -1;
    EVC_REQUIRE(!g.batch || (h2rows_all && ld_rows_all >= t->rows2_total),
                "%s: h2rows_all NULL or ld_rows_all=%lld < rows2_total=%lld", who, (long long)ld_rows_all,
                (long long)t->rows2_total);
    return phase_solve(t, g, h2rows_all ? h2rows_all : c.w.h2rows, ld_rows_all, o, nroots, c, as_stream(stream));
}

// Phase C.
static int gradient_call(const char *who, const evc_trdm_set *t, Geo g, const Out &o, int flags, void *ws,
                         size_t ws_bytes, void *stream) {
    if (check_set(t) || check_geometry(who, g, true)) return -1;
    EVC_REQUIRE(o.grad, "%s: outputs.grad is required", who);
    Call c;
    if (setup(who, t, g, flags, ws, ws_bytes, g.count, c)) return -1;
    return phase_gradient(t, g, o, flags & (EVC_FLAG_IP1_S2KL | EVC_FLAG_PARTIAL_RANK), c, as_stream(stream));
}

}  // namespace evc

using namespace evc;

// ---- the single-geometry entry points and their _batch twins: clear the stage records, build the two views, call ----
// EVC_FLAG_LOEWDIN_DONE belongs to the batch calls; callers pass one flag word to both forms, one geometry ignores it.
constexpr int kSingleFlags = ~EVC_FLAG_LOEWDIN_DONE;

extern "C" int evc_energy_with_grad(const evc_trdm_set *t, const evc_geometry *g, const evc_outputs *out,
                                    int nroots, int flags, void *ws, size_t ws_bytes, void *stream) {
    clear_kernels(kStagesAll);
    EVC_REQUIRE(out != nullptr, "evc_energy_with_grad: outputs is NULL");
    return full_call("evc_energy_with_grad", t, geo_single(g), out_single(out), nroots, flags & kSingleFlags, ws,
                     ws_bytes, stream);
}

extern "C" int evc_energy_with_grad_batch(const evc_trdm_set *t, const evc_geometry_batch *gb,
                                          const evc_outputs_batch *ob, int nroots, int flags, void *ws,
                                          size_t ws_bytes, void *stream) {
    clear_kernels(kStagesAll);
    return full_call("evc_energy_with_grad_batch", t, geo_batch(t, gb), out_batch(t, gb, ob), nroots, flags, ws,
                     ws_bytes, stream);
}

extern "C" int evc_phase_hamiltonian(const evc_trdm_set *t, const evc_geometry *g, int flags, void *ws, size_t ws_bytes,
                                     double **h2rows_local, double **h1rows, void *stream) {
    clear_kernels(kStagesHamiltonian);
    Call c;
    EVC_TRY(hamiltonian_call("evc_phase_hamiltonian", t, geo_single(g), flags & kSingleFlags, nullptr, 0, ws,
                                  ws_bytes, stream, c));
    if (h2rows_local) *h2rows_local = c.w.h2rows + t->row_offset;
    if (h1rows) *h1rows = c.w.h1part;
    return 0;
}

extern "C" int evc_phase_hamiltonian_batch(const evc_trdm_set *t, const evc_geometry_batch *gb, int flags,
                                           double *rows_out, int64_t ld_rows_out, void *ws, size_t ws_bytes,
                                           void *stream) {
    clear_kernels(kStagesHamiltonian);
    Call c;
    return hamiltonian_call("evc_phase_hamiltonian_batch", t, geo_batch(t, gb), flags, rows_out, ld_rows_out, ws,
                            ws_bytes, stream, c);
}

extern "C" int evc_phase_solve(const evc_trdm_set *t, const evc_geometry *g, const double *h2rows_all,
                               const evc_outputs *out, int nroots, int flags, void *ws, size_t ws_bytes, void *stream) {
    clear_kernels(1u << EVC_PROF_SUBSPACE);
    return solve_call("evc_phase_solve", t, geo_single(g), h2rows_all, 0, out_single(out), nroots, flags, ws, ws_bytes,
                      stream);
}

extern "C" int evc_phase_solve_batch(const evc_trdm_set *t, const evc_geometry_batch *gb, const double *h2rows_all,
                                     int64_t ld_rows_all, const evc_outputs_batch *ob, int nroots, int flags,
                                     void *ws, size_t ws_bytes, void *stream) {
    clear_kernels(1u << EVC_PROF_SUBSPACE);
    return solve_call("evc_phase_solve_batch", t, geo_batch(t, gb), h2rows_all, ld_rows_all, out_batch(t, gb, ob),
                      nroots, flags, ws, ws_bytes, stream);
}

extern "C" int evc_phase_gradient(const evc_trdm_set *t, const evc_geometry *g, const evc_outputs *out,
                                  int flags, void *ws, size_t ws_bytes, void *stream) {
    clear_kernels(kStagesGradient);
    return gradient_call("evc_phase_gradient", t, geo_single(g), out_single(out), flags, ws, ws_bytes, stream);
}

extern "C" int evc_phase_gradient_batch(const evc_trdm_set *t, const evc_geometry_batch *gb,
                                        const evc_outputs_batch *ob, int flags, void *ws, size_t ws_bytes,
                                        void *stream) {
    clear_kernels(kStagesGradient);
    return gradient_call("evc_phase_gradient_batch", t, geo_batch(t, gb), out_batch(t, gb, ob), flags, ws, ws_bytes,
                         stream);
}

extern "C" int evc_phase_set_coeffs(const evc_trdm_set *t, const double *coeffs, int natm, void *ws, size_t ws_bytes,
                                    void *stream) {
    if (check_set(t)) return -1;
    EVC_REQUIRE(coeffs, "evc_phase_set_coeffs: coeffs is NULL");
    Geo g = geo_single(nullptr);   // (no geometry: the workspace of one slot for natm atoms)
    g.natm = natm;
    Call c;
    if (setup("evc_phase_set_coeffs", t, g, 0, ws, ws_bytes, 1, c)) return -1;
    return launch_pair_weights(coeffs, t->ntrain, t->layout, c.w.w1, c.w.w2, t->row_offset, t->rows2, as_stream(stream));
}

extern "C" int evc_phase_loewdin_batch(const evc_trdm_set *t, const evc_geometry_batch *gb, int flags, void *ws,
                                       size_t ws_bytes, void *stream) {
    const char *who = "evc_phase_loewdin_batch";
    clear_kernels(1u << EVC_PROF_LOEWDIN);
    Geo g = geo_batch(t, gb);
    if (check_set(t)) return -1;
    EVC_REQUIRE(g.count >= 1 && g.count <= 4096 && g.S && g.hcore, "%s: batch descriptor / S / hcore missing", who);
    Call c;
    if (setup(who, t, g, flags, ws, ws_bytes, g.count, c)) return -1;
    hipStream_t st = as_stream(stream);
    // (rewrites U and s: after an energy-only call their eigensolver launch may still be running on the side stream)
    EVC_TRY(side_join(c.w.base, st));
    return launch_loewdin(loewdin_args(t->n, g, c), g.count, st);
}
