/*
 * evcont_hip.h -- C ABI of libevcont_hip.so: the MI355X (gfx950) kernels behind the
 * eigenvector-continuation energy/force hot path of BoothGroup/evcont.
 *
 * The reference has no FFI layer (it is pure numpy/scipy/PySCF); its boundary for this
 * path is the Python API of three modules.  Every entry point below replaces one dense
 * operation of those modules and cites it as file:line under /root/reference/evcont.
 * The host-side mirror of the Python API (the evcont_amd Python modules) binds these symbols with
 * ctypes; INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to float64 (int64 for aoslices) unless noted;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *     synchronises, nothing allocates.  State kept by the library: a thread-local error string; per
 *     kernel one bit per device "dynamic LDS limit raised" (hipFuncSetAttribute is per device: one
 *     process may drive several devices through this library); the opt-in evc_profile_* measurement
 *     hook (process-wide, mutex-protected); tuning knobs read from the environment once per process;
 *   - return value 0 = success; <0 = argument error (nothing enqueued);
 *     >0 = hipError_t of a failed launch;
 *   - matrices are row-major (C order), exactly as numpy hands them to the reference.
 */
#ifndef EVCONT_HIP_H
#define EVCONT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EVC_ABI_VERSION 10 /* 2: batched phases, evc_subspace_solve_batch, evc_integrals_oao_batch, EVC_FLAG_WARM_START;
                             3: EVC_LAYOUT_SYM8; 4: evc_profile_stage/_select, EVC_FLAG_IP1_S2KL, EVC_FLAG_ERI_S4;
                             5: evc_phase_set_coeffs; 6: evc_phase_loewdin_batch, EVC_FLAG_LOEWDIN_DONE;
                             7: training sets of up to 512 states (evc_subspace_solve[_batch] take a workspace,
                                evc_subspace_solve_ws_bytes), `flags` argument of the phase A / B entry points;
                             8: evc_profile_kernel; the workspace of the compressed layout's pipeline holds its dense
                                (pair, pair) intermediates at the pitch N(N+1)/2 rounded up to 16 doubles;
                             9: evc_release_workspace (a workspace may own a side stream);
                             10: evc_phase_gradient_roots, evc_workspace_bytes_roots, evc_outputs_roots;
                                 later additions under 10 (no existing signature or behaviour changed):
                                 evc_phase_gradient_roots_batch, evc_workspace_bytes_roots_batch;
                                 evc_fci_excite, evc_fci_trdm_rows, evc_fci_sigma, evc_fci_workspace_bytes and the
                                 stages EVC_PROF_FCI_*; additive: evc_fci_hdiag, evc_fci_dots, evc_fci_combine,
                                 evc_fci_davidson_correction, evc_fci_solve_workspace_bytes, EVC_PROF_FCI_SOLVE;
                                 additive: evc_fci_rotate, evc_fci_rotate_workspace_bytes, EVC_PROF_FCI_ROTATE;
                                 additive: evc_fci_trdm_rows_packed, evc_fci_rows_packed_workspace_bytes,
                                 EVC_PROF_FCI_PACK; additive: evc_fci_spin_apply, evc_fci_spin_diag;
                                 evc_trdm_plan_describe; additive: evc_cas_expand_rows,
                                 evc_cas_expand_workspace_bytes, evc_cas_expand_describe; additive:
                                 evc_properties_roots_batch, evc_properties_workspace_bytes, evc_sgto_dipole_batch;
                                 additive: evc_spgto_workspace_bytes, evc_spgto_integrals_batch,
                                 evc_spgto_dipole_batch; additive: evc_spdgto_workspace_bytes,
                                 evc_spdgto_integrals_batch, evc_spdgto_dipole_batch; additive:
                                 evc_fci_rotate_block, evc_fci_rotate_block_workspace_bytes; additive:
                                 evc_fci_trdm_rows_block, evc_fci_rows_block_workspace_bytes; additive:
                                 evc_sgto_dipole_grad_batch, evc_gto_dipole_grad_batch, evc_field_fold_batch;
                                 additive: evc_spdfgto_workspace_bytes, evc_spdfgto_integrals_batch,
                                 evc_spdfgto_dipole_batch, evc_spdfgto_dipole_grad_batch */

/* t-RDM storage layouts = ndim of the reference's two_RDM argument
 * (ab_initio_eigenvector_continuation.py:41-68). */
#define EVC_LAYOUT_FULL6 6 /* (T,T,N,N,N,N)  rows=T*T        cols=N^4          */
#define EVC_LAYOUT_PAIR5 5 /* (P,N,N,N,N)    rows=T(T+1)/2   cols=N^4          */
#define EVC_LAYOUT_ELEC3 3 /* (T,T,M)        rows=T*T        cols=N^2(N^2+1)/2 */
#define EVC_LAYOUT_PACK2 2 /* (P,M)          rows=T(T+1)/2   cols=M            */
/* Device-side compressed layout (no counterpart in the reference): per training pair (a >= b) the
 * 8-fold symmetrised t-RDM
 *   Gs[i,j,k,l] = mean of Gamma over (i<->j), (k<->l), (ij<->kl)
 * stored for i >= j, k >= l, u = i(i+1)/2+j >= v = k(k+1)/2+l at column u(u+1)/2+v:
 *   rows = T(T+1)/2, cols = Ms(Ms+1)/2 with Ms = N(N+1)/2      (3.7x fewer bytes than PACK2 at N = 30).
 * H_ab and the nuclear gradient only see this part of Gamma WHEN THE AO INTEGRALS HAVE THE INDEX
 * SYMMETRIES OF REAL TWO-ELECTRON INTEGRALS: eri[p,q,r,s] 8-fold symmetric and eri_ip1[x,p,q,r,s] =
 * eri_ip1[x,p,q,s,r] (true for every int2e / int2e_ip1 of real AOs).  Energies, coefficients and gradients are
 * then those of the reference layouts to rounding; g_pred is the symmetrised predicted 2-RDM. */
#define EVC_LAYOUT_SYM8 8

int evc_abi_version(void);
/* Message of the last failing call on this host thread ("" if none). */
const char *evc_last_error(void);

/* ---------------------------------------------------------------------------------
 * K5/K4  H2 = Gamma . h2   -- streaming row GEMV (HBM bound)
 *   y[r] = alpha * sum_{c<cols} A[r*ld + c] * v[c]            r < rows
 * replaces np.tensordot(two_RDM, h2, axes=4) / two_RDM.dot(h2_compressed) and
 * np.tensordot(one_RDM, h1, axes=2)   (ab_initio_eigenvector_continuation.py:38,43,47,57,64)
 * Requirements: A and v 16-byte aligned, ld even, ld >= cols.  `ws` holds the
 * per-span partial sums (deterministic two-stage reduction, no atomics).
 * --------------------------------------------------------------------------------- */
size_t evc_gemv_rows_ws_bytes(int64_t rows, int64_t cols);
int evc_gemv_rows(const double *A, int64_t rows, int64_t cols, int64_t ld, const double *v,
                  double alpha, double *y, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * K8/K7  Gamma_pred = w . Gamma  -- streaming column GEMV (GEMV-T, HBM bound)
 *   out[c] = sum_{r<rows} w[r] * A[r*ld + c]                  c < cols
 * replaces np.tensordot(weights, two_RDM) (ab_initio_gradients_loewdin.py:343,351-356).
 * Requirements: A and out 16-byte aligned, ld even.
 * --------------------------------------------------------------------------------- */
int evc_gemv_cols(const double *A, int64_t rows, int64_t cols, int64_t ld, const double *w,
                  double *out, void *stream);

/* ---------------------------------------------------------------------------------
 * a4/a5  electron-exchange-symmetry codecs (electron_integral_utils.py:38-66, 69-88)
 *   pack  : (n,n,n,n) -> row-major lower triangle of the (n^2,n^2) matrix, diagonal * diag_mult;
 *           elements [M, out_len) of `out` are zero-filled (padding for the streaming GEMV).
 *   unpack: (M,) -> (n,n,n,n), both triangles.
 * Out of place (the reference scales the caller's diagonal in place and restores it).
 * --------------------------------------------------------------------------------- */
int evc_pack_pair_sym(const double *h2, int n, double diag_mult, double *out, int64_t out_len,
                      void *stream);
int evc_unpack_pair_sym(const double *packed, int n, double *out, void *stream);

/* ---------------------------------------------------------------------------------
 * K3/K14  four-index basis rotation, FP64 MFMA (v_mfma_f64_16x16x4_f64)
 *   quarter step: out[q, a,b,c] = sum_d in[a,b,c,d] * C[d,q]     (c_transposed == 0)
 *                                 sum_d in[a,b,c,d] * C[q,d]     (c_transposed != 0)
 *   i.e. the LAST index is rotated and moved to the FRONT; four steps rotate all four
 *   indices and restore their order.
 *   full: out[i,j,k,l] = sum_abcd in[a,b,c,d] C[a,i] C[b,j] C[c,k] C[d,l]
 *   replaces pyscf.ao2mo.kernel + ao2mo.restore(1,..) (electron_integral_utils.py:136,
 *   ab_initio_gradients_loewdin.py:339) and the OAO->AO back-rotation of the 2-RDM (:224-232,
 *   with c_transposed=1).  If `three_quarter` is non-NULL it receives the tensor after three
 *   steps, K[j,k,l,a] = sum_bcd in[a,b,c,d] C[b,j] C[c,k] C[d,l]  (used by K13, :210-222).
 *   `tmp` is scratch of n^4 doubles; in/out/tmp/three_quarter must not alias.  n <= 96.
 * --------------------------------------------------------------------------------- */
int evc_quarter_transform(const double *in, const double *C, int c_transposed, int n,
                          double *out, void *stream);
int evc_four_index_transform(const double *in, const double *C, int c_transposed, int n,
                             double *out, double *tmp, double *three_quarter, void *stream);

/* ---------------------------------------------------------------------------------
 * K1/K2  Loewdin orthogonalisation, one workgroup per matrix.  n <= 32: eigensolver started in FP32 (tridiagonal or
 *        one-sided Jacobi on one wave) and refined in FP64; 32 < n <= 64: one-sided Jacobi on 16 waves; 64 < n <= 80
 *        through this entry point (no scratch buffer): two-sided Jacobi in LDS
 *   S = U diag(s) U^T ; X = U diag(s>1e-15 ? s^-1/2 : 0) U^T ; h1 = X^T hcore X
 *   replaces get_loewdin_trafo (electron_integral_utils.py:6-18) and the h1 rotation
 *   (:135, ab_initio_gradients_loewdin.py:338).  hcore/h1 may be NULL.  n <= 80 (96 inside the fused pipeline, which lends
 *   the kernel scratch from its workspace).
 * --------------------------------------------------------------------------------- */
int evc_loewdin(const double *S, const double *hcore, int n, double *X, double *U, double *s,
                double *h1, void *stream);

/* ---------------------------------------------------------------------------------
 * K6  subspace generalised eigenproblem H c = E S c on one workgroup
 *   H is assembled from the one-body part h1rows (T*T) and the two-body rows
 *   (rows2 = T*T or T(T+1)/2 values, already scaled) exactly as
 *   ab_initio_eigenvector_continuation.py:38-68 does, then solved like scipy.linalg.eigh(H,S)
 *   (LAPACK dsygvd: lower triangles, Cholesky of S, c^T S c = 1) (:73-88, :157-173).
 *   Outputs: evals[nroots] ascending (+ e_shift), evecs[nroots*T] (row k = k-th vector),
 *   w2[rows2] / w1[T*T]: weights of the two-/one-body t-RDM rows for the predicted RDMs of
 *   root 0 (ab_initio_gradients_loewdin.py:343-356), Hout[T*T] (may be NULL): the matrix handed
 *   to the eigensolver.  Hermitian branch only.
 *   T <= 512 (the reference has no bound: its Zundel learning curve uses 80 and 100 training states,
 *   scripts/MD/Zundel_thermodynamics/continuation/05_Zundel_test_potential_energy.py:182-210).  T <= 32 runs in the
 *   registers / LDS of one 256-thread workgroup and needs no workspace (ws may be NULL); larger T run on a 1024-thread
 *   workgroup with one T x T matrix in LDS (T <= 128; in global memory beyond) and need `ws` of
 *   evc_subspace_solve_ws_bytes(T, count) bytes, 16-byte aligned.
 * --------------------------------------------------------------------------------- */
size_t evc_subspace_solve_ws_bytes(int T, int count);
int evc_subspace_solve(const double *h1rows, const double *h2rows, const double *S_train, int T,
                       int layout, int nroots, double e_shift, double *evals, double *evecs,
                       double *w2, double *w1, double *Hout, void *ws, size_t ws_bytes, void *stream);
/* `count` independent problems H[g] c = E S[g] c of one size (one workgroup each): H (count,T,T) and
 * S (T,T) shared (s_stride = 0) or (count,T,T) (s_stride = T*T), lower triangles read.  Writes
 * evals (count,T) (first nroots of each row, + e_shift[g] if e_shift != NULL) and evecs (count,T,T).
 * This is what the active-learning loop needs: the continuation energies of a trajectory for SUBSETS
 * of the training set (MD_utils.py:264-299,448-483) are eigenproblems of sub-matrices of the one
 * H(R) of the full set, so the t-RDM is contracted once per geometry, not once per subset. */
int evc_subspace_solve_batch(const double *H, const double *S, int64_t s_stride, int T, int count,
                             int nroots, const double *e_shift, double *evals, double *evecs,
                             void *ws, size_t ws_bytes, void *stream);

/* OAO integrals of `count` geometries (get_basis + get_integrals, electron_integral_utils.py:91-138):
 * X = S^-1/2, h1 = X^T hcore X (count,N,N), h2 = four-index rotation of eri (count,N,N,N,N); `trafo`
 * (count,N,N) receives X if non-NULL.  Inputs stacked along the leading axis.  Used by the
 * "farthest_point_ham" selection metric (MD_utils.py:363-405).  n <= 96. */
size_t evc_integrals_oao_ws_bytes(int n, int count);
int evc_integrals_oao_batch(int n, int count, const double *S, const double *hcore, const double *eri,
                            double *h1, double *h2, double *trafo, void *ws, size_t ws_bytes,
                            void *stream);

/* ---------------------------------------------------------------------------------
 * Fused per-geometry pipeline (ab_initio_gradients_loewdin.py:308-379 get_energy_with_grad,
 * ab_initio_eigenvector_continuation.py:178-250 *_OAO)
 * --------------------------------------------------------------------------------- */
typedef struct evc_trdm_set {
    int32_t n;           /* orbitals N (<= 96; the reference's largest orbital space is 58) */
    int32_t ntrain;      /* training states T (<= 512) */
    int32_t layout;      /* EVC_LAYOUT_* */
    int32_t reserved;
    int64_t rows2;       /* rows of the two-body matrix view held by THIS rank */
    int64_t row_offset;  /* index of the first local row in the global row numbering */
    int64_t rows2_total; /* global number of rows (T*T or T(T+1)/2) */
    int64_t cols2;       /* N^4 or M */
    int64_t ld2;         /* leading dimension of two_rdm (even, >= cols2) */
    int64_t ld1;         /* leading dimension of one_rdm (even, >= N*N) */
    const double *two_rdm; /* (rows2, ld2) */
    const double *one_rdm; /* (T*T, ld1), replicated on every rank */
    const double *s_train; /* (T,T) */
} evc_trdm_set;

typedef struct evc_geometry {
    int32_t natm;
    int32_t reserved;
    double enuc;             /* mol.energy_nuc() */
    const double *S;         /* (N,N)       int1e_ovlp */
    const double *hcore;     /* (N,N)       scf.hf.get_hcore */
    const double *eri;       /* (N,N,N,N)   int2e; 16-byte aligned (as eri_ip1) */
    const double *ipovlp;    /* (3,N,N)     int1e_ipovlp             (NULL: energy only) */
    const double *dhcore;    /* (A,3,N,N)   hcore_generator()(atom)  (NULL: energy only) */
    const double *eri_ip1;   /* (3,N,N,N,N) int2e_ip1                (NULL: energy only) */
    const double *gnuc;      /* (A,3)       grad_nuc()               (NULL: energy only) */
    const int64_t *aoslices; /* (A,2) [start,stop)                   (NULL: energy only) */
} evc_geometry;

typedef struct evc_outputs {
    double *energy;  /* [nroots]  total energies (electronic + enuc) */
    double *coeffs;  /* [nroots*T] */
    double *grad;    /* [A*3] or NULL */
    double *d_pred;  /* [N*N]  predicted 1-RDM (always written by the gradient phase) */
    double *g_pred;  /* [N^4]  predicted 2-RDM, unpacked; may be NULL (for the packed layouts the gradient
                        phase then never materialises it) */
    double *hmat;    /* [T*T] or NULL: matrix handed to the eigensolver */
} evc_outputs;

/* flags */
#define EVC_FLAG_ENERGY_ONLY 1  /* stop after the eigensolve */
#define EVC_FLAG_PARTIAL_RANK 2 /* multi-GPU: this rank is not rank 0 -> its partial gradient carries
                                   only the two-body contribution of its rows */
#define EVC_FLAG_WARM_START 4   /* the workspace holds the results of a previous evaluation at a NEARBY geometry
                                   (an MD step): the two Jacobi eigensolvers (overlap matrix, subspace problem) start
                                   from its eigenvectors and converge in 2-3 sweeps instead of 7-8.  Results agree
                                   with a cold start to solver tolerance (~1e-14), not bit for bit; stale or
                                   never-written eigenvectors are detected and ignored.  Fused entry points only. */

#define EVC_FLAG_IP1_S2KL 8     /* geometry.eri_ip1 is (3,N,N,N(N+1)/2) [per geometry of a batch]: int2e_ip1 packed in its
                                   last two AO indices, element (x,p,q,k(k+1)/2+l), k >= l -- what PySCF returns for
                                   mol.intor("int2e_ip1", aosym="s2kl").  Half the bytes of the largest input; the
                                   contraction then streams dense rows.  Only with EVC_LAYOUT_SYM8 and N <= 64 (the
                                   path that uses the r <-> s symmetry of int2e_ip1 anyway; beyond 32 orbitals
                                   together with EVC_FLAG_ERI_S4). */
#define EVC_FLAG_ERI_S4 16      /* geometry.eri is the dense (Ms,Ms) matrix, Ms = N(N+1)/2 [per geometry of a batch]: int2e
                                   packed in both index pairs, element (p(p+1)/2+q, r(r+1)/2+s), p >= q, r >= s -- what PySCF
                                   returns for mol.intor("int2e", aosym="s4").  A quarter of the bytes.  Fused entry points,
                                   EVC_LAYOUT_SYM8 and N <= 64 only. */

#define EVC_FLAG_LOEWDIN_DONE 32 /* the workspace already holds X, U, s and h1 of THESE geometries (evc_phase_loewdin_batch
                                   ran on it): phase A skips the Loewdin kernel.  Lets a host overlap that latency-bound
                                   kernel -- it reads only S and hcore -- with the upload of the large integral arrays
                                   (hosted MD) or with the previous batch's streaming kernels (throughput).  Batch entry
                                   points only. */

/* The workspace also caches the inverse Cholesky factor of t->s_train next to the matrix it was computed from; a call
 * whose s_train is bit-identical to that copy reuses the factor.  ZERO-FILL a workspace once after allocating it (the
 * Python layer does): a recycled allocation must not look like a hit. */
size_t evc_workspace_bytes(const evc_trdm_set *t, int natm);

/* Phase A: Loewdin + integrals + H rows.  Writes h2rows_local[rows2] (scaled two-body rows of this
 * rank) and h1rows[T*T] into the workspace; pointers are returned through the out arguments so a
 * multi-GPU host can all-gather the rows between the phases.
 * flags: EVC_FLAG_ERI_S4 (g->eri packed), EVC_FLAG_WARM_START. */
int evc_phase_hamiltonian(const evc_trdm_set *t, const evc_geometry *g, int flags, void *ws, size_t ws_bytes,
                          double **h2rows_local, double **h1rows, void *stream);
/* Phase B: eigensolve from the complete row vector h2rows_all[rows2_total].  flags: EVC_FLAG_WARM_START. */
int evc_phase_solve(const evc_trdm_set *t, const evc_geometry *g, const double *h2rows_all,
                    const evc_outputs *out, int nroots, int flags, void *ws, size_t ws_bytes, void *stream);
/* Phase C: predicted RDMs of root 0 + Loewdin-response nuclear gradient (other roots: evc_phase_gradient_roots). */
int evc_phase_gradient(const evc_trdm_set *t, const evc_geometry *g, const evc_outputs *out,
                       int flags, void *ws, size_t ws_bytes, void *stream);
/* Between B and C, optional: replace the row weights phase B left in the workspace by those of a coefficient vector
 * the CALLER supplies (coeffs[T], device): w1 = c c^T, two-body rows 2 c_a c_b / c_a^2 (pair layouts) or c_a c_b
 * (ab_initio_gradients_loewdin.py:343-356).  This is how hermitian=False is served: the T x T pencil (outputs.hmat of
 * phase B) is solved by scipy.linalg.eig on the host, exactly as the reference does (:76-88), and phase C then builds
 * the predicted RDMs and the gradient from ITS eigenvector.  `natm` as passed to evc_workspace_bytes. */
int evc_phase_set_coeffs(const evc_trdm_set *t, const double *coeffs, int natm, void *ws, size_t ws_bytes,
                         void *stream);
/* Phase C for several roots of ONE geometry in one pass: forces on excited-state surfaces and interstate couplings.
 * The overlap matrix of the training states does not depend on the geometry, so for every eigenpair of H c = E S c
 * (c^T S c = 1) dE_k/dR = c_k^T (dH/dR) c_k (ab_initio_gradients_loewdin.py:341-379 with c_k in place of c_0), and the
 * interstate coupling vector h_kl = c_k^T (dH/dR) c_l is the same functional of the symmetric weighting
 * W = (c_k c_l^T + c_l c_k^T) / 2 (the gradient is linear in the predicted RDMs).  The derivative coupling is
 * h_kl / (E_l - E_k); dividing by the gap is the caller's business.
 *
 * Slot p of the call evaluates the pair (k, l) = (pairs[2p], pairs[2p+1]) of rows of coeffs (nvec, T), device: every
 * stage of the gradient chain covers all slots in one launch, and the t-RDM is streamed once per 32 slots (the batched
 * K8 of evc_energy_with_grad_batch) instead of once per root.
 *   pairs   HOST array (npairs, 2), 0 <= k <= l < nvec, 1 <= npairs <= 4096; nvec <= T.
 *   ws      at least evc_workspace_bytes_roots(t, natm, npairs) bytes; slot 0 holds phases A+B of THIS geometry: the
 *           state an evc_energy_with_grad(..., nroots, EVC_FLAG_ENERGY_ONLY, ...) call (or evc_phase_hamiltonian +
 *           evc_phase_solve) on the same workspace leaves.  Hermitian branch: coeffs = that call's outputs.coeffs;
 *           hermitian=False: the caller's host-solved eigenvectors.  The call overwrites slots 1 .. npairs-1 (and the
 *           row weights of slot 0).
 *   flags   EVC_FLAG_IP1_S2KL only (as for evc_phase_gradient); EVC_FLAG_PARTIAL_RANK is rejected.
 * WARNING: at (near-)degenerate roots the eigenvectors are not unique; the forces and couplings then follow whichever
 * eigenvectors the solver returned (no degeneracy treatment). */
typedef struct evc_outputs_roots {
    double *grad;    /* (npairs,A,3): slot (k,k) = total gradient of root k (electronic + grad_nuc);
                        slot (k,l), k != l = electronic coupling vector c_k^T dH/dR c_l (no nuclear term) */
    double *d_pred;  /* (npairs,N,N) or NULL: predicted (transition) 1-RDM of the slot's weighting */
    double *g_pred;  /* (npairs,N^4) or NULL: predicted 2-RDM, unpacked, as for evc_outputs.g_pred */
} evc_outputs_roots;

size_t evc_workspace_bytes_roots(const evc_trdm_set *t, int natm, int npairs);
int evc_phase_gradient_roots(const evc_trdm_set *t, const evc_geometry *g, const double *coeffs, int nvec,
                             const int32_t *pairs, int npairs, const evc_outputs_roots *out, int flags, void *ws,
                             size_t ws_bytes, void *stream);
/* A+B(+C) back to back on one device. */
int evc_energy_with_grad(const evc_trdm_set *t, const evc_geometry *g, const evc_outputs *out,
                         int nroots, int flags, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * Batched form: `count` independent geometries of the SAME molecule (same N, A, aoslices) per call.
 * Every launch of the pipeline covers the whole batch, and the two streaming kernels read the
 * t-RDM ONCE for up to 32 geometries (K5 becomes (rows,cols)x(cols,G), K8 (G,rows)x(rows,cols)),
 * so the HBM cost of the t-RDM per evaluation drops by the batch size.  This is the throughput
 * form for PES scans / batched re-evaluations; an MD run is count = 1.
 * All arrays are stacked along a leading batch axis, C order.
 * --------------------------------------------------------------------------------- */
typedef struct evc_geometry_batch {
    int32_t natm;
    int32_t count;
    const double *enuc;      /* (count)           mol.energy_nuc() per geometry, DEVICE array */
    const double *S;         /* (count,N,N) */
    const double *hcore;     /* (count,N,N) */
    const double *eri;       /* (count,N,N,N,N) */
    const double *ipovlp;    /* (count,3,N,N)       (NULL: energy only) */
    const double *dhcore;    /* (count,A,3,N,N)     (NULL: energy only) */
    const double *eri_ip1;   /* (count,3,N,N,N,N)   (NULL: energy only) */
    const double *gnuc;      /* (count,A,3)         (NULL: energy only) */
    const int64_t *aoslices; /* (A,2) shared by the batch */
} evc_geometry_batch;

typedef struct evc_outputs_batch {
    double *energy;  /* (count,T)    first nroots entries of each row are written */
    double *coeffs;  /* (count,T,T)  first nroots rows of each block are written */
    double *grad;    /* (count,A,3) or NULL with EVC_FLAG_ENERGY_ONLY */
    double *d_pred;  /* (count,N,N) or NULL (kept in the workspace) */
    double *g_pred;  /* (count,N,N,N,N) or NULL (kept in the workspace) */
    double *hmat;    /* (count,T,T) or NULL */
} evc_outputs_batch;

size_t evc_workspace_bytes_batch(const evc_trdm_set *t, int natm, int count);
/* The full calls (evc_energy_with_grad, evc_energy_with_grad_batch) compute the Loewdin transformation X = S^-1/2
 * (electron_integral_utils.py:6-18) by a Newton-Schulz iteration and keep the eigendecomposition of S, which only the
 * response term of the gradient needs (ab_initio_gradients_loewdin.py:41-134,300-303), off the critical path: for
 * N <= 32 and T <= 32 it rides in the launch of the subspace solve; for 33 ... 64 orbitals (or larger training sets)
 * calls of fewer than 12 geometries run it on a side stream the library creates per device, forked from and joined into
 * `stream` inside the call (two events per workspace, created at its first such call) -- the stream semantics of the
 * call are unchanged.  Before freeing a workspace that may have been used that way, hand its pointer to
 * evc_release_workspace: it waits for the last such launch into the workspace and destroys the events (a pointer that
 * owns none: no-op, returns 0).  EVC_LOEWDIN_SPLIT=0: one Loewdin kernel always. */
int evc_release_workspace(void *ws);
int evc_energy_with_grad_batch(const evc_trdm_set *t, const evc_geometry_batch *gb,
                               const evc_outputs_batch *ob, int nroots, int flags, void *ws,
                               size_t ws_bytes, void *stream);

/* Phase C of evc_phase_gradient_roots for EVERY geometry of a batch in one pass: the same host list of root pairs
 * (k, l) for each of the gb->count geometries.  Slot (k,k) = total gradient of root k, slot (k,l), k != l = electronic
 * coupling vector c_k^T dH/dR c_l of that geometry (semantics, degeneracy warning: evc_phase_gradient_roots).
 *   coeffs  DEVICE (count,T,T), as evc_energy_with_grad_batch writes outputs.coeffs: rows 0 .. nvec-1 of block g are
 *           the coefficient vectors of geometry g (hermitian=False: the caller's host-solved eigenvectors, same layout).
 *   pairs   HOST array (npairs, 2), 0 <= k <= l < nvec; 1 <= count * npairs <= 4096; nvec <= T.
 *   ws      at least evc_workspace_bytes_roots_batch(t, natm, count, npairs) bytes; geometries 0 .. count-1 of it hold
 *           phases A+B of THESE geometries: the state evc_energy_with_grad_batch(..., nroots >= nvec,
 *           EVC_FLAG_ENERGY_ONLY, ...) (or evc_phase_hamiltonian_batch + evc_phase_solve_batch) on the same workspace
 *           leaves.  The call overwrites the slots behind them (and the row weights of the first count).
 *   flags   EVC_FLAG_IP1_S2KL only; EVC_FLAG_PARTIAL_RANK is rejected.
 * Outputs (evc_outputs_roots) are ROOT-PAIR-MAJOR: grad (npairs,count,A,3), d_pred (npairs,count,N,N) or NULL,
 * g_pred (npairs,count,N^4) or NULL -- entry [p][g] is pair p of geometry g.
 * The slots s = p * count + g go through the gradient chain of the batch entry points together (the t-RDM is streamed
 * once per 32 slots); on the packed int2e_ip1 route (EVC_FLAG_IP1_S2KL) each geometry's int2e_ip1 is read once per up
 * to 8 of its root pairs. */
size_t evc_workspace_bytes_roots_batch(const evc_trdm_set *t, int natm, int count, int npairs);
int evc_phase_gradient_roots_batch(const evc_trdm_set *t, const evc_geometry_batch *gb, const double *coeffs, int nvec,
                                   const int32_t *pairs, int npairs, const evc_outputs_roots *out, int flags, void *ws,
                                   size_t ws_bytes, void *stream);

/* Phase L: Loewdin orthogonalisation of the batch alone (electron_integral_utils.py:6-18,135): reads gb->S and
 * gb->hcore only, leaves X, U, s, h1 in the workspace for a following call with EVC_FLAG_LOEWDIN_DONE.
 * flags: EVC_FLAG_WARM_START. */
int evc_phase_loewdin_batch(const evc_trdm_set *t, const evc_geometry_batch *gb, int flags, void *ws, size_t ws_bytes,
                            void *stream);

/* The three phases of the pair-sharded evaluation for a batch (t may hold a row slice).
 * A: writes the scaled two-body rows of this rank to rows_out[g*ld_rows_out + r], r < t->rows2
 *    (caller's buffer: the send buffer of the all-gather).  flags: EVC_FLAG_ERI_S4 (gb->eri packed: the phases then
 *    run the same symmetric pipeline as the fused entry point), EVC_FLAG_LOEWDIN_DONE, EVC_FLAG_WARM_START.
 * B: h2rows_all[g*ld_rows_all + p], p < t->rows2_total, is the gathered row vector of geometry g.
 *    flags: EVC_FLAG_WARM_START.
 * C: as evc_phase_gradient; with EVC_FLAG_PARTIAL_RANK ob->grad receives only the two-body share;
 *    EVC_FLAG_IP1_S2KL as for the fused entry point. */
int evc_phase_hamiltonian_batch(const evc_trdm_set *t, const evc_geometry_batch *gb, int flags, double *rows_out,
                                int64_t ld_rows_out, void *ws, size_t ws_bytes, void *stream);
int evc_phase_solve_batch(const evc_trdm_set *t, const evc_geometry_batch *gb, const double *h2rows_all,
                          int64_t ld_rows_all, const evc_outputs_batch *ob, int nroots, int flags, void *ws,
                          size_t ws_bytes, void *stream);
int evc_phase_gradient_batch(const evc_trdm_set *t, const evc_geometry_batch *gb,
                             const evc_outputs_batch *ob, int flags, void *ws, size_t ws_bytes,
                             void *stream);

/* Gradient of given (not predicted) RDMs: get_grad_elec_OAO (ab_initio_gradients_loewdin.py:255-305).
 * `trafo` = caller's ao_mo_trafo (N,N) or NULL for the Loewdin trafo of g->S; the trafo derivative is
 * the Loewdin response of g->S in both cases (:274-277).  Writes the ELECTRONIC gradient (no grad_nuc)
 * to grad[A*3]. */
int evc_grad_elec_oao(int n, const evc_geometry *g, const double *trafo, const double *one_rdm,
                      const double *two_rdm, double *grad, void *ws, size_t ws_bytes, void *stream);
size_t evc_grad_elec_ws_bytes(int n, int natm);

/* ---------------------------------------------------------------------------------
 * Tensor-valued building blocks of ab_initio_gradients_loewdin.py (off the fused path, which uses
 * the adjoint form and never materialises them).  Layouts are the reference's: (N,N,N,N) and
 * (N,N,A,3), C order.  n <= 64 (evc_one_el_grad: n <= 60).
 *   evc_loewdin_trafo_grad      loewdin_trafo_grad(S)            (:41-112)  LG[p,q,a,b] = dX_pq/dS_ab(sym)
 *                               in Daleckii-Krein closed form; ws = 2n^2+n doubles
 *   evc_derivative_ao_mo_trafo  get_derivative_ao_mo_trafo(mol)  (:115-134) dX[k,l,A,x]; ws as above
 *   evc_one_el_grad             get_one_el_grad(mol, X, dX)      (:155-187) h1_jac[j,n,A,x]
 *   evc_two_el_grad             two_el_grad(h2_ao, G, X, dX, ip1, slices) (:190-252) -> (A,3)
 *   evc_contract_nnA3           out[A,x] = sum_ij T[i,j,A,x] * (transposed ? M[j,i] : M[i,j])  (:300)
 * --------------------------------------------------------------------------------- */
int evc_loewdin_trafo_grad(const double *S, int n, double *LG, double *ws, void *stream);
int evc_derivative_ao_mo_trafo(const double *S, const double *ipovlp, const int64_t *aoslices, int n,
                               int natm, double *dX, double *ws, void *stream);
int evc_one_el_grad(const double *X, const double *hcore, const double *dhcore, const double *dX, int n,
                    int natm, double *out, void *stream);
size_t evc_two_el_grad_ws_bytes(int n);
int evc_two_el_grad(const double *h2_ao, const double *two_rdm, const double *X, const double *dX,
                    const double *ip1, const int64_t *aoslices, int n, int natm, double *out, void *ws,
                    size_t ws_bytes, void *stream);
int evc_contract_nnA3(const double *T, const double *M, int transposed, int n, int natm, double *out,
                      void *stream);

/* ---------------------------------------------------------------------------------
 * Full-CI training states (fci_small.py: SmallFCI._excite_all, .trans_rdm12, .contract) for real CI vectors c[na][nb]
 * over alpha / beta occupation strings ordered by their integer value, norb <= 16, any (n_alpha, n_beta).
 *   tab_a (na, npad), tab_b (nb, npad)  DEVICE int32 string tables, npad = norb^2 rounded up to 16:
 *       tab[I * npad + p * norb + q] = +-(J + 1) where <I| a_p^+ a_q |J> = +-1, 0 where there is no such J and in the
 *       pad columns (evcont_amd/fci_tables.py builds them).
 * The determinants are split into blocks of R = max(256, ceil(dim / 256) rounded up to 64) rows; every sum over the
 * determinants is formed per block and the blocks are added in order, whatever the workspace and the number of kets:
 * results are reproducible bit for bit, and a row call equals its single-pair calls.
 *
 * evc_fci_workspace_bytes(norb, na, nb, minimal): bytes with which evc_fci_trdm_rows and evc_fci_sigma keep every
 *       intermediate of a CI vector resident (minimal = 0: one pass, the bra side of a row call formed once), or the
 *       least they accept (minimal != 0: the excitations D = E_pq c are then formed and consumed in chunks; the
 *       sigma intermediate G, norb^2 * dim doubles, is always whole).  0 on an argument error.
 * evc_fci_excite: rows k0 .. k0 + nk - 1 of D[pq](k) = (E_pq c)(k) (zero for k >= dim and in the pad columns) as
 *       EVC_FCI_DET_MAJOR    D[(k - k0) * ld + pq]           ld = npad
 *       EVC_FCI_DET_MAJOR_T  D[(k - k0) * ld + q * norb + p] ld = npad   (the bra side <E_qp bra|)
 *       EVC_FCI_ORB_MAJOR    D[pq * ld + (k - k0)]           ld >= nk, all npad rows are written
 * evc_fci_trdm_rows: one bra against nkets kets (`kets`: HOST array of nkets DEVICE pointers), conventions of
 *       SmallFCI.trans_rdm12: ovlp[i] = <bra|ket_i>, dm1[i][p][q] = <bra| q^+ p |ket_i>,
 *       dm2[i][p][q][r][s] = <bra| p^+ r^+ s q |ket_i>;  dm1 (nkets, norb^2), dm2 (nkets, norb^4), dense.
 * evc_fci_sigma: sigma = H c, H = sum h'_pq E_pq + 1/2 sum (pq|rs) E_pq E_rs, h'_pq = h1_pq - 1/2 sum_r (pr|rq);
 *       h1 (norb, norb), h2 (norb, norb, norb, norb) chemists' order, no symmetry assumed; sigma must not alias c.
 * --------------------------------------------------------------------------------- */
#define EVC_FCI_DET_MAJOR 0
#define EVC_FCI_DET_MAJOR_T 1
#define EVC_FCI_ORB_MAJOR 2
size_t evc_fci_workspace_bytes(int norb, int64_t na, int64_t nb, int minimal);
int evc_fci_excite(int norb, int64_t na, int64_t nb, const int32_t *tab_a, const int32_t *tab_b, const double *c,
                   int64_t k0, int64_t nk, int layout, double *D, int64_t ld, void *stream);
int evc_fci_trdm_rows(int norb, int64_t na, int64_t nb, const int32_t *tab_a, const int32_t *tab_b, const double *bra,
                      const double *const *kets, int nkets, double *ovlp, double *dm1, double *dm2, void *ws,
                      size_t ws_bytes, void *stream);
int evc_fci_sigma(int norb, int64_t na, int64_t nb, const int32_t *tab_a, const int32_t *tab_b, const double *h1,
                  const double *h2, const double *c, double *sigma, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * The block row call: nbras bras (1 ... 16) against shared kets.  `bras`, `kets` and `nkets_of` are HOST arrays, `bras`
 * and `kets` of DEVICE pointers.  Bra r is taken against kets[0 .. nkets_of[r] - 1]; nkets_of must not decrease, each
 * entry 1 ... 4096, and `kets` has nkets_of[nbras - 1] entries.  That covers the rectangular block (all counts equal)
 * and the triangular one (T + 1, T + 2, ..., T + R) of a training-set append, where the bras are the last kets: a bra
 * pointer may also be a ket pointer.
 * Outputs are ragged and consecutive: row off_r + i for (bra r, ket i), off_r = sum of nkets_of[r' < r]; ovlp[row],
 * dm1[row][norb^2] and dm2[row][norb^4] follow evc_fci_trdm_rows.  No output may overlap a bra or ket vector.
 * The ket-side excitations D = E_pq ket of a determinant chunk are formed once for every bra that sees the ket (the
 * bras are a dimension of the product's grid); determinant blocks, tilings and the order of the partial sums are those
 * of evc_fci_trdm_rows, so row (r, i) has the bits of evc_fci_trdm_rows(bras[r], kets[:nkets_of[r]]) row i for every
 * accepted workspace and every nbras.  evc_fci_trdm_rows is the nbras = 1 case of the same routine.
 * evc_fci_rows_block_workspace_bytes(norb, na, nb, nbras, minimal): partial sums per bra, then with minimal = 0 the
 *       bra-side D~ of all bras and one ket-side D resident, with minimal != 0 one determinant block of each; equal to
 *       evc_fci_workspace_bytes for nbras = 1, not decreasing in nbras, 0 on an argument error.
 * The stage EVC_PROF_FCI_TRDM records the single call's text followed by " bras=<nbras>".
 * --------------------------------------------------------------------------------- */
size_t evc_fci_rows_block_workspace_bytes(int norb, int64_t na, int64_t nb, int nbras, int minimal);
int evc_fci_trdm_rows_block(int norb, int64_t na, int64_t nb, const int32_t *tab_a, const int32_t *tab_b,
                            const double *const *bras, int nbras, const double *const *kets, const int *nkets_of,
                            double *ovlp, double *dm1, double *dm2, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * The row call with its two-body results written in place into the (pairs, ld) DEVICE matrix the evaluator streams
 * (evcont_amd/resident.py): the same product as evc_fci_trdm_rows (same tilings, determinant blocks and order of the
 * partial sums; ovlp and dm1 as there), then per ket the dense block dm2[p,q,r,s] goes through a scratch slot of the
 * workspace into row i of `rows` (pitch ld doubles):
 *   EVC_LAYOUT_PACK2   column R(R+1)/2 + C, R = pN+q >= C = rN+s, holds dm2[p,q,r,s] (multiplier 1);
 *   EVC_LAYOUT_SYM8    column u(u+1)/2 + v, u = i(i+1)/2+j (i >= j), v = k(k+1)/2+l (k >= l), u >= v, holds
 *                      0.125 * (((((((d0+d1)+d2)+d3)+d4)+d5)+d6)+d7) with d_m = dm2 at (i,j,k,l), (j,i,k,l), (i,j,l,k),
 *                      (j,i,l,k), (k,l,i,j), (l,k,i,j), (k,l,j,i), (l,k,j,i): the bits DeviceTRDMs.compress_sym8_ gives
 *                      for the six-index block.
 * Columns cols ... ld - 1 of the nkets rows are written as zeros; nothing else of `rows` is touched.  ld: a multiple of
 * 16, at least cols rounded up to 16, below 2^31.  Any other layout is refused.
 * evc_fci_rows_packed_workspace_bytes(norb, na, nb, minimal): evc_fci_workspace_bytes(...) plus the slot of norb^4
 *       doubles (rounded up to 256 bytes); 0 on an argument error.  Every accepted workspace gives the same bits.
 * --------------------------------------------------------------------------------- */
size_t evc_fci_rows_packed_workspace_bytes(int norb, int64_t na, int64_t nb, int minimal);
int evc_fci_trdm_rows_packed(int norb, int64_t na, int64_t nb, const int32_t *tab_a, const int32_t *tab_b,
                             const double *bra, const double *const *kets, int nkets, double *ovlp, double *dm1,
                             int layout, double *rows, int64_t ld, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * Transition RDMs between CAS states in different orbital sets (evcont_amd/cas_small.py states the reduction): the
 * active-space t-RDMs of one bra against nkets kets, as evc_fci_trdm_rows writes them for the bra's vector and the
 * rotated, scaled ket vectors, expanded into the OAO basis of n orbitals with the core contributions.  Per ket i, with
 * A = A_act[i] (n, ncas; the bra's active orbitals made orthogonal to the core of ket i, so one per ket), B = B_act[i]
 * (n, ncas), Q = Qc[i] (n, n; bra index first), S = ovlp[i]:
 *   Qa = A d1[i]^T B^T,   dm1[i] = (2 S Q + Qa)^T,
 *   dm2[p,q,r,s] = sum_tuvw d2[i][t,u,v,w] A[p,t] B[q,u] A[r,v] B[s,w]
 *                + S (4 Q[p,q] Q[r,s] - 2 Q[p,s] Q[r,q]) + 2 Q[p,q] Qa[r,s] + 2 Qa[p,q] Q[r,s] - Q[p,s] Qa[r,q] - Qa[p,s] Q[r,q]
 * Qc == NULL: no core orbitals (the Q terms are absent).  `layout`: EVC_LAYOUT_FULL6 writes the dense n^4 block of ket i
 * at rows + i * ld (ld >= n^4); EVC_LAYOUT_PACK2 / EVC_LAYOUT_SYM8 write row i in the format of evc_fci_trdm_rows_packed
 * (ld a multiple of 16, at least the layout's columns, the pad columns zero; the bits of the host codecs applied to the
 * dense block).  Any other layout is refused.  1 <= ncas <= 16, ncas <= n <= 64, 1 <= nkets <= 512, ld < 2^31; every
 * pointer a DEVICE pointer aligned to 16 bytes (ovlp is read on the device: no host synchronisation); ws_bytes >=
 * evc_cas_expand_workspace_bytes(n, ncas, nkets) (0 outside the limits).  Everything invalid is refused before any
 * launch.  The caller's stream, no allocation, no library state, no profile stage; no atomics and no split sums: the same
 * bits from run to run, and row i of a call equals the single-ket call on ket i.
 * evc_cas_expand_describe: one line per launch of an evc_cas_expand_rows call of that shape (kernel name with template
 * arguments, grid; the per-ket launches once), a pure function of its arguments.  Writes at most buf_len - 1 characters
 * and a NUL; returns the length of the whole text, -1 on an invalid argument.
 * --------------------------------------------------------------------------------- */
size_t evc_cas_expand_workspace_bytes(int n, int ncas, int nkets);
int evc_cas_expand_rows(int n, int ncas, int nkets, const double *A_act, const double *B_act, const double *Qc,
                        const double *ovlp, const double *d1, const double *d2, double *dm1, int layout, double *rows,
                        int64_t ld, void *ws, size_t ws_bytes, void *stream);
int evc_cas_expand_describe(int n, int ncas, int layout, char *buf, size_t buf_len);

/* ---------------------------------------------------------------------------------
 * Vector work of an eigensolver around evc_fci_sigma (evcont_amd/fci_davidson.py: block Davidson with the diagonal of H
 * as preconditioner) on CI vectors that stay on the device.  A set of vectors is a row-major (count, ld) DEVICE array of
 * doubles, ld >= dim = na * nb; at most 256 vectors per set and call.  Every sum over the determinants is formed per
 * block of R determinants (R as above) in a fixed order and the blocks are added in order by a second launch: the same
 * bits for every grouping of the vectors and from run to run, no atomics.
 *
 * evc_fci_solve_workspace_bytes(norb, na, nb, nvec): bytes that serve evc_fci_hdiag and every evc_fci_dots /
 *       evc_fci_davidson_correction call with at most nvec vectors per set.  0 on an argument error.
 * evc_fci_hdiag: hdiag[I] = <I|H|I> of the operator evc_fci_sigma applies (no symmetry of h2 assumed): with the
 *       occupations n_p = n_p,alpha + n_p,beta of determinant I,
 *       sum_p h'_pp n_p + 1/2 sum_pr (pp|rr) n_p n_r + 1/2 sum_{p != q} (pq|qp) sum_spin n_p,spin (1 - n_q,spin).
 * evc_fci_dots: out[i * ny + j] = X_i . Y_j (out: nx * ny DEVICE doubles).  X and Y may be the same set.
 * evc_fci_combine: Out_r = beta Out_r + sum_{j < m} coef[j * ldc + r] V_j for r < k; coef on the DEVICE; beta == 0 does
 *       not read Out; m == 0 scales Out (V and coef are then ignored).  Out must not overlap V (refused).
 * evc_fci_davidson_correction: for the k Ritz pairs (theta_r, y_r = coef[. * ldc + r]) of the basis V with W = H V,
 *       r_r = sum_j y_jr W_j - theta_r sum_j y_jr V_j, rnorm2[r] = |r_r|^2 and T_r = r_r / d, d = hdiag - theta_r with |d|
 *       floored at 1e-8 keeping its sign (d = 0 counts as +1e-8); coef, theta, rnorm2 on the DEVICE.  T must not overlap
 *       V, W or hdiag (refused).
 * --------------------------------------------------------------------------------- */
size_t evc_fci_solve_workspace_bytes(int norb, int64_t na, int64_t nb, int nvec);
int evc_fci_hdiag(int norb, int64_t na, int64_t nb, const int32_t *tab_a, const int32_t *tab_b, const double *h1,
                  const double *h2, double *hdiag, void *ws, size_t ws_bytes, void *stream);
int evc_fci_dots(int64_t dim, const double *X, int64_t ldx, int nx, const double *Y, int64_t ldy, int ny, double *out,
                 void *ws, size_t ws_bytes, void *stream);
int evc_fci_combine(int64_t dim, const double *V, int64_t ldv, int m, const double *coef, int ldc, int k, double beta,
                    double *Out, int64_t ldo, void *stream);
int evc_fci_davidson_correction(int64_t dim, const double *V, int64_t ldv, const double *W, int64_t ldw, int m,
                                const double *coef, int ldc, const double *theta, int k, const double *hdiag, double *T,
                                int64_t ldt, double *rnorm2, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * S^2 on CI vectors that stay on the device (csrc/fci_spin.hip; host statements: evcont_amd/fci_small.py
 * spin_square_vector, evcont_amd/fci_tables.py spin_square_through_tables), for the spin penalty
 * shift (S^2 - S(S+1)) of DeviceFCI(spin_penalty=...) and for <S^2> of a state.  With Sz = (n_alpha - n_beta) / 2, the
 * electron numbers read off the first string of each table, and k = Sz (Sz + 1) + n_beta:
 *       (S^2 c)[Ia, Ib] = k c[Ia, Ib] - sum_pq sgn_a sgn_b c[Ja, Jb],   Ja, sgn_a from tab_a[Ia][p norb + q],
 *                                                                       Jb, sgn_b from tab_b[Ib][q norb + p],
 *       <I|S^2|I>       = k - popcount(occ(Ia) & occ(Ib)).
 * evc_fci_spin_apply: out = beta out + alpha (S^2 c - ss c).  c and out are rows of vector sets as above (8-byte aligned
 *       DEVICE doubles, na * nb each); beta == 0 does not read out; out must not overlap c (refused).  alpha = 1, ss = 0,
 *       beta = 0 gives S^2 c; alpha = shift, ss = S(S+1), beta = 1 adds the penalty to the row evc_fci_sigma just wrote;
 *       <S^2> is this call followed by evc_fci_dots.
 * evc_fci_spin_diag: hdiag[I] += alpha (<I|S^2|I> - ss), the same penalty on the diagonal evc_fci_hdiag wrote.
 * Limits as evc_fci_hdiag: 1 <= norb <= 16, 1 <= na, nb <= 12870 (nb = 1: the table of no beta electron).  No workspace.
 * Every element is one sum in a fixed order ((k - ss) c first, pq ascending, then alpha times the sum, then beta out; no
 * fused step): the same bits from run to run, and exact on integer data.  Both leave their record on
 * EVC_PROF_FCI_SOLVE.
 * --------------------------------------------------------------------------------- */
int evc_fci_spin_apply(int norb, int64_t na, int64_t nb, const int32_t *tab_a, const int32_t *tab_b, const double *c,
                       double alpha, double ss, double beta, double *out, void *stream);
int evc_fci_spin_diag(int norb, int64_t na, int64_t nb, const int32_t *tab_a, const int32_t *tab_b, double alpha,
                      double ss, double *hdiag, void *stream);

/* ---------------------------------------------------------------------------------
 * Rotation of a CI vector under an orbital transformation (PySCF's fci.addons.transform_ci for a square u;
 * evcont_amd/fci_small.py: transform_ci).  With occ(I) the ascending occupied orbitals of string I and k electrons of a
 * spin,
 *       T[I, J] = det( u[occ(I)][:, occ(J)] )   (1 x 1 = [1] for k = 0),      out = T_a^T . c . T_b.
 * Row index of u: the old orbital, column index: the new one; nothing assumes u orthogonal.
 *   strs_a (na), strs_b (nb)  DEVICE int32 occupation masks of the strings, ascending (bit p = orbital p); may alias.
 *   u_a, u_b                  HOST doubles, (norb, norb) row-major, one per spin; may alias.
 *   c, out                    DEVICE (na, nb); out must not alias c (refused); c is not written.
 *   ws                        DEVICE workspace, 16-byte aligned, ws_bytes >= evc_fci_rotate_workspace_bytes(..., 1).
 * Minors of order k <= 8 are computed directly (LU with partial pivoting); for k >= 9 they come from the complementary
 * minors of u^-1 (Jacobi), which the entry point forms on the host: a u whose smallest pivot is below 1e-12 of its largest
 * is then refused.  T is formed in panels of columns whose width depends on na / nb alone, and no sum is split: every
 * accepted workspace gives the same bits, from run to run.
 * evc_fci_rotate_workspace_bytes(..., minimal): bytes that keep T_a, T_b and the intermediate c . T_b resident
 *       (minimal = 0), or the least accepted (minimal != 0: the intermediate and one panel of each T).  0 on an argument
 *       error.  na, nb must be the binomials C(norb, nocc_a), C(norb, nocc_b); 1 <= norb <= 16.
 * --------------------------------------------------------------------------------- */
size_t evc_fci_rotate_workspace_bytes(int norb, int nocc_a, int nocc_b, int64_t na, int64_t nb, int minimal);
int evc_fci_rotate(int norb, int nocc_a, int nocc_b, int64_t na, int64_t nb, const int32_t *strs_a,
                   const int32_t *strs_b, const double *u_a, const double *u_b, const double *c, double *out, void *ws,
                   size_t ws_bytes, void *stream);
/* evc_fci_rotate_block: nvec >= 1 vectors under one (u_a, u_b): out[v] = T_a^T . c[v] . T_b.  `c` and `out` are HOST
 *       arrays of nvec DEVICE pointers (the form evc_fci_trdm_rows takes its kets); no output may be an input or another
 *       output (refused).  Every panel of T_b and of T_a is formed once per call and applied to all vectors, 16 of them
 *       per product launch; the workspace holds one intermediate per vector.  Vector v has the bits evc_fci_rotate gives
 *       on c[v], for every accepted workspace and from run to run.  Refusals (nvec < 1, a null pointer, aliasing, a short
 *       workspace, the shape) come before any launch.  The record of EVC_PROF_FCI_ROTATE is that of evc_fci_rotate
 *       followed by " vecs=<nvec>".
 * evc_fci_rotate_block_workspace_bytes(..., nvec, minimal): as evc_fci_rotate_workspace_bytes with nvec intermediates;
 *       0 on an argument error. */
size_t evc_fci_rotate_block_workspace_bytes(int norb, int nocc_a, int nocc_b, int64_t na, int64_t nb, int nvec,
                                            int minimal);
int evc_fci_rotate_block(int norb, int nocc_a, int nocc_b, int64_t na, int64_t nb, const int32_t *strs_a,
                         const int32_t *strs_b, const double *u_a, const double *u_b, int nvec, const double *const *c,
                         double *const *out, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * AO integrals of s-Gaussian molecules on the device (csrc/sgto.hip; the host statement is evcont_amd/hchain.py
 * s_gaussian_mol): one contracted s function per centre, the same contraction of nprim primitives on every centre, real
 * nuclear charges.  One call writes every array of an evc_geometry_batch for `count` geometries, in the layout the
 * evaluator reads, so a dynamics step stays on the device from coordinates to forces.
 *   coords        DEVICE (count, natm, 3), Bohr.          charges       DEVICE (natm).
 *   exponents, coefficients   HOST (nprim): exponents (> 0) and contraction coefficients of NORMALISED primitives; they
 *                 reach the kernels by value.
 *   out           every pointer DEVICE and writable, shapes as in evc_geometry_batch (N = natm); ipovlp, dhcore, eri_ip1
 *                 and gnuc may be NULL with EVC_FLAG_ENERGY_ONLY and are then not written.
 *   flags         EVC_FLAG_ENERGY_ONLY (S, hcore, eri, enuc only), EVC_FLAG_ERI_S4 (eri is (count, Ms, Ms), Ms = N(N+1)/2),
 *                 EVC_FLAG_IP1_S2KL (eri_ip1 is (count, 3, N, N, Ms)); the packed forms need natm <= 64.  Any other flag is
 *                 refused.
 *   ws            DEVICE workspace (the primitive-pair table), 16-byte aligned, at least evc_sgto_workspace_bytes(...).
 * Limits: 1 <= natm <= 96, 1 <= nprim <= 8, 1 <= count <= 65535.  A null required pointer, a shape outside the limits, an
 * unknown flag, a non-positive exponent or a workspace that is too small is refused before anything is launched (rc < 0,
 * evc_last_error).  Caller's stream, no allocation, no library state; nothing but the output arrays and the workspace
 * is written.  No sum is split and there are no atomics: the same bits from run to run, for every batch size (geometry g
 * of a batch = the call on it alone), and the full forms are the unpacked packed forms; eri with EVC_FLAG_ENERGY_ONLY has
 * the bits of eri without it.  S and hcore are exactly symmetric.  No primitive quartet is screened.
 * evc_sgto_workspace_bytes: 0 on a shape outside the limits.
 * --------------------------------------------------------------------------------- */
typedef struct evc_sgto_outputs {
    double *enuc;    /* (count) */
    double *S;       /* (count,N,N) */
    double *hcore;   /* (count,N,N) */
    double *eri;     /* (count,N,N,N,N), or (count,Ms,Ms) with EVC_FLAG_ERI_S4 */
    double *ipovlp;  /* (count,3,N,N) */
    double *dhcore;  /* (count,A,3,N,N) */
    double *eri_ip1; /* (count,3,N,N,N,N), or (count,3,N,N,Ms) with EVC_FLAG_IP1_S2KL */
    double *gnuc;    /* (count,A,3) */
} evc_sgto_outputs;
size_t evc_sgto_workspace_bytes(int natm, int nprim, int count);
int evc_sgto_integrals_batch(int natm, int nprim, int count, const double *coords, const double *charges,
                             const double *exponents, const double *coefficients, const evc_sgto_outputs *out, int flags,
                             void *ws, size_t ws_bytes, void *stream);
/* The AO dipole integrals of the same molecules, the one integral the call above does not produce (csrc/properties.hip;
 * host statement: HChainMol.dipole_integrals): dip (count,3,N,N) = <mu| r - origin |nu>; per primitive pair
 * (P - origin) S_prim with P as in s_gaussian_mol (on coincident coordinates the centre exactly).  coords DEVICE
 * (count,natm,3); ex, co, origin HOST; limits and refusals of evc_sgto_integrals_batch (natm <= 96, nprim <= 8, positive
 * exponents).  One sum per element over the primitive pairs in ascending order, mirrored: exactly symmetric, the same
 * bits from run to run and for every batch size. */
int evc_sgto_dipole_batch(int natm, int nprim, int count, const double *coords, const double *ex, const double *co,
                          const double origin[3], double *dip, void *stream);

/* ---------------------------------------------------------------------------------
 * AO integrals of molecules of contracted Cartesian s and p Gaussian shells on the device (csrc/spgto.hip; the host
 * statement is evcont_amd/gto_small.py sp_gaussian_mol): water, Zundel, ... in STO-3G or 6-31G from the coordinates.  One
 * call writes every array of an evc_geometry_batch for `count` geometries (N = the number of contracted functions, A =
 * natm), into the evc_sgto_outputs of evc_sgto_integrals_batch, with its flags and forms.  AO order: shells in the given
 * order, a p shell as x, y, z.  dhcore: the operator term of nucleus A plus the rows and columns of all functions on A.
 *   coords        DEVICE (count, natm, 3), Bohr.          charges       DEVICE (natm).
 *   shell_atom, shell_l, shell_prim_offset, exponents, coefficients   HOST: per shell its centre (ascending), l (0 or 1)
 *                 and the range [shell_prim_offset[s], shell_prim_offset[s+1]) of its primitives (offset[0] = 0; nshell+1
 *                 entries) in exponents (> 0) / coefficients (of NORMALISED primitives, used as given: a caller that wants
 *                 contracted functions of unit norm scales them beforehand).  They reach the kernels by value.
 *   flags         EVC_FLAG_ENERGY_ONLY, EVC_FLAG_ERI_S4, EVC_FLAG_IP1_S2KL as for evc_sgto_integrals_batch; any other flag
 *                 is refused.
 *   ws            DEVICE workspace (the primitive-pair table), 16-byte aligned, at least
 *                 evc_spgto_workspace_bytes(natm, nshell, nprim_total, nao, count).
 * Limits: l <= 1, 1 <= natm <= 64, nao <= 64, 1 ... 8 primitives per shell, at most 128 primitives in all,
 * 1 <= count <= 65535.  A null required pointer, a shape outside the limits, an l outside {0, 1}, a shell_atom out of
 * range or not ascending, a non-positive exponent, an unknown flag or a workspace that is too small or misaligned is
 * refused before anything is launched (rc < 0, evc_last_error names the function).  Caller's stream, no allocation, no
 * library state; nothing but the output arrays and the workspace is written.  No sum is split between threads: the same
 * bits from run to run and for every batch size (geometry g of a batch = the call on it alone), and the full forms are
 * the unpacked packed forms.  S and hcore are exactly symmetric, eri within each index pair, dhcore in its last two
 * indices.  No primitive quartet is screened.  eri with EVC_FLAG_ENERGY_ONLY need NOT have the bits of eri without it (the
 * two use Boys functions of different highest order); they agree to rounding.
 * evc_spgto_workspace_bytes: 0 (and a message) on a shape outside the limits.
 * evc_spgto_dipole_batch: dip (count,3,N,N) = <mu| r - origin |nu> of the same molecules; origin HOST; needs no workspace;
 * one sum per element over the primitive pairs in ascending order, mirrored: exactly symmetric.
 * --------------------------------------------------------------------------------- */
size_t evc_spgto_workspace_bytes(int natm, int nshell, int nprim_total, int nao, int count);
int evc_spgto_integrals_batch(int natm, int nshell, int count, const double *coords, const double *charges,
                              const int *shell_atom, const int *shell_l, const int *shell_prim_offset,
                              const double *exponents, const double *coefficients, const evc_sgto_outputs *out, int flags,
                              void *ws, size_t ws_bytes, void *stream);
int evc_spgto_dipole_batch(int natm, int nshell, int count, const double *coords, const int *shell_atom,
                           const int *shell_l, const int *shell_prim_offset, const double *exponents,
                           const double *coefficients, const double origin[3], double *dip, void *stream);

/* ---------------------------------------------------------------------------------
 * AO integrals of molecules of contracted s, p and REAL SPHERICAL d Gaussian shells on the device (csrc/spdgto.hip; the
 * host statement is evcont_amd/gto_spd.py spd_gaussian_mol): water in cc-pVDZ from the coordinates.  The argument lists,
 * the outputs (evc_sgto_outputs), the three flags, the forms and the guarantees are those of the evc_spgto_* calls above;
 * shell_l may be 0, 1 or 2.  AO order: shells in the given order, a p shell as x, y, z, a d shell as its five real
 * spherical functions in the order m = -2 ... 2: xy, yz, 2z^2 - x^2 - y^2, xz, x^2 - y^2, each of the norm of the
 * normalised primitive x y exp(-a r^2) times its coefficient (the Cartesian combination x^2 + y^2 + z^2 never appears).
 * Limits: l <= 2, 1 <= natm <= 64, nao <= 64 (2l + 1 functions per shell), 1 ... 8 primitives per shell, at most 128
 * primitives in all, 1 <= count <= 65535; contractions are segmented (a generally contracted table repeats its
 * primitives).  A null required pointer (the gradient outputs are required unless EVC_FLAG_ENERGY_ONLY), a shape outside
 * the limits, an l outside {0, 1, 2}, a shell_atom out of range or not ascending, a bad shell_prim_offset, a non-positive
 * exponent, an unknown flag or a workspace that is too small or misaligned is refused before anything is launched
 * (rc < 0, evc_last_error names the function).  A nucleus without functions is allowed.  Caller's stream, no allocation,
 * no library state.  Molecules of s and p shells alone are served by both families; evc_spgto_* is the faster route for
 * them and the two need not agree in the last bits.
 * --------------------------------------------------------------------------------- */
size_t evc_spdgto_workspace_bytes(int natm, int nshell, int nprim_total, int nao, int count);
int evc_spdgto_integrals_batch(int natm, int nshell, int count, const double *coords, const double *charges,
                               const int *shell_atom, const int *shell_l, const int *shell_prim_offset,
                               const double *exponents, const double *coefficients, const evc_sgto_outputs *out, int flags,
                               void *ws, size_t ws_bytes, void *stream);
int evc_spdgto_dipole_batch(int natm, int nshell, int count, const double *coords, const int *shell_atom,
                            const int *shell_l, const int *shell_prim_offset, const double *exponents,
                            const double *coefficients, const double origin[3], double *dip, void *stream);

/* ---------------------------------------------------------------------------------
 * AO integrals of molecules of contracted s, p, REAL SPHERICAL d and REAL SPHERICAL f Gaussian shells on the device
 * (csrc/spdfgto.hip; the host statement is evcont_amd/gto_spdf.py spdf_gaussian_mol): the shape of water in cc-pVTZ from
 * the coordinates.  The argument lists, the outputs (evc_sgto_outputs), the three flags, the forms, the refusals and the
 * guarantees are those of the evc_spdgto_* calls above; shell_l may be 0, 1, 2 or 3 and nao counts 2l + 1 functions per
 * shell (at most 7 nshell, at most 64).  AO order: an f shell as its seven real spherical functions in the order
 * m = -3 ... 3: y(3x^2 - y^2)/sqrt(24), xyz, y(4z^2 - x^2 - y^2)/sqrt(40), z(2z^2 - 3x^2 - 3y^2)/sqrt(60),
 * x(4z^2 - x^2 - y^2)/sqrt(40), z(x^2 - y^2)/2, x(x^2 - 3y^2)/sqrt(24), each times the norm of the normalised primitive
 * x y z exp(-a r^2) and its coefficient.  The two-electron kernel runs a body specialised on the highest l of the bra
 * pair and of the ket pair of an element; which body computes an element depends on the basis alone, so the same bits
 * come out from run to run, for every batch size and in the packed and full forms.  Molecules with l <= 2 are served by
 * both families and the two need not agree in the last bits.
 * evc_spdfgto_dipole_grad_batch: ipdip[g,x,c,mu,nu] = <d_x mu| r_c - origin_c |nu> of these molecules, with the argument
 * list, the alignment rule and the refusals of evc_gto_dipole_grad_batch (which stops at l = 2).
 * --------------------------------------------------------------------------------- */
size_t evc_spdfgto_workspace_bytes(int natm, int nshell, int nprim_total, int nao, int count);
int evc_spdfgto_integrals_batch(int natm, int nshell, int count, const double *coords, const double *charges,
                                const int *shell_atom, const int *shell_l, const int *shell_prim_offset,
                                const double *exponents, const double *coefficients, const evc_sgto_outputs *out, int flags,
                                void *ws, size_t ws_bytes, void *stream);
int evc_spdfgto_dipole_batch(int natm, int nshell, int count, const double *coords, const int *shell_atom,
                             const int *shell_l, const int *shell_prim_offset, const double *exponents,
                             const double *coefficients, const double origin[3], double *dip, void *stream);
int evc_spdfgto_dipole_grad_batch(int natm, int nshell, int count, const double *coords, const int *shell_atom,
                                  const int *shell_l, const int *shell_prim_offset, const double *exponents,
                                  const double *coefficients, const double origin[3], double *ipdip, void *stream);

/* ---------------------------------------------------------------------------------
 * Observables of continuation states (csrc/properties.hip; host statement: evcont_amd/properties.py; the reference's
 * scripts/MD/H2O-H3O+/evaluate_dipole_moment_charges_continuation.py:72-90 per geometry on the host): for every root pair
 * (k, l) of `pairs` and every geometry of a batch the predicted (transition) 1-RDM of the symmetric weighting
 * W = (c_k c_l^T + c_l c_k^T) / 2 -- the quantity evc_outputs_roots.d_pred holds --, its back-rotation P = X D X^T to the AO
 * basis, the dipole moment and the atomic populations.
 *   ws       an evaluation workspace whose geometries 0 .. count-1 hold phases A+B of THESE geometries (the contract of
 *            evc_phase_gradient_roots_batch; count = 1: the single-geometry entry points), ws_bytes >= count x the bytes
 *            of one geometry (evc_workspace_bytes(t, in->natm)).  Only X of each geometry is read and nothing is written,
 *            so a gradient call may follow or precede on the same workspace.
 *   coeffs   DEVICE (count,T,T), rows 0 .. nvec-1 of each block used.
 *   pairs    HOST (npairs,2), 0 <= k <= l < nvec, 1 <= count * npairs <= 4096.  Slots s = p * count + g; every output is
 *            ROOT-PAIR-MAJOR.  Degeneracy warning: evc_phase_gradient_roots.
 *   scratch  DEVICE, 16-byte aligned, at least evc_properties_workspace_bytes(n, ntrain, natm, count, npairs) bytes (0 on a
 *            shape outside the limits): the row-chunk partial sums of D.  T^2 rows are cut into chunks that depend on T
 *            alone and the chunks are added in ascending order: the same bits from run to run.
 * Inputs, all DEVICE: S (count,N,N) (for mulliken), dip (count,3,N,N) = <mu| r - origin |nu>, charges (A), coords
 * (count,A,3) (for dipole), aoslices (A,2) int64 shared by the batch (for mulliken / loewdin); origin by value.
 * Outputs, each may be NULL:
 *   d_oao    (npairs,count,N,N)   D
 *   d_ao     (npairs,count,N,N)   P = X D X^T
 *   dipole   (npairs,count,3)     atomic units; k == l: sum_A Z_A (R_A - origin) - tr(P r); k != l: -tr(P r)
 *   mulliken (npairs,count,A)     populations sum_{mu in A} (P S)_mu,mu   (plain Mulliken, PySCF's mulliken_pop; not the
 *                                 meta-Loewdin analysis of mulliken_meta)
 *   loewdin  (npairs,count,A)     populations sum_{mu in A} D_mu,mu       (the OAO basis is the Loewdin basis)
 * Populations, not charges.  Refused on the host before any launch (rc < 0): a null pointer (of an input only when an
 * output that needs it is asked for), n > 96, T > 512, pairs out of order, count * npairs out of range, misaligned
 * pointers, short scratch, short ws.  Caller's stream, no allocation, no profile stage.
 * --------------------------------------------------------------------------------- */
typedef struct evc_property_inputs {
    int32_t natm;
    int32_t count;
    const double *S;         /* (count,N,N) */
    const double *dip;       /* (count,3,N,N) */
    const int64_t *aoslices; /* (A,2) [start,stop) */
    const double *charges;   /* (A) */
    const double *coords;    /* (count,A,3) Bohr */
    double origin[3];
} evc_property_inputs;
typedef struct evc_property_outputs {
    double *d_oao;
    double *d_ao;
    double *dipole;
    double *mulliken;
    double *loewdin;
} evc_property_outputs;
size_t evc_properties_workspace_bytes(int n, int ntrain, int natm, int count, int npairs);
int evc_properties_roots_batch(const evc_trdm_set *t, const evc_property_inputs *in, const double *coeffs, int nvec,
                               const int32_t *pairs, int npairs, const evc_property_outputs *out, const void *ws,
                               size_t ws_bytes, void *scratch, size_t scratch_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * A uniform electric field on the device (csrc/field.hip; host statement: evcont_amd/field.py).  H(F) = H0 - mu . F changes
 * four arrays of an evc_geometry_batch and nothing else of the chain:
 *   hcore += sum_c F_c dip_c      dhcore[A,x] += sum_c F_c d dip_c / dR_Ax
 *   enuc  -= sum_A Z_A F . (R_A - origin)         gnuc[A] -= Z_A F
 * with dip (count,3,N,N) = <mu| r - origin |nu> of the dipole calls above and its nuclear derivative from
 *   ipdip (count,3,3,N,N),  ipdip[x,c,mu,nu] = <d_x mu| r_c - origin_c |nu>
 * (the electron-coordinate gradient on the bra, the convention of ipovlp):
 *   d dip_c[mu,nu] / dR_Ax = - ipdip[x,c,mu,nu] [mu in A] - ipdip[x,c,nu,mu] [nu in A].
 * evc_sgto_dipole_grad_batch: ipdip of the s-Gaussian molecules of evc_sgto_integrals_batch, with the argument list, the
 *   limits and the refusals of evc_sgto_dipole_batch (natm <= 96, nprim <= 8, positive exponents, 8-byte aligned device
 *   pointers).  Closed form per primitive pair, delta_xc (a/p) S - 2 mu (A - B)_x (P_c - origin_c) S, with P as in
 *   s_gaussian_mol (on coincident coordinates the centre exactly).
 * evc_gto_dipole_grad_batch: ipdip of molecules of contracted shells with l <= 2 (the AO order and the d functions of
 *   evc_spdgto_integrals_batch), with the argument list, the limits and the refusals of evc_spdgto_dipole_batch; it
 *   serves the molecules of evc_spgto_* as well.  The bra derivative 2a (i + 1) - i (i - 1) in the powers of dimension x
 *   of the dipole factor, whose operator adds one more power in dimension c.
 * Both: coords DEVICE (count,natm,3); the basis and origin HOST; one thread per ORDERED pair (mu, nu), one sum over the
 *   primitive pairs (and monomials) in one fixed ascending order; ipdip[x,c] + ipdip[x,c]^T = - delta_xc S to rounding.
 * evc_field_fold_batch: adds the four terms IN PLACE to arrays an integrals call has written.
 *   n, natm, count   N <= 96, 1 <= natm <= 65535, 1 <= count <= 65535.
 *   dip, ipdip, aoslices (A,2) int64, charges (A), coords (count,A,3), field (count,3): DEVICE; one field per geometry.
 *   origin           HOST; the origin dip and ipdip were computed for.
 *   flags            0, or EVC_FLAG_ENERGY_ONLY: hcore and enuc alone; ipdip, aoslices, dhcore and gnuc may then be NULL
 *                    and are not touched.  Any other flag is refused.
 *   hcore (count,N,N), dhcore (count,A,3,N,N), enuc (count), gnuc (count,A,3): DEVICE, read and written.
 *   One thread owns an element pair mu >= nu, reads the element (mu, nu) and writes it and its mirror: hcore stays
 *   exactly symmetric, dhcore in its last two indices.  A zero field leaves every array as it was.
 * All three: a null required pointer, a shape outside the limits, an l outside {0, 1, 2}, a non-positive exponent, a
 * misaligned pointer or an unknown flag is refused before anything is launched (rc < 0, evc_last_error starts with the
 * function's name).  Caller's stream, no allocation, no library state, no workspace, no profile stage.  No sum is split
 * between threads and nothing is accumulated between threads: the same bits from run to run and for every batch size.
 * --------------------------------------------------------------------------------- */
int evc_sgto_dipole_grad_batch(int natm, int nprim, int count, const double *coords, const double *ex, const double *co,
                               const double origin[3], double *ipdip, void *stream);
int evc_gto_dipole_grad_batch(int natm, int nshell, int count, const double *coords, const int *shell_atom,
                              const int *shell_l, const int *shell_prim_offset, const double *exponents,
                              const double *coefficients, const double origin[3], double *ipdip, void *stream);
int evc_field_fold_batch(int n, int natm, int count, const double *dip, const double *ipdip, const int64_t *aoslices,
                         const double *charges, const double *coords, const double *field, const double origin[3],
                         int flags, double *hcore, double *dhcore, double *enuc, double *gnuc, void *stream);

/* ---------------------------------------------------------------------------------
 * Measurement hook (bench.py): while enabled, the fused pipeline records hipEvents on the launch
 * stream immediately before and after the launches of the stages below, for up to max_samples
 * evaluations.  evc_profile_end synchronises those events, returns the summed durations in
 * milliseconds with the number of launches for K5 (rows GEMV) and K8 (cols GEMV), and frees them;
 * afterwards evc_profile_stage reports the same two numbers for any stage selected for that session.
 * Process-wide state.
 * --------------------------------------------------------------------------------- */
#define EVC_PROF_ROWS 0           /* K5  H2 = Gamma . h2 (+ one-body) */
#define EVC_PROF_COLS 1           /* K8  predicted RDMs */
#define EVC_PROF_PAIR_TRANSFORM 2 /* fused pair steps of the two four-index rotations (4 launches per call) */
#define EVC_PROF_IP1 3            /* int2e_ip1 contraction (+ dhcore dots, Y2 slab sums) */
#define EVC_PROF_Y2 4             /* Y2 = K3 . Gamma_sym */
#define EVC_PROF_UNPACK 5         /* unpack/symmetrise the predicted 2-RDM */
#define EVC_PROF_LOEWDIN 6        /* Loewdin orthogonalisation */
#define EVC_PROF_SUBSPACE 7       /* subspace generalised eigenproblem */
#define EVC_PROF_FCI_EXCITE 8     /* evc_fci_*: D = E_pq c (last launch: the layout it wrote) */
#define EVC_PROF_FCI_TRDM 9       /* evc_fci_trdm_rows: split-K product, with its tiling */
#define EVC_PROF_FCI_SIGMA 10     /* evc_fci_sigma: G = h2 . D and the gather */
#define EVC_PROF_FCI_SOLVE 11     /* evc_fci_hdiag / _dots / _combine / _davidson_correction / _spin_apply / _spin_diag:
                                     the kernels of the last such call and its grouping, e.g.
                                     "fci_spin_apply_kernel beta=1 tiles=870", "fci_spin_diag_kernel" (not cleared by
                                     the other evc_fci_* entry points) */
#define EVC_PROF_FCI_ROTATE 12    /* evc_fci_rotate: the minor kernel of each spin, whether it took the complementary
                                     minors, the panels of each T, and the product kernel; evc_fci_rotate_block: the
                                     same followed by " vecs=<nvec>" */
#define EVC_PROF_FCI_PACK 13      /* evc_fci_trdm_rows_packed: the packing kernel, e.g.
                                     "fci_row_pack_kernel<8> rows=3 cols=231 ld=240" (<1>: PACK2, <8>: SYM8) */
int evc_profile_begin(int max_samples);
int evc_profile_end(double *rows_ms, int *rows_n, double *cols_ms, int *cols_n);
int evc_profile_stage(int stage, double *ms, int *launches);
/* Stages timed by the next sessions: bit s = stage s (default: EVC_PROF_ROWS and EVC_PROF_COLS only -- every timed
 * launch costs two event records, which is visible in the one-geometry-at-a-time regime). */
int evc_profile_select(unsigned stage_mask);
/* Name (with template arguments) of the kernel the library most recently launched for a stage, e.g.
 * "gemv_rows_lds_kernel<2,7,2> G=32" (K5 / EVC_PROF_ROWS: followed by the geometries that launch contracted): what a
 * measurement of that stage timed.  Every entry point first clears the stages it can launch (evc_energy_with_grad and
 * evc_energy_with_grad_batch all eight, an evc_phase_* call the stages of its phase), so a stage the last call did not
 * run reads "".  Process-wide: not meaningful while calls run concurrently on several host threads. */
const char *evc_profile_kernel(int stage);

/* The K5 / K8 dispatch of a call of `count` geometries (slots) on `t`, as text, one line per pass over the t-RDM -- first
 * the K5 passes, then the K8 passes of the gradient phase:
 *   "K5 g0=<first geometry> G=<geometries> <kernel> nspans=<two-body>,<one-body>"   (0: not carried by this pass)
 *   "K8 g0=<first geometry> G=<geometries> <kernel>"
 * <kernel> is the name evc_profile_kernel reports when that pass is the stage's last.  A pure function of the integer
 * fields of `t` (n, ntrain, rows2, cols2, ld2, ld1; no pointer is read), count, the knobs EVC_ROWS_LDS, EVC_ROWS_LDS_NT,
 * EVC_ROWS_LDS_MINCOLS, EVC_COLS_LDS and the CU count of the device: device_cus > 0 names it (no device is needed),
 * device_cus <= 0 asks the current device.  Writes at most buf_len - 1 characters and a NUL; returns the length of the
 * whole text, -1 on an invalid argument. */
int evc_trdm_plan_describe(const evc_trdm_set *t, int count, int device_cus, char *buf, size_t buf_len);

#ifdef __cplusplus
}
#endif
#endif /* EVCONT_HIP_H */
