"""Which kernel each profile stage launches, case by case: the dispatch table of the library.

Every case names the inputs of one call and, for each of the eight stages of ``evc_profile_kernel``
(include/evcont_hip.h ``EVC_PROF_*``), the prefix of the name the library must report having launched last for it;
``""`` means the stage does not run in that call.  ``tests/test_gpu_dispatch_map.py`` runs every case with an empty
``env`` against the oracle and asserts the records; ``tests/test_dispatch_closure.py`` checks that every kernel a stage
can launch (``hipLaunchKernelGGL`` in ``evcont_amd/csrc``) occurs as an expected name here, so that a new branch without
a row fails the host-side suite.

Fields of a case:
  n, T, A, G       orbitals, training states, atoms, geometries per call
  layout           "full6" | "pair5" | "elec3" | "pack2" | "sym8" (the reference's four layouts, and the compressed one)
  packed           int2e / int2e_ip1 handed over packed (aosym s4 / s2kl; sym8 and N <= 64 only)
  energy_only      the call is energy-only; ``expect`` holds its records, ``expect_grad`` those after the
                   ``evc_phase_gradient`` call that follows it on the same workspace
  warm             two calls, the second warm-started; ``expect`` holds the second call's records
  nroots           roots asked for
  api              "single" (evc_energy_with_grad, ContinuationEvaluator) or "batch" (evc_energy_with_grad_batch);
                   "roots" (ContinuationEvaluator.energies_with_grads: an energy-only evc_energy_with_grad, then
                   evc_phase_gradient_roots) or "roots_batch" (BatchedEvaluator.multistate_energies_with_grads: an
                   energy-only evc_energy_with_grad_batch, then evc_phase_gradient_roots_batch); ``expect`` holds the
                   records after both calls (the gradient stages from the roots call)
  pairs            (roots APIs) the root pairs (k, l), k <= l < nroots, of every geometry
  keep             the predicted 1- and 2-RDMs are requested as outputs (and checked)
  env              knobs the branch needs; they are read once per process, so such rows are run by the test named in
                   ``covered_by`` in a process of its own, not here

The last launch of a stage wins: PAIR_TRANSFORM of a gradient call names the second gradient-side step, ROWS / COLS of
a batch that is split in groups name the last group's kernel.
"""

STAGES = ("k5_rows", "k8_cols", "pair_transform", "ip1", "y2", "unpack", "loewdin", "subspace")

# records every split / side-stream form of the Loewdin step leaves (csrc/pipeline.hip phase_hamiltonian, csrc/side_stream.hip)
L_RIDE = "loewdin_kernel part=1"                                        # n <= 32, T <= 32: rides in the solve launch
L_SIDE32 = "loewdin_kernel part=1; side stream: loewdin_kernel part=2"  # n <= 32, T > 32, < 12 geometries
L_ONE32 = "loewdin_kernel part=0"
L_SIDE64 = "loewdin_ns64_kernel part=1; side stream: loewdin_big_kernel part=2"   # 32 < n <= 64, < 12 geometries
L_BIG = "loewdin_big_kernel part=0"                                     # n > 64, or >= 12 geometries beyond 32 orbitals

# the fused gradient-side route (17 <= n <= 30, packed inputs, >= 4 geometries, one slot per geometry, no 2-RDM output)
Y2_PAIRSTEP = "y2d_kernel<1> pairstep"   # Y2 inside the first pair step
PT_DOT = "ptd_kernel<0> +ip1"            # the int2e_ip1 dot inside the second ...
IP1_REST = "ip1_dh_kernel<8> pairs (dot in ptd)"   # ... and what is left to ip1_dh_kernel


def case(id, n, T, A, G, layout, expect, packed=False, energy_only=False, warm=False, nroots=1, api="batch",
         keep=False, env=None, covered_by=None, expect_grad=None, pairs=None):
    assert set(expect) == set(STAGES), id
    assert expect_grad is None or set(expect_grad) == set(STAGES), id
    return dict(id=id, n=n, T=T, A=A, G=G, layout=layout, packed=packed, energy_only=energy_only, warm=warm,
                nroots=nroots, api=api, keep=keep, env=env or {}, covered_by=covered_by, expect=expect,
                expect_grad=expect_grad, pairs=pairs)


def all_pairs(nroots):
    """The diagonal pairs, then the couplings k < l."""
    return [(k, k) for k in range(nroots)] + [(k, l) for k in range(nroots) for l in range(k + 1, nroots)]


def st(rows, cols, pt, ip1, y2, unpack, loewdin, subspace):
    return dict(zip(STAGES, (rows, cols, pt, ip1, y2, unpack, loewdin, subspace)))


CASES = [
    # ---- smallest shapes, every reference layout on the two-pair-step route (n <= 32)
    case("n1_full6_single", 1, 1, 1, 1, "full6", api="single", keep=True,
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_rs_kernel<1>", "pt_kernel<16,0>", "ip1_dh_kernel<8> chunks",
                   "y2_kernel<1>", "sym_oao_t_kernel", L_RIDE, "subspace_loewdin_kernel few=0")),
    case("n2_sym8_packed_single_rdms", 2, 2, 1, 1, "sym8", packed=True, api="single", keep=True,
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_rs_kernel<1>", "pt_pipe_kernel<16,0>",
                   "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>", "unpack8_pairs_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("n10_pair5_G2", 10, 3, 2, 2, "pair5",
         expect=st("gemv_rows_kernel<8,2> G=2", "gemv_cols_rs_kernel<2>", "pt_kernel<16,0>", "ip1_dh_kernel<8> chunks",
                   "y2_kernel<1>", "sym_oao_t_kernel", L_RIDE, "subspace_loewdin_kernel few=1")),
    case("n12_elec3_single", 12, 3, 2, 1, "elec3", api="single",
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_rs_kernel<1>", "pt_kernel<16,0>", "ip1_dh_kernel<8> chunks",
                   "y2_kernel<1>", "unpack_sym_kernel", L_RIDE, "subspace_loewdin_kernel few=1")),
    case("n14_pack2_G3", 14, 3, 2, 3, "pack2",
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_rs_kernel<1>", "pt_kernel<16,0>", "ip1_dh_kernel<8> chunks",
                   "y2_kernel<1>", "unpack_sym_kernel", L_RIDE, "subspace_loewdin_kernel few=1")),
    # ---- the compressed layout with packed inputs across the pair-step kernels' edges
    case("n15_sym8_packed_G1", 15, 3, 2, 1, "sym8", packed=True,
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_rs_kernel<1>", "pt_pipe4_kernel<16,0>",
                   "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>", "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("n16_sym8_packed_G3", 16, 3, 2, 3, "sym8", packed=True,
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_rs_kernel<1>", "pt_pipe4_kernel<16,0>",
                   "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>", "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("n16_sym8_packed_G4", 16, 3, 2, 4, "sym8", packed=True,
         expect=st("gemv_rows_wr_kernel<8,4,2> G=4", "gemv_cols_rs_kernel<4>", "pt_pipe_kernel<16,0>",
                   "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>", "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("n17_sym8_packed_G3", 17, 3, 2, 3, "sym8", packed=True,
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_rs_kernel<1>", "pt_pipe4_kernel<32,0>",
                   "ip1_dh_kernel<8> pairs", "y2d_kernel", "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("n17_sym8_packed_G4", 17, 3, 2, 4, "sym8", packed=True,
         expect=st("gemv_rows_wr_kernel<8,4,2> G=4", "gemv_cols_rs_kernel<4>", PT_DOT,
                   IP1_REST, Y2_PAIRSTEP, "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("n29_sym8_packed_G8", 29, 2, 2, 8, "sym8", packed=True,
         expect=st("gemv_rows_wr_kernel<4,8,4> G=8", "gemv_cols_rs_kernel<8>", PT_DOT,
                   IP1_REST, Y2_PAIRSTEP, "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("n30_sym8_packed_G9", 30, 2, 2, 9, "sym8", packed=True,
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_rs_kernel<1>", PT_DOT, IP1_REST,
                   Y2_PAIRSTEP, "unpack8_prep_kernel", L_RIDE, "subspace_loewdin_kernel few=1")),
    # (n = 31, 32: the software-pipelined pair step needs more than 80 KB of LDS -> the phase-alternating pt_kernel)
    case("n31_sym8_packed_G4", 31, 2, 2, 4, "sym8", packed=True,
         expect=st("gemv_rows_wr_kernel<8,4,2> G=4", "gemv_cols_rs_kernel<4>", "pt_kernel<32,1>",
                   "ip1_dh_kernel<8> pairs", "y2_fused_kernel<32>", "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("n32_sym8_packed_G12", 32, 2, 1, 12, "sym8", packed=True,
         expect=st("gemv_rows_lds_kernel<1,2,4> G=12", "gemv_cols_mfma_rs_kernel<2,6,1>", "pt_kernel<32,1>",
                   "ip1_dh_kernel<8> pairs", "y2_fused_kernel<32>", "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("n20_sym8_packed_G2_rdms", 20, 3, 2, 2, "sym8", packed=True, keep=True,
         expect=st("gemv_rows_kernel<8,2> G=2", "gemv_cols_rs_kernel<2>", "pt_pipe4_kernel<32,0>",
                   "ip1_dh_kernel<8> pairs", "y2d_kernel", "unpack8_pairs_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("n20_sym8_full_G2", 20, 3, 2, 2, "sym8",
         expect=st("gemv_rows_kernel<8,2> G=2", "gemv_cols_rs_kernel<2>", "pt_kernel<32,1>", "ip1_dh_kernel<8> chunks",
                   "y2d_kernel", "unpack8_prep_kernel", L_RIDE, "subspace_loewdin_kernel few=1")),
    # ---- batch sizes around the K5 / K8 group boundaries (8 / 9, 11 / 12, 32 / 33)
    case("n6_sym8_packed_G11", 6, 3, 2, 11, "sym8", packed=True,
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_rs_kernel<1>", "pt_pipe_kernel<16,0>",
                   "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>", "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("n6_sym8_packed_G32", 6, 3, 2, 32, "sym8", packed=True,
         expect=st("gemv_rows_mfma_pipe_kernel<2,7,1,1> G=32", "gemv_cols_mfma_rs_kernel<8,3,2>",
                   "pt_pipe_kernel<16,0>", "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>", "unpack8_prep_kernel",
                   L_RIDE, "subspace_loewdin_kernel few=1")),
    case("n6_sym8_packed_G33", 6, 3, 2, 33, "sym8", packed=True,
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_rs_kernel<1>", "pt_pipe_kernel<16,0>",
                   "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>", "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("n14_T6_sym8_packed_G17", 14, 6, 2, 17, "sym8", packed=True,
         expect=st("gemv_rows_", "gemv_cols_lds_kernel", "pt_pipe_kernel<16,0>", "ip1_dh_kernel<8> pairs",
                   "y2_fused_kernel<16>", "unpack8_prep_kernel", L_RIDE, "subspace_loewdin_kernel few=1")),
    case("n14_T23_sym8_packed_G17", 14, 23, 2, 17, "sym8", packed=True,
         expect=st("gemv_rows_", "gemv_cols_lds_slab_kernel", "pt_pipe_kernel<16,0>", "ip1_dh_kernel<8> pairs",
                   "y2_fused_kernel<16>", "unpack8_prep_kernel", L_RIDE, "subspace_loewdin_kernel few=1")),
    # ---- training-set sizes: the subspace kernels and their few-roots route
    case("n6_T32_sym8_packed_G2_nroots3", 6, 32, 2, 2, "sym8", packed=True, nroots=3,
         expect=st("gemv_rows_kernel<8,2> G=2", "gemv_cols_rs_kernel<2>", "pt_pipe4_kernel<16,0>",
                   "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>", "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("n6_T33_sym8_packed_G2_nroots2", 6, 33, 2, 2, "sym8", packed=True, nroots=2,
         expect=st("gemv_rows_kernel<8,2> G=2", "gemv_cols_rs_kernel<2>", "pt_pipe4_kernel<16,0>",
                   "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>", "unpack8_prep_kernel", L_SIDE32,
                   "subspace_big_kernel<1> few=1")),
    case("n4_T8_pack2_single_nroots5", 4, 8, 1, 1, "pack2", nroots=5, api="single",
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_rs_kernel<1>", "pt_kernel<16,0>", "ip1_dh_kernel<8> chunks",
                   "y2_kernel<1>", "unpack_sym_kernel", L_RIDE, "subspace_loewdin_kernel few=0")),
    case("n2_T130_sym8_packed_G1_nroots2", 2, 130, 1, 1, "sym8", packed=True, nroots=2,
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_rs_kernel<1>", "pt_pipe_kernel<16,0>",
                   "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>", "unpack8_prep_kernel", L_SIDE32,
                   "subspace_big_kernel<0> few=0")),
    case("n3_T40_full6_single_nroots5", 3, 40, 1, 1, "full6", nroots=5, api="single",
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_rs_kernel<1>", "pt_kernel<16,0>", "ip1_dh_kernel<8> chunks",
                   "y2_kernel<1>", "sym_oao_t_kernel", L_SIDE32, "subspace_big_kernel<1> few=0")),
    # ---- flags: energy-only followed by a gradient phase, warm start
    case("n12_sym8_packed_G2_energy_then_grad", 12, 3, 2, 2, "sym8", packed=True, energy_only=True,
         expect=st("gemv_rows_kernel<8,2> G=2", "", "pt_pipe4_kernel<16,1>", "", "", "", L_RIDE,
                   "subspace_loewdin_kernel few=1"),
         expect_grad=st("gemv_rows_kernel<8,2> G=2", "gemv_cols_rs_kernel<2>", "pt_pipe4_kernel<16,0>",
                        "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>", "unpack8_prep_kernel", L_RIDE,
                        "subspace_loewdin_kernel few=1")),
    case("n10_sym8_packed_G2_warm", 10, 3, 2, 2, "sym8", packed=True, warm=True,
         expect=st("gemv_rows_kernel<8,2> G=2", "gemv_cols_rs_kernel<2>", "pt_pipe4_kernel<16,0>",
                   "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>", "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=0")),
    case("n40_sym8_packed_single_warm", 40, 3, 2, 1, "sym8", packed=True, warm=True, api="single",
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_kernel<1>", "pt64_kernel<0>", "ip1_dh_kernel<8> pairs",
                   "y2_64_kernel", "unpack8_pairs_kernel", L_SIDE64, "subspace_kernel few=0")),
    # ---- beyond 32 orbitals: 64-wide symmetric pipeline, quarter steps, the side-stream Loewdin step
    case("n33_sym8_packed_single", 33, 3, 2, 1, "sym8", packed=True, api="single",
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_rs_kernel<1>", "pt64_kernel<0>", "ip1_dh_kernel<8> pairs",
                   "y2_64_kernel", "unpack8_pairs_kernel", L_SIDE64, "subspace_kernel few=1")),
    case("n33_sym8_packed_G2_rdms", 33, 3, 2, 2, "sym8", packed=True, keep=True,
         expect=st("gemv_rows_kernel<8,2> G=2", "gemv_cols_rs_kernel<2>", "pt64_kernel<0>", "ip1_dh_kernel<8> pairs",
                   "y2_64_kernel", "unpack8_pairs_kernel", L_SIDE64, "subspace_kernel few=1")),
    case("n33_sym8_full_G2", 33, 3, 2, 2, "sym8",
         expect=st("gemv_rows_kernel<8,2> G=2", "gemv_cols_rs_kernel<2>", "qt_kernel<48>", "ip1_dh_kernel<8> chunks",
                   "y2_sb_kernel<3>", "unpack8_kernel lead_half=0", L_SIDE64, "subspace_kernel few=1")),
    case("n33_sym8_full_G2_energy_then_grad", 33, 3, 2, 2, "sym8", energy_only=True,
         expect=st("gemv_rows_kernel<8,2> G=2", "", "qt_kernel<48>", "", "", "pack_sym8_kernel", L_SIDE64,
                   "subspace_kernel few=1"),
         expect_grad=st("gemv_rows_kernel<8,2> G=2", "gemv_cols_rs_kernel<2>", "qt_kernel<48>",
                        "ip1_dh_kernel<8> chunks", "y2_sb_kernel<3>", "unpack8_kernel lead_half=0", L_SIDE64,
                        "subspace_kernel few=1")),
    case("n33_full6_single", 33, 2, 1, 1, "full6", api="single", keep=True,
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_kernel<1>", "qt_kernel<48>", "ip1_dh_kernel<8> chunks",
                   "y2_kernel<3>", "sym_oao_t_kernel", L_SIDE64, "subspace_kernel few=1")),
    case("n34_pair5_G2", 34, 2, 1, 2, "pair5",
         expect=st("gemv_rows_kernel<8,2> G=2", "gemv_cols_kernel<2>", "qt_kernel<48>", "ip1_dh_kernel<8> chunks",
                   "y2_kernel<3>", "sym_oao_t_kernel", L_SIDE64, "subspace_kernel few=1")),
    case("n40_elec3_single_energy_then_grad", 40, 2, 1, 1, "elec3", energy_only=True, api="single",
         expect=st("gemv_rows_kernel<8,1> G=1", "", "qt_kernel<48>", "", "", "pack_kernel", L_SIDE64,
                   "subspace_kernel few=1"),
         expect_grad=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_kernel<1>", "qt_kernel<48>", "ip1_dh_kernel<8> chunks",
                        "y2_kernel<3>", "unpack_sym_kernel", L_SIDE64, "subspace_kernel few=1")),
    case("n40_pack2_G11", 40, 2, 1, 11, "pack2",
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_kernel<1>", "qt_kernel<48>", "ip1_dh_kernel<8> chunks",
                   "y2_kernel<3>", "unpack_sym_kernel", L_SIDE64, "subspace_kernel few=1")),
    case("n40_sym8_packed_G12", 40, 2, 1, 12, "sym8", packed=True,
         expect=st("gemv_rows_lds_kernel<1,2,4> G=12", "gemv_cols_mfma_kernel<1,2,6,1>", "pt64_kernel<0>",
                   "ip1_dh_kernel<8> pairs", "y2_64_kernel", "unpack8_pairs_kernel", L_BIG, "subspace_kernel few=1")),
    case("n64_sym8_packed_single", 64, 1, 1, 1, "sym8", packed=True, api="single",
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_kernel<1>", "pt64_kernel<0>", "ip1_dh_kernel<8> pairs",
                   "y2_64_kernel", "unpack8_pairs_kernel", L_SIDE64, "subspace_kernel few=0")),
    case("n65_sym8_full_single", 65, 1, 1, 1, "sym8", api="single",
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_kernel<1>", "qt_kernel<80>", "ip1_dh_kernel<8> chunks",
                   "y2_sb_kernel<4>", "unpack8_kernel lead_half=0", L_BIG, "subspace_kernel few=0")),
    # ---- excited-state forces and couplings: every root pair of a geometry is a slot of the gradient chain.  IP1 of
    #      the packed pair-block route reads a geometry's int2e_ip1 rows once for up to kIp1MaxSlots of its slots
    #      (roots_batch, P >= 2: "slots=K", K the largest power of two <= min(P, 8)); else one slot per block.  K8 runs
    #      the G * P slots (single geometry: P) in its batched groups
    case("roots_n6_sym8_packed_single_P3", 6, 5, 2, 1, "sym8", packed=True, api="roots", nroots=2,
         pairs=all_pairs(2),
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_rs_kernel<1>", "pt_pipe4_kernel<16,0>",
                   "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>", "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("roots_batch_n6_sym8_packed_G2_P1", 6, 5, 2, 2, "sym8", packed=True, api="roots_batch", nroots=2,
         pairs=[(0, 1)],
         expect=st("gemv_rows_kernel<8,2> G=2", "gemv_cols_rs_kernel<2>", "pt_pipe4_kernel<16,0>",
                   "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>", "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("roots_batch_n6_sym8_packed_G2_P3", 6, 5, 2, 2, "sym8", packed=True, api="roots_batch", nroots=2,
         pairs=all_pairs(2),
         expect=st("gemv_rows_kernel<8,2> G=2", "gemv_cols_rs_kernel<2>", "pt_pipe_kernel<16,0>",
                   "ip1_dh_kernel<8> pairs slots=2", "y2_fused_kernel<16>", "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("roots_batch_n10_sym8_packed_G3_P6", 10, 5, 2, 3, "sym8", packed=True, api="roots_batch", nroots=3,
         pairs=all_pairs(3),
         expect=st("gemv_rows_kernel<8,1> G=1", "gemv_cols_mfma_rs_kernel<8,3,2>", "pt_pipe_kernel<16,0>",
                   "ip1_dh_kernel<8> pairs slots=4", "y2_fused_kernel<16>", "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("roots_batch_n6_sym8_packed_G2_P10", 6, 5, 2, 2, "sym8", packed=True, api="roots_batch", nroots=4,
         pairs=all_pairs(4),
         expect=st("gemv_rows_kernel<8,2> G=2", "gemv_cols_mfma_rs_kernel<8,3,2>", "pt_pipe_kernel<16,0>",
                   "ip1_dh_kernel<8> pairs slots=8", "y2_fused_kernel<16>", "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("roots_batch_n6_pack2_G2_P3", 6, 5, 2, 2, "pack2", api="roots_batch", nroots=2, pairs=all_pairs(2),
         expect=st("gemv_rows_kernel<8,2> G=2", "gemv_cols_rs_kernel<2>", "pt_kernel<16,0>", "ip1_dh_kernel<8> chunks",
                   "y2_kernel<1>", "unpack_sym_kernel", L_RIDE, "subspace_loewdin_kernel few=1")),
]

# Branches only a knob reaches.  The knobs are read once per process: these rows are run by the test named in
# ``covered_by`` (a fresh process per knob set), never by test_gpu_dispatch_map.py.
_V = "tests.test_gpu_variants::test_variant_passes_parity_subset"
KNOB_CASES = [
    case("knob_pt_kernel", 24, 3, 2, 32, "sym8", packed=True, env={"EVC_PT_PIPE": "0", "EVC_PT_DMA": "0"},
         covered_by=_V + "[env0]",
         expect=st("gemv_rows_", "gemv_cols", "pt_kernel<32,1>", "ip1_dh_kernel<8> pairs", "y2_fused_kernel<32>",
                   "unpack8_prep_kernel", L_RIDE, "subspace_loewdin_kernel few=1")),
    case("knob_pt_pipe", 24, 3, 2, 32, "sym8", packed=True, env={"EVC_PT_DMA": "0"}, covered_by=_V + "[env1]",
         expect=st("gemv_rows_", "gemv_cols", "pt_pipe_kernel<32,0>", "ip1_dh_kernel<8> pairs", "y2_fused_kernel<32>",
                   "unpack8_prep_kernel", L_RIDE, "subspace_loewdin_kernel few=1")),
    case("knob_subspace_few_off", 6, 40, 2, 2, "sym8", packed=True, env={"EVC_SUBSPACE_FEW": "0"},
         covered_by=_V + "[env2]",
         expect=st("gemv_rows_", "gemv_cols", "pt_pipe4_kernel<16,0>", "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>",
                   "unpack8_prep_kernel", L_SIDE32, "subspace_big_kernel<1> few=0")),
    case("knob_loewdin_one_kernel", 10, 3, 2, 2, "sym8", packed=True, env={"EVC_LOEWDIN_SPLIT": "0"},
         covered_by=_V + "[env3]",
         expect=st("gemv_rows_", "gemv_cols", "pt_pipe4_kernel<16,0>", "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>",
                   "unpack8_prep_kernel", L_ONE32, "subspace_kernel few=1")),
    case("knob_eigh_fp64", 10, 3, 2, 2, "sym8", packed=True, env={"EVC_EIGH_F32": "0"}, covered_by=_V + "[env4]",
         expect=st("gemv_rows_", "gemv_cols", "pt_pipe4_kernel<16,0>", "ip1_dh_kernel<8> pairs", "y2_fused_kernel<16>",
                   "unpack8_prep_kernel", L_ONE32, "subspace_kernel few=0")),
    case("knob_rows_mfma_pipe", 30, 20, 2, 32, "sym8", packed=True, env={"EVC_ROWS_LDS": "0"},
         covered_by=_V + "[env7]",
         expect=st("gemv_rows_mfma_pipe_kernel", "gemv_cols", PT_DOT, IP1_REST, Y2_PAIRSTEP,
                   "unpack8_prep_kernel", L_RIDE, "subspace_loewdin_kernel few=1")),
    case("knob_rows_lds_nt", 10, 20, 2, 32, "sym8", packed=True,
         env={"EVC_ROWS_LDS_MINCOLS": "1", "EVC_ROWS_LDS_NT": "7"}, covered_by=_V + "[env11]",
         expect=st("gemv_rows_lds_kernel", "gemv_cols", "pt_pipe_kernel<16,0>", "ip1_dh_kernel<8> pairs",
                   "y2_fused_kernel<16>", "unpack8_prep_kernel", L_RIDE, "subspace_loewdin_kernel few=1")),
    case("knob_cols_mfma", 30, 20, 2, 32, "sym8", packed=True, env={"EVC_COLS_LDS": "0"}, covered_by=_V + "[env14]",
         expect=st("gemv_rows_lds_kernel", "gemv_cols_mfma", PT_DOT, IP1_REST, Y2_PAIRSTEP,
                   "unpack8_prep_kernel", L_RIDE, "subspace_loewdin_kernel few=1")),
    # one of the two fused steps off: the other stays (n = 17, 4 geometries: the smallest shape on the fused route).  These two
    # rows hold the WHOLE pair_transform / ip1 / y2 records (a prefix would also match the fused record): the covering
    # tests compare them with == in their knob-off process (knob_row)
    case("knob_y2_pairstep_off", 17, 3, 2, 4, "sym8", packed=True, env={"EVC_Y2_PAIRSTEP": "0"},
         covered_by="tests.test_gpu_y2_pairstep::test_knob_off_agrees",
         expect=st("gemv_rows_", "gemv_cols", PT_DOT, IP1_REST, "y2d_kernel", "unpack8_prep_kernel", L_RIDE,
                   "subspace_loewdin_kernel few=1")),
    case("knob_ip1_pairstep_off", 17, 3, 2, 4, "sym8", packed=True, env={"EVC_IP1_PAIRSTEP": "0"},
         covered_by="tests.test_gpu_ip1_pairstep::test_batch_against_oracle_and_knob_off",
         expect=st("gemv_rows_", "gemv_cols", "ptd_kernel<0>", "ip1_dh_kernel<8> pairs", Y2_PAIRSTEP,
                   "unpack8_prep_kernel", L_RIDE, "subspace_loewdin_kernel few=1")),
]


def knob_row(id):
    return next(c for c in KNOB_CASES if c["id"] == id)
