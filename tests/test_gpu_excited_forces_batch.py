"""GPU tests of excited-state forces and interstate couplings for many geometries per call
(include/evcont_hip.h evc_phase_gradient_roots_batch, ``BatchedEvaluator.multistate_energies_with_grads``,
``get_multistate_energies_with_grads``, ``MD_utils.state_swarm``).

The oracle is the one of tests/test_gpu_excited_forces.py, per geometry: root k's gradient is F(c_k) + grad_nuc, the
coupling ½[F(c_k + c_l) - F(c_k) - F(c_l)], with F(c) = grad_elec_OAO(predicted_rdms(c)) of oracle/evcont_oracle.py.
The geometries of a batch are distinct synthetic problems (different AO seeds), so a slot that read another
geometry's integrals would fail its own oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

from evcont_amd.synthetic import make_ao_arrays, make_trdms
from oracle import evcont_oracle as orc
from test_gpu_excited_forces import DEV, Oracle, all_pairs, in_layout, _h6_training, _bent

pytestmark = pytest.mark.gpu


def _evs(trd, A, G):
    from evcont_amd.evaluator import BatchedEvaluator
    return BatchedEvaluator(trd, A, G)


def check_batch(ev, aob, oracles, nroots, pairs, tol_g=1e-9, rdms=False, hermitian=True):
    """Every geometry of the batch against its own oracle; returns the call's result tuple."""
    res = ev.multistate_energies_with_grads(aob, nroots, pairs, return_density_matrices=rdms, hermitian=hermitian)
    E, Cd, grads = res[:3]
    pairs = [(k, k) for k in range(nroots)] if pairs is None else pairs
    G = len(oracles)
    assert E.shape == (G, nroots) and Cd.shape[:2] == (G, nroots) and grads.shape[:2] == (G, len(pairs))
    for g, o in enumerate(oracles):
        np.testing.assert_allclose(E[g], o.E, rtol=0, atol=1e-10, err_msg=f"geometry {g}")
        o.align(Cd[g])
        np.testing.assert_allclose(np.abs(Cd[g]), np.abs(o.C), rtol=0, atol=1e-8)
        for p, (k, l) in enumerate(pairs):
            np.testing.assert_allclose(grads[g, p], o.slot(k, l), rtol=0, atol=tol_g,
                                       err_msg=f"geometry {g}, slot {(k, l)}")
    return res


def check_single(trd, A, daos, res, nroots, pairs, hermitian=True):
    """The batched result of each geometry equals the single-geometry roots path (ContinuationEvaluator).  The two
    paths may run different eigensolver launches (batch vs one geometry), so an eigenvector may come back with the
    other sign: a coupling slot (k, l) is compared after the sign s_k s_l of the coefficient rows."""
    from evcont_amd.evaluator import ContinuationEvaluator
    ev1 = ContinuationEvaluator(trd, A)
    for g, dao in enumerate(daos):
        E1, C1, g1 = ev1.energies_with_grads(dao, nroots, pairs, hermitian=hermitian)
        s = np.sign(np.sum(res[1][g] * C1, axis=1))
        np.testing.assert_allclose(res[0][g], E1, rtol=0, atol=1e-12)
        np.testing.assert_allclose(res[1][g] * s[:, None], C1, rtol=0, atol=1e-12)
        for p, (k, l) in enumerate(pairs):
            np.testing.assert_allclose(res[2][g][p] * s[k] * s[l], g1[p], rtol=0, atol=1e-12, err_msg=f"slot {(k, l)}")


def host_case(n, T, A, seed_t, seeds, lname):
    """(trd-builder inputs, host AO arrays per geometry, oracles): the synthetic t-RDMs of seed_t in the reference
    layout behind `lname` and one AO problem per seed."""
    S, one, two = make_trdms(n, T, seed_t)
    ref_l = "pack2" if lname.startswith("sym8") else lname
    two_l = in_layout(two, ref_l)
    aos = [make_ao_arrays(n, A, s, ip1_rs_symmetric=True) for s in seeds]
    return S, one, two_l, aos


def device_inputs(lname, S, one, two_l, aos, A):
    from evcont_amd.evaluator import DeviceTRDMs, DeviceAO, DeviceAOBatch
    trd = DeviceTRDMs(one, two_l, S, DEV, compress="sym8" if lname.startswith("sym8") else None)
    packed = lname == "sym8_packed"
    daos = [DeviceAO.from_arrays(a, DEV, pack_ip1=packed, pack_eri=packed) for a in aos]
    return trd, daos, DeviceAOBatch.stack(daos)


@pytest.mark.parametrize("lname", ["full6", "pair5", "elec3", "pack2", "sym8", "sym8_packed"])
def test_batch_roots_every_layout(lname):
    n, T, A, nroots = 6, 5, 3, 3
    S, one, two_l, aos = host_case(n, T, A, 36, (1036, 1037, 1038), lname)
    oracles = [Oracle(a, one, two_l, S, nroots) for a in aos]
    trd, daos, aob = device_inputs(lname, S, one, two_l, aos, A)
    ev = _evs(trd, A, 3)
    res = check_batch(ev, aob, oracles, nroots, all_pairs(nroots))
    check_single(trd, A, daos, res, nroots, all_pairs(nroots))
    # the geometries differ: a batch that read geometry 0's integrals for every slot would have failed above
    assert np.abs(res[2][1] - res[2][0]).max() > 1e-3 and np.abs(res[2][2] - res[2][0]).max() > 1e-3
    # a second call on the same (grown) workspace, diagonal slots only
    check_batch(ev, aob, oracles, nroots, None)


@pytest.mark.parametrize("n,seed_t,seed0", [(6, 36, 1039), (20, 50, 2000), (31, 61, 1061)])
@pytest.mark.parametrize("lname", ["pack2", "sym8_packed"])
def test_batch_roots_pair_routes(n, seed_t, seed0, lname):
    """N <= 32: the fused pair steps; 17 <= N <= 30 the ptd / y2d kernels; sym8 + packed inputs the multi-slot ip1."""
    from evcont_amd import _lib
    T, A, nroots, G = 5, 3, 3, 4
    S, one, two_l, aos = host_case(n, T, A, seed_t, range(seed0, seed0 + G), lname)
    oracles = [Oracle(a, one, two_l, S, nroots) for a in aos]
    trd, daos, aob = device_inputs(lname, S, one, two_l, aos, A)
    res = check_batch(_evs(trd, A, G), aob, oracles, nroots, all_pairs(nroots))
    rec = _lib.load().evc_profile_kernel(_lib.PROF_STAGES["ip1"]).decode()
    if lname == "sym8_packed":
        assert rec == "ip1_dh_kernel<8> pairs slots=4", rec          # 6 pairs: chunks of 4 + 2
    else:
        assert "slots=" not in rec, rec
    check_single(trd, A, daos, res, nroots, all_pairs(nroots))


def test_batch_roots_n40_packed_side_stream():
    """N = 40, sym8 + packed (the 64 x 64 pair pipeline), G = 2: the energy-only batch call sends U and s to the side
    stream, which the roots call joins before it copies them."""
    from evcont_amd import _lib
    n, T, A, nroots, G = 40, 5, 3, 3, 2
    S, one, two_l, aos = host_case(n, T, A, 70, (4000, 4001), "sym8_packed")
    oracles = [Oracle(a, one, two_l, S, nroots) for a in aos]
    trd, daos, aob = device_inputs("sym8_packed", S, one, two_l, aos, A)
    ev = _evs(trd, A, G)
    ev.enqueue(aob, nroots, energy_only=True)          # a preceding energy-only batch on the same workspace
    res = check_batch(ev, aob, oracles, nroots, all_pairs(nroots), tol_g=1e-8)
    assert _lib.load().evc_profile_kernel(_lib.PROF_STAGES["pair_transform"]).decode().startswith("pt64_kernel")
    assert "slots=4" in _lib.load().evc_profile_kernel(_lib.PROF_STAGES["ip1"]).decode()
    check_single(trd, A, daos, res, nroots, all_pairs(nroots))


def test_batch_roots_n65_quarter_steps():
    from evcont_amd.evaluator import DeviceTRDMs, DeviceAOBatch
    from evcont_amd.synthetic import make_device_ao, make_device_trdm_rows
    n, T, sizes, nroots, G = 65, 3, (40, 25), 2, 2
    S, one, rows = make_device_trdm_rows(n, T, 2, 5265, DEV)
    daos = [make_device_ao(n, len(sizes), 5265000 + 17 * g, DEV, sizes, ip1_rs_symmetric=True) for g in range(G)]
    c = lambda t: t.cpu().numpy()
    oracles = []
    for d in daos:
        ao = orc.AOBundle(S=c(d.S), hcore=c(d.hcore), eri=c(d.eri), ipovlp=c(d.ipovlp), dhcore=c(d.dhcore),
                          eri_ip1=c(d.eri_ip1), aoslices=c(d.aoslices), enuc=d.enuc, gnuc=c(d.gnuc))
        oracles.append(Oracle(ao, c(one), c(rows), c(S), nroots, min_gap=1e-3))
    trd = DeviceTRDMs.from_device_rows(one, rows, S, 2)
    del rows
    check_batch(_evs(trd, len(sizes), G), DeviceAOBatch.stack(daos), oracles, nroots, all_pairs(nroots), tol_g=1e-8)


def test_batch_roots_large_T_subspace_kernel():
    n, T, A, nroots, G = 6, 40, 3, 3, 3
    S, one, two_l, aos = host_case(n, T, A, 3340, (3341, 3343, 3344), "pack2")
    oracles = [Oracle(a, one, two_l, S, nroots) for a in aos]
    for lname in ("pack2", "sym8"):
        trd, daos, aob = device_inputs(lname, S, one, two_l, aos, A)
        check_batch(_evs(trd, A, G), aob, oracles, nroots, all_pairs(nroots))


def _profiled(fn):
    from evcont_amd import _lib
    lib = _lib.load()
    assert lib.evc_profile_begin(16) == 0
    try:
        fn()
    finally:
        rows_ms, rows_n, cols_ms, cols_n = C.c_double(), C.c_int(), C.c_double(), C.c_int()
        assert lib.evc_profile_end(C.byref(rows_ms), C.byref(rows_n), C.byref(cols_ms), C.byref(cols_n)) == 0
    return rows_n.value, cols_n.value


@pytest.mark.parametrize("G,nroots,pairs_of", [(9, 4, "diag"), (8, 4, "diag"), (2, 3, "all")])
def test_batch_roots_k8_groups_and_records(G, nroots, pairs_of):
    """G x P slots through K8 in groups of 32 (9 x 4 = 36: two groups, the second of 4; 8 x 4 = 32: one group) with
    sym8 + packed inputs; the energy call streams the two-body t-RDM once in K5 for the whole batch.

    launch_gemv_cols records ONE timed COLS stage per gradient call (its kMaxBatchG groups run back to back inside it)
    and names the kernel of its last group: the group count ceil(G * P / 32) shows as that kernel's group size."""
    from evcont_amd import _lib
    n, T, A = 6, 6, 3
    pairs = [(k, k) for k in range(nroots)] if pairs_of == "diag" else all_pairs(nroots)
    S, one, two_l, aos = host_case(n, T, A, 36, range(1100, 1100 + G), "sym8_packed")
    oracles = [Oracle(a, one, two_l, S, nroots) for a in aos]
    trd, daos, aob = device_inputs("sym8_packed", S, one, two_l, aos, A)
    ev = _evs(trd, A, G)
    check_batch(ev, aob, oracles, nroots, pairs)          # (grows the workspace outside the profile session)
    lib = _lib.load()
    rows_n, cols_n = _profiled(lambda: ev.multistate_energies_with_grads(aob, nroots, pairs))
    slots = G * len(pairs)
    groups = -(-slots // 32)
    assert rows_n == 1, rows_n            # K5: one pass over the t-RDM for the batch's energies
    assert cols_n == 1, cols_n            # K8: one stage record covering all groups
    k8 = lib.evc_profile_kernel(_lib.PROF_STAGES["k8_cols"]).decode()
    last = slots - 32 * (groups - 1)      # size of the last group
    if last < 12:                         # (below the matrix-core threshold: launches of 8, 4, 2, 1 slots, each named
        assert k8.endswith(f"<{last & -last}>"), (k8, slots)     # by its size; the record is the smallest)
    else:
        assert "mfma" in k8 or "lds" in k8, (k8, slots)
    ip1 = lib.evc_profile_kernel(_lib.PROF_STAGES["ip1"]).decode()
    assert ip1 == f"ip1_dh_kernel<8> pairs slots={4 if len(pairs) >= 4 else 2}", ip1


def test_batch_roots_nonhermitian():
    n, T, A, nroots, G = 6, 5, 3, 3, 3
    for lname in ("full6", "pack2"):
        S, one, two_l, aos = host_case(n, T, A, 36, (1040, 1041, 1043), lname)
        oracles = [Oracle(a, one, two_l, S, nroots, hermitian=False) for a in aos]
        trd, daos, aob = device_inputs(lname, S, one, two_l, aos, A)
        res = check_batch(_evs(trd, A, G), aob, oracles, nroots, all_pairs(nroots), hermitian=False)
        check_single(trd, A, daos, res, nroots, all_pairs(nroots), hermitian=False)


def test_batch_roots_density_matrices():
    """D_pred / Gamma_pred come back geometry-major, one per slot."""
    from evcont_amd.evaluator import ContinuationEvaluator
    n, T, A, nroots, G = 6, 5, 3, 2, 2
    S, one, two_l, aos = host_case(n, T, A, 36, (1042, 1044), "pack2")
    trd, daos, aob = device_inputs("pack2", S, one, two_l, aos, A)
    res = _evs(trd, A, G).multistate_energies_with_grads(aob, nroots, all_pairs(nroots), return_density_matrices=True)
    assert res[3].shape == (G, 3, n, n) and res[4].shape == (G, 3, n ** 4)
    ev1 = ContinuationEvaluator(trd, A)
    for g in range(G):
        r1 = ev1.energies_with_grads(daos[g], nroots, all_pairs(nroots), return_density_matrices=True)
        sg = np.sign(np.sum(res[1][g] * r1[1], axis=1))       # (eigenvector signs: see check_single)
        for p, (k, l) in enumerate(all_pairs(nroots)):
            np.testing.assert_allclose(res[3][g][p] * sg[k] * sg[l], r1[3][p], rtol=0, atol=1e-13)
            np.testing.assert_allclose(res[4][g][p] * sg[k] * sg[l], r1[4][p].reshape(-1), rtol=0, atol=1e-13)


def test_list_api_and_h6_forces_physical():
    """H6 chain with FCI training states: the list API matches the single-geometry API, and root-1 forces of three bent
    geometries equal central differences of root-1 energies."""
    from evcont_amd.ab_initio_gradients_loewdin import (get_multistate_energies_with_grads,
                                                        get_multistate_energy_with_grad)
    from evcont_amd.evaluator import DeviceTRDMs, DeviceAO, ContinuationEvaluator
    from evcont_amd.hchain import s_gaussian_mol
    cont = _h6_training()
    S, one, two = cont.overlap, cont.one_rdm, cont.two_rdm
    Rs = [_bent(seed=s) for s in (11, 12, 13)]
    mols = [s_gaussian_mol(R) for R in Rs]
    E, grads, h = get_multistate_energies_with_grads(mols, one, two, S, 3, return_couplings=True)
    assert E.shape == (3, 3) and grads.shape == (3, 3, 6, 3) and h.shape == (3, 3, 3, 6, 3)
    for g, m in enumerate(mols):
        E1, g1, h1 = get_multistate_energy_with_grad(m, one, two, S, 3, return_couplings=True)
        np.testing.assert_allclose(E[g], E1, rtol=0, atol=1e-12)
        np.testing.assert_allclose(grads[g], g1, rtol=0, atol=1e-12)
        np.testing.assert_allclose(np.abs(h[g]), np.abs(h1), rtol=0, atol=1e-12)   # (signs follow the eigenvectors)
        np.testing.assert_array_equal(h[g], np.swapaxes(h[g], 0, 1))
        assert E[g, 1] - E[g, 0] >= 1e-2, E[g]
    ev = ContinuationEvaluator(DeviceTRDMs(one, two, S, DEV), 6)
    e1 = lambda r: np.float64(ev.energies(DeviceAO.from_arrays(s_gaussian_mol(r, need_grad=False), DEV,
                                                               energy_only=True), 2)[0][1])
    step = 2e-4
    for g, R in enumerate(Rs):
        g_fd = np.zeros((6, 3))
        for a in range(6):
            for x in range(3):
                Rp, Rm = R.copy(), R.copy()
                Rp[a, x] += step
                Rm[a, x] -= step
                g_fd[a, x] = (e1(Rp) - e1(Rm)) / (2 * step)
        assert np.abs(grads[g, 1] - g_fd).max() < 2e-7, g


def test_state_swarm_conserves_energy():
    """Four NVE trajectories on root 1, one batched call per step: each conserves its total energy within what the
    ground-state NVE test of test_gpu_hchain.py allows at dt = 2 (5e-5 Ha), and trajectory 0 equals a single
    trajectory driven through get_state_scanner."""
    from evcont_amd.MD_utils import state_swarm, get_state_scanner, nve_velocity_verlet
    from evcont_amd.hchain import s_gaussian_mol
    from test_hchain_physics import bent_chain
    cont = _h6_training()
    S, one, two = cont.overlap, cont.one_rdm, cont.two_rdm
    mols = [s_gaussian_mol(bent_chain(6, d=1.9, seed=s, amp=0.05)) for s in (5, 6, 7, 8)]
    frames = state_swarm(mols, one, two, S, root=1, dt=2.0, steps=40)
    assert len(frames) == 40
    etot = np.array([f["epot"] + f["ekin"] for f in frames])         # (steps, G)
    assert etot.shape == (40, 4)
    assert np.all(frames[-1]["ekin"] > 1e-4)                          # kinetic energy was gained
    assert np.abs(etot - etot[0]).max() < 5e-5, np.abs(etot - etot[0]).max(axis=0)
    ref = nve_velocity_verlet(get_state_scanner(mols[0], one, two, S, root=1), mols[0], dt=2.0, steps=5)
    for k in range(5):
        np.testing.assert_allclose(frames[k]["coord"][0], ref[k]["coord"], rtol=0, atol=1e-10)
