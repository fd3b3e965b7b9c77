"""GPU tests of the excited-state forces and interstate couplings (include/evcont_hip.h evc_phase_gradient_roots,
``ContinuationEvaluator.energies_with_grads``, ``get_multistate_energy_with_grad``, ``MD_utils.get_state_scanner``).

The oracle is composed of ``oracle/evcont_oracle.py`` functions only: root k's gradient is the reference's
``get_energy_with_grad`` with c_k in place of c_0, F(c_k) + grad_nuc with F(c) = grad_elec_OAO(predicted_rdms(c)); the
coupling is h_kl = [F(c_k + c_l) - F(c_k) - F(c_l)] / 2.  Synthetic data: cond(S_train) <= 1e3 and root gaps >= 1e-2 Ha
(asserted)."""
import ctypes as C

import numpy as np
import pytest
import torch

from evcont_amd.synthetic import make_ao_arrays, make_trdms, pack_rows
from oracle import evcont_oracle as orc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAYOUTS = {"full6": (False, False), "pair5": (True, False), "elec3": (False, True), "pack2": (True, True)}


def bundle(a):
    return orc.AOBundle(a.S, a.hcore, a.eri, a.ipovlp, a.dhcore, a.eri_ip1, a.aoslices, a.enuc, a.gnuc)


def in_layout(two, name):
    p, e = LAYOUTS[name]
    return pack_rows(two, p, e) if (p or e) else two


def sym8(G):
    a = G + np.swapaxes(G, -4, -3)
    a = a + np.swapaxes(a, -2, -1)
    a = a + np.moveaxis(a, (-2, -1), (-4, -3))
    return a / 8.0


def all_pairs(nroots):
    return [(k, k) for k in range(nroots)] + [(k, l) for k in range(nroots) for l in range(k + 1, nroots)]


class Oracle:
    """Energies, coefficients and the gradient functional F of one geometry on the ORIGINAL t-RDMs."""

    def __init__(self, ao, one, two, S, nroots, hermitian=True, min_gap=1e-2):
        self.b, self.one, self.two, self.n = bundle(ao), one, two, ao.S.shape[0]
        assert np.linalg.cond(S) <= 1e3
        self.E, self.C = orc.approximate_multistate_OAO(self.b, one, two, S, min(S.shape[0], nroots + 1), hermitian)
        if len(self.E) > 1:
            assert np.min(np.diff(self.E)) >= min_gap, np.diff(self.E)
        self.E, self.C = self.E[:nroots], self.C[:nroots]
        self.X = orc.loewdin_trafo(self.b.S)
        self.dX = orc.derivative_ao_mo_trafo(self.b)
        self._F = {}

    def align(self, C_dev):
        s = np.sign(np.sum(self.C * C_dev, axis=1))
        self.C = self.C * s[:, None]

    def F(self, c):
        """F(c), memoised per coefficient vector (its bytes): a coupling slot reuses F(c_k) and F(c_l)."""
        key = np.ascontiguousarray(c, dtype=np.float64).tobytes()
        if key not in self._F:
            D, G = orc.predicted_rdms(c, self.one, self.two, self.n)
            self._F[key] = orc.grad_elec_OAO(self.b, D, G, X=self.X, dX=self.dX)
            self._F[key].setflags(write=False)
        return self._F[key]

    def slot(self, k, l):
        if k == l:
            return self.F(self.C[k]) + self.b.gnuc
        return 0.5 * (self.F(self.C[k] + self.C[l]) - self.F(self.C[k]) - self.F(self.C[l]))


def check(ev, dao, o, nroots, pairs, rdms=False, sym=False, tol_g=1e-9):
    res = ev.energies_with_grads(dao, nroots, pairs, return_density_matrices=rdms)
    pairs = [(k, k) for k in range(nroots)] if pairs is None else pairs
    E, Cd, grads = res[:3]
    np.testing.assert_allclose(E, o.E, rtol=0, atol=1e-10)
    o.align(Cd)
    np.testing.assert_allclose(np.abs(Cd), np.abs(o.C), rtol=0, atol=1e-8)
    for p, (k, l) in enumerate(pairs):
        np.testing.assert_allclose(grads[p], o.slot(k, l), rtol=0, atol=tol_g, err_msg=f"slot {(k, l)}")
    if rdms:
        D, G = res[3], res[4]
        for p, (k, l) in enumerate(pairs):
            if k != l:
                continue
            Do, Go = orc.predicted_rdms(o.C[k], o.one, o.two, o.n)
            Go = np.asarray(Go).reshape((o.n,) * 4)
            np.testing.assert_allclose(D[p], Do, rtol=0, atol=1e-11)
            np.testing.assert_allclose(G[p], sym8(Go) if sym else Go, rtol=0, atol=1e-11)
    return res


# seeds whose synthetic problems have root gaps >= 1e-2 Ha (asserted by Oracle)
SEED = {1: 31, 6: 36, 31: 61}


@pytest.mark.parametrize("n", [1, 6, 31])
@pytest.mark.parametrize("lname", ["full6", "pair5", "elec3", "pack2", "sym8", "sym8_packed"])
def test_roots_every_layout(lname, n):
    from evcont_amd.evaluator import DeviceTRDMs, DeviceAO, ContinuationEvaluator
    T, A = 5, min(n, 3)
    S, one, two = make_trdms(n, T, SEED[n])
    ao = make_ao_arrays(n, A, 1000 + SEED[n], ip1_rs_symmetric=True)
    ref_l = "pack2" if lname.startswith("sym8") else lname
    two_l = in_layout(two, ref_l)
    o = Oracle(ao, one, two_l, S, 3)
    trd = DeviceTRDMs(one, two_l, S, DEV, compress="sym8" if lname.startswith("sym8") else None)
    packed = lname == "sym8_packed"
    dao = DeviceAO.from_arrays(ao, DEV, pack_ip1=packed, pack_eri=packed)
    ev = ContinuationEvaluator(trd, A)
    check(ev, dao, o, 3, all_pairs(3), rdms=not packed, sym=lname == "sym8")
    # one root on the same evaluator, then the single-root path still gives root 0 of the reference
    o1 = Oracle(ao, one, two_l, S, 1)
    check(ev, dao, o1, 1, None)
    E0, g0 = ev.energy_with_grad(dao)
    assert abs(E0 - o.E[0]) < 1e-10 and np.abs(g0 - o.slot(0, 0)).max() < 1e-9


def _device_case(n, T, sizes, seed):
    from evcont_amd.synthetic import make_device_ao, make_device_trdm_rows
    S, one, rows = make_device_trdm_rows(n, T, 2, seed, DEV)
    dao = make_device_ao(n, len(sizes), seed * 1000, DEV, sizes, ip1_rs_symmetric=True)
    c = lambda t: t.cpu().numpy()
    ao = orc.AOBundle(S=c(dao.S), hcore=c(dao.hcore), eri=c(dao.eri), ipovlp=c(dao.ipovlp), dhcore=c(dao.dhcore),
                      eri_ip1=c(dao.eri_ip1), aoslices=c(dao.aoslices), enuc=dao.enuc, gnuc=c(dao.gnuc))
    return S, one, rows, dao, ao


@pytest.mark.parametrize("n,T,sizes,legs", [(33, 5, (17, 16), ("sym8", "sym8_packed")),
                                            (58, 5, (30, 14, 14), ("sym8", "sym8_packed")),
                                            (70, 3, (40, 30), ("pack2", "sym8"))])
def test_roots_beyond_32_orbitals(n, T, sizes, legs):
    from evcont_amd.evaluator import DeviceTRDMs, ContinuationEvaluator
    S, one, rows, dao, ao = _device_case(n, T, sizes, 5200 + n)
    nroots = min(T, 3)
    o = Oracle(ao, one.cpu().numpy(), rows.cpu().numpy(), S.cpu().numpy(), nroots)
    trd = DeviceTRDMs.from_device_rows(one, rows, S, 2)
    pairs = all_pairs(nroots)
    if "pack2" in legs:
        check(ContinuationEvaluator(trd, len(sizes)), dao, o, nroots, pairs, tol_g=1e-8)
    trd.compress_sym8_()
    del rows
    if "sym8" in legs:
        check(ContinuationEvaluator(trd, len(sizes)), dao, o, nroots, pairs, tol_g=1e-8)
    if "sym8_packed" in legs:
        check(ContinuationEvaluator(trd, len(sizes)), dao.packed_ip1(eri=True), o, nroots, pairs, tol_g=1e-8)


def test_roots_large_T_subspace_kernel():
    from evcont_amd.evaluator import DeviceTRDMs, DeviceAO, ContinuationEvaluator
    n, T, A = 6, 40, 3
    S, one, two = make_trdms(n, T, 3340)
    ao = make_ao_arrays(n, A, 3341, ip1_rs_symmetric=True)
    two_l = in_layout(two, "pack2")
    o = Oracle(ao, one, two_l, S, 3)
    for compress in (None, "sym8"):
        ev = ContinuationEvaluator(DeviceTRDMs(one, two_l, S, DEV, compress=compress), A)
        check(ev, DeviceAO.from_arrays(ao, DEV), o, 3, all_pairs(3))


def test_more_than_32_slots_two_k8_groups():
    """34 diagonal slots: two groups of the batched K8 (32 + 2) in one call."""
    from evcont_amd.evaluator import DeviceTRDMs, DeviceAO, ContinuationEvaluator
    n, T, A, nroots = 6, 40, 3, 34
    S, one, two = make_trdms(n, T, 3340)
    ao = make_ao_arrays(n, A, 3341, ip1_rs_symmetric=True)
    two_l = in_layout(two, "pack2")
    o = Oracle(ao, one, two_l, S, nroots, min_gap=1e-3)      # the 35 lowest roots, >= 1e-3 Ha apart
    ev = ContinuationEvaluator(DeviceTRDMs(one, two_l, S, DEV), A)
    check(ev, DeviceAO.from_arrays(ao, DEV), o, nroots, [(k, k) for k in range(nroots)])


def test_root0_matches_ground_state_path():
    from evcont_amd.ab_initio_gradients_loewdin import get_energy_with_grad, get_multistate_energy_with_grad
    from evcont_amd.evaluator import DeviceTRDMs, DeviceAO, ContinuationEvaluator
    n, T, A = 6, 5, 3
    S, one, two = make_trdms(n, T, 36)
    ao = make_ao_arrays(n, A, 1036, ip1_rs_symmetric=True)
    two_l = in_layout(two, "pack2")
    E, g = get_multistate_energy_with_grad(ao, one, two_l, S, 3)
    E0, g0 = get_energy_with_grad(ao, one, two_l, S)
    assert E.shape == (3,) and g.shape == (3, A, 3)
    assert abs(E[0] - E0) < 1e-12 and np.abs(g[0] - g0).max() < 1e-12
    ev = ContinuationEvaluator(DeviceTRDMs(one, two_l, S, DEV), A)
    dao = DeviceAO.from_arrays(ao, DEV)
    Er, _, gr = ev.energies_with_grads(dao, 3)
    E1, g1 = ev.energy_with_grad(dao)
    assert abs(Er[0] - E1) < 1e-12 and np.abs(gr[0] - g1).max() < 1e-12
    # couplings through the public API: symmetric, electronic on the diagonal
    E, g, h, D, G = get_multistate_energy_with_grad(ao, one, two_l, S, 3, return_couplings=True,
                                                    return_density_matrices=True)
    assert h.shape == (3, 3, A, 3) and D.shape == (3, n, n) and G.shape == (3, n, n, n, n)
    np.testing.assert_array_equal(h, h.transpose(1, 0, 2, 3))
    np.testing.assert_allclose(h[1, 1] + ao.gnuc, g[1], rtol=0, atol=1e-12)
    o = Oracle(ao, one, two_l, S, 3)
    o.align(ev.energies_with_grads(dao, 3)[1])          # (the coupling's sign follows the device eigenvectors)
    np.testing.assert_allclose(h[0, 2], o.slot(0, 2), rtol=0, atol=1e-9)


@pytest.mark.parametrize("lname", ["full6", "pack2"])
def test_nonhermitian_roots(lname):
    from evcont_amd.evaluator import DeviceTRDMs, DeviceAO, ContinuationEvaluator
    from evcont_amd.ab_initio_gradients_loewdin import get_multistate_energy_with_grad
    n, T, A = 6, 5, 3
    S, one, two = make_trdms(n, T, 36)
    ao = make_ao_arrays(n, A, 1036, ip1_rs_symmetric=True)
    two_l = in_layout(two, lname)
    o = Oracle(ao, one, two_l, S, 3, hermitian=False)
    ev = ContinuationEvaluator(DeviceTRDMs(one, two_l, S, DEV), A)
    E, Cd, grads = ev.energies_with_grads(DeviceAO.from_arrays(ao, DEV), 3, all_pairs(3), hermitian=False)
    np.testing.assert_allclose(E, o.E, rtol=0, atol=1e-10)
    o.align(Cd)
    np.testing.assert_allclose(Cd, o.C, rtol=0, atol=1e-8)        # the same 2-norm vectors
    for p, (k, l) in enumerate(all_pairs(3)):
        np.testing.assert_allclose(grads[p], o.slot(k, l), rtol=0, atol=1e-9)
    E2, g2 = get_multistate_energy_with_grad(ao, one, two_l, S, 3, hermitian=False)
    np.testing.assert_allclose(E2, o.E, rtol=0, atol=1e-10)
    np.testing.assert_allclose(g2, grads[:3], rtol=0, atol=1e-12)


def test_one_pass_over_the_trdm():
    from evcont_amd import _lib
    from evcont_amd.evaluator import DeviceTRDMs, DeviceAO, ContinuationEvaluator
    n, T, A = 6, 5, 3
    S, one, two = make_trdms(n, T, 36)
    ao = make_ao_arrays(n, A, 1036, ip1_rs_symmetric=True)
    ev = ContinuationEvaluator(DeviceTRDMs(one, in_layout(two, "pack2"), S, DEV, compress="sym8"), A)
    dao = DeviceAO.from_arrays(ao, DEV)
    ev.energies_with_grads(dao, 4)          # (grows the workspace, outside the session)
    lib = _lib.load()
    assert lib.evc_profile_begin(8) == 0
    try:
        ev.energies_with_grads(dao, 4)
    finally:
        rows_ms, rows_n, cols_ms, cols_n = C.c_double(), C.c_int(), C.c_double(), C.c_int()
        assert lib.evc_profile_end(C.byref(rows_ms), C.byref(rows_n), C.byref(cols_ms), C.byref(cols_n)) == 0
    assert cols_n.value == 1 and rows_n.value == 1
    for st in ("k8_cols", "pair_transform", "ip1", "y2", "unpack"):
        assert lib.evc_profile_kernel(_lib.PROF_STAGES[st]) != b"", st
    assert b"G=4" in lib.evc_profile_kernel(_lib.PROF_STAGES["k8_cols"]) or \
        b"<4>" in lib.evc_profile_kernel(_lib.PROF_STAGES["k8_cols"])


def _h6_training():
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    from evcont_amd.fci_small import SmallFCI
    from evcont_amd.hchain import hydrogen_chain
    cont = FCI_EVCont_obj(cisolver=SmallFCI(), cibasis="OAO", roots_train=[0, 1])
    for d in (1.5, 2.0, 2.8):
        cont.append_to_rdms(hydrogen_chain(6, d, need_grad=False))
    return cont


def _bent(seed=11, d=1.9, amp=0.15):
    rng = np.random.default_rng(seed)
    R = np.zeros((6, 3))
    R[:, 0] = d * np.arange(6)
    return R + amp * rng.standard_normal((6, 3))


def test_state_scanner():
    from evcont_amd.MD_utils import get_scanner, get_state_scanner, nve_velocity_verlet
    from evcont_amd.ab_initio_gradients_loewdin import get_multistate_energy_with_grad
    from evcont_amd.hchain import s_gaussian_mol
    cont = _h6_training()
    S, one, two = cont.overlap, cont.one_rdm, cont.two_rdm
    m = s_gaussian_mol(_bent())
    e0, g0 = get_state_scanner(m, one, two, S, root=0)(m)
    e, g = get_scanner(m, one, two, S)(m)
    assert abs(e0 - e) < 1e-12 and np.abs(g0 - g).max() < 1e-12
    sc = get_state_scanner(m, one, two, S, root=2)
    e2, g2 = sc(m)
    E, G = get_multistate_energy_with_grad(m, one, two, S, 3)
    assert abs(e2 - E[2]) < 1e-12 and np.abs(g2 - G[2]).max() < 1e-12
    assert sc.base.predicted_one_rdm.shape == (6, 6)
    frames = nve_velocity_verlet(sc, m, dt=2.0, steps=3)
    assert len(frames) == 3 and np.abs(frames[2]["coord"] - frames[0]["coord"]).max() > 0.0


def test_h6_excited_state_forces_physical():
    from evcont_amd.evaluator import DeviceTRDMs, DeviceAO, ContinuationEvaluator
    from evcont_amd.hchain import hydrogen_chain, s_gaussian_mol
    cont = _h6_training()
    S, one, two = cont.overlap, cont.one_rdm, cont.two_rdm
    ev = ContinuationEvaluator(DeviceTRDMs(one, two, S, DEV), 6)
    # a training geometry: both trained roots are reproduced
    E, _, _ = ev.energies_with_grads(DeviceAO.from_arrays(hydrogen_chain(6, 2.0), DEV), 2)
    np.testing.assert_allclose(E, cont.ens[2:4], rtol=0, atol=1e-8)
    R = _bent()
    E, _, grads = ev.energies_with_grads(DeviceAO.from_arrays(s_gaussian_mol(R), DEV), 3, all_pairs(3))
    assert E[1] - E[0] >= 1e-2 and E[2] - E[1] >= 1e-2, E
    for p in range(grads.shape[0]):
        assert np.abs(grads[p].sum(axis=0)).max() < 1e-8, p      # no net force, no net coupling
    e1 = lambda r: np.float64(ev.energies(DeviceAO.from_arrays(s_gaussian_mol(r, need_grad=False), DEV,
                                                               energy_only=True), 2)[0][1])
    h = 2e-4
    g_fd = np.zeros((6, 3))
    for a in range(6):
        for x in range(3):
            Rp, Rm = R.copy(), R.copy()
            Rp[a, x] += h
            Rm[a, x] -= h
            g_fd[a, x] = (e1(Rp) - e1(Rm)) / (2 * h)
    assert np.abs(grads[1] - g_fd).max() < 2e-7
