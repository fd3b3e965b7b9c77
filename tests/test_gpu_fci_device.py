"""GPU tests of the device full-CI solver (evcont_amd/fci_device.py, csrc/fci.hip) against the host solver
fci_small.SmallFCI, on hydrogen-chain integrals in the OAO basis (host oracle) and random normalised CI vectors.

Tolerances of the element-wise comparisons are derived, not chosen:

* t-RDMs.  Every element of M[pq,rs] = <E_qp bra | E_rs ket> is a sum of ``dim`` products, on the device and on the
  host alike, so each side obeys |err| <= dim * 2^-53 * max_pq ||D~_bra[pq]|| * max_rs ||D_ket[rs]|| (Cauchy-Schwarz on
  the standard dot-product bound).  The test computes that bound from the host's D and allows twice it (one per side);
  dm1 and the exact identities of the device result are held to the same figure.
* sigma.  sigma(I) = sum_pq h'_pq D[pq](I) + 1/2 sum_pq (E_pq G[pq])(I) with G[pq](J) = sum_rs (pq|rs) D[rs](J) nests an
  N^2-term sum (G) inside a 2 N^2-term sum (the alpha and beta gathers over pq) next to the N^2 terms of h'; D itself is
  a two-term sum and the 1/2 and h' products round once each.  With every term taken in absolute value,
      S(I) = sum_pq |h'_pq| A[pq](I) + 1/2 sum_pq (|E_pq| (|h2| A)[pq])(I),   A[pq] = |E_pq| |c|,
  each side obeys |err(I)| <= (3 N^2 + 4) * 2^-53 * S(I) whatever its summation order; the test allows twice that,
  element by element.  (No sum of length dim occurs in a sigma vector.)
"""
import time

import numpy as np
import pytest
import torch

from evcont_amd.hchain import hydrogen_chain, s_gaussian_mol
from evcont_amd.fci_small import SmallFCI
from oracle import evcont_oracle as orc
from test_hchain_physics import bundle, bent_chain

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CASES = [(4, (2, 2)), (6, (3, 3)), (6, (3, 2)), (8, (4, 4)), (10, (5, 5))]
_HOST = SmallFCI()
_SOLVER = []


def solver():
    from evcont_amd.fci_device import DeviceFCI
    if not _SOLVER:
        _SOLVER.append(DeviceFCI())
    return _SOLVER[0]


def oao_integrals(norb, d=1.8):
    m = hydrogen_chain(norb, d, need_grad=False)
    return orc.integrals_oao(bundle(m), orc.loewdin_trafo(m.S))


def random_vectors(norb, nelec, count, seed):
    _, _, na, nb = _HOST._ops(norb, nelec)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        v = rng.standard_normal((na, nb))
        out.append(v / np.linalg.norm(v))
    return out


def trdm_bound(bra, ket, norb, nelec):
    n2 = norb * norb
    Db = _HOST._excite_all(bra, norb, nelec).reshape(n2, -1)
    Dk = _HOST._excite_all(ket, norb, nelec).reshape(n2, -1)
    dim = Db.shape[1]
    return dim * U * np.linalg.norm(Db, axis=1).max() * np.linalg.norm(Dk, axis=1).max()


def sigma_bound(h1, h2, c, norb, nelec):
    ea, ebT, na, nb = _HOST._ops(norb, nelec)
    n2 = norb * norb
    h2 = np.asarray(h2, dtype=np.float64).reshape(norb, norb, norb, norb)
    hp = np.abs(np.asarray(h1, dtype=np.float64) - 0.5 * np.einsum("prrq->pq", h2))
    ac = np.abs(np.asarray(c, dtype=np.float64).reshape(na, nb))
    A = np.empty((n2, na, nb))
    for p in range(norb):
        for q in range(norb):
            A[p * norb + q] = abs(ea[p][q]) @ ac + (abs(ebT[p][q]).T @ ac.T).T
    S = np.tensordot(hp.reshape(-1), A, axes=(0, 0))
    G = (np.abs(h2).reshape(n2, n2) @ A.reshape(n2, -1)).reshape(A.shape)
    for p in range(norb):
        for q in range(norb):
            g = G[p * norb + q]
            S += 0.5 * (abs(ea[p][q]) @ g + (abs(ebT[p][q]).T @ g.T).T)
    return (3 * n2 + 4) * U * S


def check_identities(ov, dm1, dm2, nelec, tol):
    ne = nelec[0] + nelec[1]
    assert abs(np.trace(dm1) - ne * ov) <= tol
    assert abs(np.einsum("pprr->", dm2) - ne * (ne - 1) * ov) <= tol
    assert np.abs(dm2 - dm2.transpose(2, 3, 0, 1)).max() <= tol


@pytest.mark.parametrize("norb,nelec", CASES)
def test_trdms_against_host(norb, nelec):
    """1, 2, 4: pairs and a row call against SmallFCI.trans_rdm12 within the derived bound; exact identities; the row
    call equals its single calls and itself bit for bit."""
    dev = solver()
    K = 3
    vecs = random_vectors(norb, nelec, K + 1, seed=norb * 10 + nelec[1])
    bra, kets = vecs[0], vecs[1:] + [vecs[0]]
    ov, one, two = dev.trans_rdm12_rows(bra, kets, norb, nelec)
    assert ov.shape == (K + 1,) and one.shape == (K + 1, norb, norb) and two.shape == (K + 1,) + (norb,) * 4
    worst = 0.0
    for i, ket in enumerate(kets):
        r1, r2 = _HOST.trans_rdm12(bra, ket, norb, nelec)
        tol = 2.0 * trdm_bound(bra, ket, norb, nelec)
        e1, e2 = np.abs(one[i] - r1).max(), np.abs(two[i] - r2).max()
        eo = abs(ov[i] - np.dot(bra.ravel(), ket.ravel()))
        worst = max(worst, e1 / tol, e2 / tol)
        print(f"trdm norb={norb} nelec={nelec} ket {i}: dim={bra.size} bound={tol:.3e} |d dm1|={e1:.3e} "
              f"|d dm2|={e2:.3e} |d ovlp|={eo:.3e}")
        assert e1 <= tol and e2 <= tol and eo <= tol
        check_identities(ov[i], one[i], two[i], nelec, tol)
        s1, s2 = dev.trans_rdm12(bra, ket, norb, nelec)
        assert np.array_equal(s1, one[i]) and np.array_equal(s2, two[i])       # rows = K single calls, bitwise
    ov2, one2, two2 = dev.trans_rdm12_rows(bra, kets, norb, nelec)
    assert np.array_equal(ov, ov2) and np.array_equal(one, one2) and np.array_equal(two, two2)
    m1, m2 = dev.make_rdm12(bra, norb, nelec)
    assert np.array_equal(m1, one[K]) and np.array_equal(m2, two[K])
    assert abs(ov[K] - 1.0) <= 2.0 * trdm_bound(bra, bra, norb, nelec)
    print(f"trdm norb={norb} nelec={nelec}: worst error / allowed = {worst:.3e}")


@pytest.mark.parametrize("norb,nelec", CASES)
def test_trdms_in_chunks_are_bitwise_the_resident_result(norb, nelec):
    """A workspace of the least size (excitations formed block by block, the bra side again per ket) gives the bits of
    the resident pass."""
    from evcont_amd import _lib
    from evcont_amd.fci_device import DeviceFCI
    lib = _lib.load()
    vecs = random_vectors(norb, nelec, 3, seed=77 + norb)
    _, _, na, nb = _HOST._ops(norb, nelec)
    small = DeviceFCI(workspace_bytes=lib.evc_fci_workspace_bytes(norb, na, nb, 1))
    a = solver().trans_rdm12_rows(vecs[0], vecs[1:], norb, nelec)
    b = small.trans_rdm12_rows(vecs[0], vecs[1:], norb, nelec)
    rec = lib.evc_profile_kernel(_lib.FCI_PROF_STAGES["fci_trdm"]).decode()
    assert rec.startswith("fci_trdm_kernel<")
    if na * nb > 512:
        assert "bra_resident=0" in rec, rec
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    h1, h2 = oao_integrals(norb)
    assert np.array_equal(solver().contract(h1, h2, vecs[0], norb, nelec), small.contract(h1, h2, vecs[0], norb, nelec))


@pytest.mark.parametrize("norb,nelec", CASES)
def test_contract_against_host(norb, nelec):
    """3: the sigma vector against SmallFCI.contract within the derived element-wise bound; twice the same bits."""
    dev = solver()
    h1, h2 = oao_integrals(norb)
    c = random_vectors(norb, nelec, 1, seed=5 + norb)[0]
    got = dev.contract(h1, h2, c, norb, nelec)
    want = _HOST.contract(h1, h2, c, norb, nelec)
    tol = 2.0 * sigma_bound(h1, h2, c, norb, nelec)
    err = np.abs(got - want)
    print(f"sigma norb={norb} nelec={nelec}: dim={c.size} max|d|={err.max():.3e} min bound={tol.min():.3e} "
          f"max(err/bound)={(err / tol).max():.3e}")
    assert got.shape == want.shape and (err <= tol).all()
    assert np.array_equal(got, dev.contract(h1, h2, c, norb, nelec))
    assert abs(dev.energy(h1, h2, c, norb, nelec) - _HOST.energy(h1, h2, c, norb, nelec)) < 1e-10


@pytest.mark.parametrize("norb,nelec", CASES)
@pytest.mark.parametrize("nroots", [1, 3])
def test_kernel_against_host(norb, nelec, nroots):
    """3: energies to 1e-10 Ha, eigenvectors to 1e-7 up to the sign.  Both solvers fix the sign by making the coefficient
    of largest magnitude positive, which is asserted for each; the vectors themselves are compared up to an overall sign,
    because a state that is odd under the exchange of the alpha and beta strings (the Ms = 0 triplets) has its largest
    coefficient twice, +x and -x, and which of the two a solver meets first is decided by the last bit."""
    h1, h2 = oao_integrals(norb)
    t0 = time.time()
    e_d, v_d = solver().kernel(h1, h2, norb, nelec, nroots=nroots)
    t1 = time.time()
    e_h, v_h = _HOST.kernel(h1, h2, norb, nelec, nroots=nroots)
    t2 = time.time()
    if nroots == 1:
        assert isinstance(e_d, float) and v_d.ndim == 2
        e_d, v_d, e_h, v_h = [e_d], [v_d], [e_h], [v_h]
    assert len(e_d) == len(v_d) == nroots
    de = max(abs(a - b) for a, b in zip(e_d, e_h))
    dv = max(min(np.abs(a - b).max(), np.abs(a + b).max()) for a, b in zip(v_d, v_h))
    for v in list(v_d) + list(v_h):
        assert v.flat[np.argmax(np.abs(v))] > 0.0
    print(f"kernel norb={norb} nelec={nelec} nroots={nroots}: |dE|={de:.2e} |dv|={dv:.2e} device {t1 - t0:.2f} s "
          f"host {t2 - t1:.2f} s")
    assert de < 1e-10 and dv < 1e-7


def test_h12_one_pair_and_one_sigma():
    """(12, (6, 6)): 853 776 determinants, a single pair and a single sigma vector against the host."""
    norb, nelec = 12, (6, 6)
    dev = solver()
    bra, ket = random_vectors(norb, nelec, 2, seed=12)
    t0 = time.time()
    d1, d2 = dev.trans_rdm12(bra, ket, norb, nelec)
    t1 = time.time()
    r1, r2 = _HOST.trans_rdm12(bra, ket, norb, nelec)
    t2 = time.time()
    tol = 2.0 * trdm_bound(bra, ket, norb, nelec)
    e1, e2 = np.abs(d1 - r1).max(), np.abs(d2 - r2).max()
    print(f"trdm norb=12: dim={bra.size} bound={tol:.3e} |d dm1|={e1:.3e} |d dm2|={e2:.3e} device call {t1 - t0:.2f} s "
          f"host {t2 - t1:.2f} s")
    assert e1 <= tol and e2 <= tol
    ov = dev.trans_rdm12_rows(bra, [ket], norb, nelec)[0][0]
    check_identities(ov, d1, d2, nelec, tol)
    h1, h2 = oao_integrals(norb)
    got = dev.contract(h1, h2, bra, norb, nelec)
    want = _HOST.contract(h1, h2, bra, norb, nelec)
    stol = 2.0 * sigma_bound(h1, h2, bra, norb, nelec)
    err = np.abs(got - want)
    print(f"sigma norb=12: max|d|={err.max():.3e} max(err/bound)={(err / stol).max():.3e}")
    assert (err <= stol).all()


class CountingFCI:
    """DeviceFCI that counts what the container asks of it."""

    def __new__(cls):
        from evcont_amd.fci_device import DeviceFCI

        class _Counting(DeviceFCI):
            rows_calls = 0
            pair_calls = 0

            def trans_rdm12_rows(self, *a, **k):
                self.rows_calls += 1
                return super().trans_rdm12_rows(*a, **k)

            def trans_rdm12(self, *a, **k):
                self.pair_calls += 1
                return super().trans_rdm12(*a, **k)

        return _Counting()


def _fci_kernels_ran():
    from evcont_amd import _lib
    lib = _lib.load()
    return {k: lib.evc_profile_kernel(s).decode() for k, s in _lib.FCI_PROF_STAGES.items()}


def test_container_grown_on_the_device_h6():
    """5: the three H6 spacings of test_fci_container_growth_prune_and_device_copy."""
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    from evcont_amd.ab_initio_gradients_loewdin import get_energy_with_grad
    spacings = (1.5, 2.0, 2.8)
    dsolver = CountingFCI()
    cd = FCI_EVCont_obj(cisolver=dsolver, cibasis="OAO")
    ch = FCI_EVCont_obj(cisolver=SmallFCI(), cibasis="OAO")
    for d in spacings:
        cd.append_to_rdms(hydrogen_chain(6, d, need_grad=False))
        ch.append_to_rdms(hydrogen_chain(6, d, need_grad=False))
    assert dsolver.rows_calls == 3 and dsolver.pair_calls == 0
    ran = _fci_kernels_ran()
    assert ran["fci_trdm"].startswith("fci_trdm_kernel<") and ran["fci_sigma"].startswith("fci_sigma_gemm_kernel<")
    assert ran["fci_excite"].startswith("fci_excite_")
    assert cd.two_rdm.shape == (3, 3, 6, 6, 6, 6) and cd.mol_index == [0, 1, 2]
    m = s_gaussian_mol(bent_chain(6, d=1.9, seed=11, amp=0.15))
    Ed, gd = get_energy_with_grad(m, cd.one_rdm, cd.two_rdm, cd.overlap)
    Eh, gh = get_energy_with_grad(m, ch.one_rdm, ch.two_rdm, ch.overlap)
    print(f"H6 container: |dE|={abs(Ed - Eh):.2e} |dg|={np.abs(gd - gh).max():.2e}")
    assert abs(Ed - Eh) < 1e-10 and np.abs(gd - gh).max() < 1e-9
    E, _ = get_energy_with_grad(hydrogen_chain(6, 2.0), cd.one_rdm, cd.two_rdm, cd.overlap)
    assert abs(E - cd.ens[1]) < 1e-8 and abs(cd.ens[1] - ch.ens[1]) < 1e-10


def test_container_grown_on_the_device_h10_two_roots(h10_fci):
    """5: the H10 spacings of the golden set with roots_train=[0, 1]: ten training states."""
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    from evcont_amd.ab_initio_gradients_loewdin import get_energy_with_grad, get_multistate_energy_with_grad
    dsolver = CountingFCI()
    cd = FCI_EVCont_obj(cisolver=dsolver, cibasis="OAO", nroots=2, roots_train=[0, 1])
    ch = FCI_EVCont_obj(cisolver=SmallFCI(), cibasis="OAO", nroots=2, roots_train=[0, 1])
    t = [0.0, 0.0]
    for d in h10_fci["spacings"]:
        for k, c in enumerate((cd, ch)):
            t0 = time.time()
            c.append_to_rdms(hydrogen_chain(10, float(d), need_grad=False))
            t[k] += time.time() - t0
    print(f"H10 container, 10 states: device solver {t[0]:.1f} s, host solver {t[1]:.1f} s")
    assert dsolver.rows_calls == 10 and dsolver.pair_calls == 0
    ran = _fci_kernels_ran()
    assert ran["fci_trdm"].startswith("fci_trdm_kernel<4,2>") and ran["fci_sigma"].startswith("fci_sigma_gemm_kernel<4>")
    assert cd.overlap.shape == (10, 10) and cd.mol_index == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    np.testing.assert_allclose(cd.ens[0::2], h10_fci["ens"], rtol=0, atol=1e-8)
    m = s_gaussian_mol(h10_fci["R_test"])
    Ed, gd = get_energy_with_grad(m, cd.one_rdm, cd.two_rdm, cd.overlap)
    Eh, gh = get_energy_with_grad(m, ch.one_rdm, ch.two_rdm, ch.overlap)
    print(f"H10 container: ground |dE|={abs(Ed - Eh):.2e} |dg|={np.abs(gd - gh).max():.2e}")
    assert abs(Ed - Eh) < 1e-10 and np.abs(gd - gh).max() < 1e-9
    Ed, gd = get_multistate_energy_with_grad(m, cd.one_rdm, cd.two_rdm, cd.overlap, 2)
    Eh, gh = get_multistate_energy_with_grad(m, ch.one_rdm, ch.two_rdm, ch.overlap, 2)
    print(f"H10 container: two roots |dE|={np.abs(Ed - Eh).max():.2e} |dg|={np.abs(gd - gh).max():.2e}")
    assert np.abs(Ed - Eh).max() < 1e-10 and np.abs(gd - gh).max() < 1e-9
    d = float(h10_fci["spacings"][2])
    E, _ = get_energy_with_grad(hydrogen_chain(10, d), cd.one_rdm, cd.two_rdm, cd.overlap)
    assert abs(E - cd.ens[4]) < 1e-8 and abs(E - float(h10_fci["ens"][2])) < 1e-8


def test_limits_raise_before_any_launch():
    """6: norb = 17 and a workspace too small for the problem."""
    from evcont_amd import _lib
    from evcont_amd._lib import EvcontHipError
    from evcont_amd.fci_device import DeviceFCI
    before = _fci_kernels_ran()
    with pytest.raises(EvcontHipError, match="norb=17"):
        DeviceFCI().trans_rdm12_rows(np.zeros(4), [np.zeros(4)], 17, (1, 1))
    bra, ket = random_vectors(8, (4, 4), 2, seed=1)
    with pytest.raises(EvcontHipError, match="workspace_bytes=65536"):
        DeviceFCI(workspace_bytes=65536).trans_rdm12(bra, ket, 8, (4, 4))
    h1, h2 = oao_integrals(8)
    with pytest.raises(EvcontHipError, match="workspace_bytes=65536"):
        DeviceFCI(workspace_bytes=65536).contract(h1, h2, bra, 8, (4, 4))
    with pytest.raises(EvcontHipError, match="complex"):
        solver().trans_rdm12(bra.astype(complex), ket, 8, (4, 4))
    assert _fci_kernels_ran() == before
    torch.cuda.synchronize()
