"""Host tests of the CI-vector rotation under an orbital transformation (fci_small.transform_ci, the reference of the
device kernels of csrc/fci_rotate.hip), of the small RHF that supplies the canonical basis of array-level molecules
(scf_small.rhf), and of the route FCI_EVCont_obj takes with cibasis="canonical" when its solver has a transform_ci.

``signed_permutation`` / ``permuted_by_strings`` / ``random_orthogonal`` / ``general_u`` are shared with
tests/test_gpu_fci_rotate.py."""
import numpy as np
import pytest

from evcont_amd.fci_davidson import NumpyOps, davidson
from evcont_amd.fci_small import SmallFCI, _strings, minor_matrix, transform_ci
from evcont_amd.hchain import hydrogen_chain
from evcont_amd.scf_small import rhf
from oracle import evcont_oracle as orc
from test_hchain_physics import bundle


def signed_permutation(norb, seed):
    """``(u, perm, sign)``: ``u[p, perm[p]] = sign[p]``, i.e. new orbital ``perm[p]`` = ``sign[p]`` x old orbital p."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(norb)
    sign = rng.choice([-1.0, 1.0], size=norb)
    u = np.zeros((norb, norb))
    u[np.arange(norb), perm] = sign
    return u, perm, sign


def _string_map(norb, nocc, perm, sign):
    """For every old string: (index of the string its orbitals are sent to, sign) -- the product of the orbital signs
    and of the parity of the permutation that puts the images of its orbitals, taken in ascending order of the old
    ones, in ascending order.  No determinant is evaluated."""
    strs = _strings(norb, nocc)
    index = {s: i for i, s in enumerate(strs)}
    target, sgn = np.empty(len(strs), dtype=np.int64), np.empty(len(strs))
    for i, s in enumerate(strs):
        occ = [p for p in range(norb) if (s >> p) & 1]
        img = [int(perm[p]) for p in occ]
        inversions = sum(1 for a in range(len(img)) for b in range(a + 1, len(img)) if img[a] > img[b])
        target[i] = index[sum(1 << q for q in img)]
        sgn[i] = np.prod([sign[p] for p in occ]) * (-1.0 if inversions & 1 else 1.0)
    return target, sgn


def permuted_by_strings(c, norb, nelec, perm_a, sign_a, perm_b=None, sign_b=None):
    """What transform_ci gives for signed permutations, by moving entries."""
    if perm_b is None:
        perm_b, sign_b = perm_a, sign_a
    ta, sa = _string_map(norb, nelec[0], perm_a, sign_a)
    tb, sb = _string_map(norb, nelec[1], perm_b, sign_b)
    out = np.zeros_like(c)
    out[np.ix_(ta, tb)] = sa[:, None] * c * sb[None, :]
    return out


def random_orthogonal(norb, seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((norb, norb)))
    return q * np.sign(np.diag(r))


def general_u(norb, seed):
    return np.eye(norb) + 0.3 * np.random.default_rng(seed).standard_normal((norb, norb))


def random_ci(norb, nelec, seed):
    na, nb = len(_strings(norb, nelec[0])), len(_strings(norb, nelec[1]))
    return np.random.default_rng(seed).standard_normal((na, nb))


SHAPES = [(5, (3, 2)), (6, (5, 4))]


@pytest.mark.parametrize("norb,nelec", SHAPES + [(3, (0, 3)), (1, (1, 0))])
def test_identity_returns_the_input(norb, nelec):
    c = random_ci(norb, nelec, 1)
    assert np.array_equal(transform_ci(c, nelec, np.eye(norb)), c)
    assert np.array_equal(SmallFCI().transform_ci(c, nelec, np.eye(norb)), c)


@pytest.mark.parametrize("norb,nelec", SHAPES + [(4, (2, 2)), (7, (0, 7)), (6, (1, 3))])
def test_signed_permutation_moves_and_signs_the_entries_exactly(norb, nelec):
    u, perm, sign = signed_permutation(norb, seed=norb)
    c = np.random.default_rng(norb).integers(-3, 4, size=random_ci(norb, nelec, 0).shape).astype(np.float64)
    want = permuted_by_strings(c, norb, nelec, perm, sign)
    assert np.array_equal(transform_ci(c, nelec, u), want)
    assert np.abs(want).sum() == np.abs(c).sum()
    u2, perm2, sign2 = signed_permutation(norb, seed=norb + 50)
    want = permuted_by_strings(c, norb, nelec, perm, sign, perm2, sign2)
    assert np.array_equal(transform_ci(c, nelec, (u, u2)), want)


@pytest.mark.parametrize("make", [random_orthogonal, general_u])
@pytest.mark.parametrize("norb,nelec", SHAPES)
def test_two_rotations_compose_like_their_product(norb, nelec, make):
    """Cauchy-Binet: the matrices of minors multiply like the matrices."""
    c = random_ci(norb, nelec, 2)
    u1, u2, v1, v2 = (make(norb, s) for s in (3, 4, 5, 6))
    one = transform_ci(transform_ci(c, nelec, u1), nelec, u2)
    both = transform_ci(c, nelec, u1 @ u2)
    scale = np.abs(both).max()
    assert np.abs(one - both).max() <= 1e-12 * scale
    one = transform_ci(transform_ci(c, nelec, (u1, v1)), nelec, (u2, v2))
    both = transform_ci(c, nelec, (u1 @ u2, v1 @ v2))
    assert np.abs(one - both).max() <= 1e-12 * np.abs(both).max()
    if make is random_orthogonal:
        assert abs(np.linalg.norm(both) - np.linalg.norm(c)) <= 1e-12 * np.linalg.norm(c)


@pytest.mark.parametrize("norb,k", [(5, 3), (6, 5), (9, 7), (10, 9)])
def test_complementary_minors_give_the_same_matrix(norb, k):
    """Jacobi: det(u[I, J]) = det(u) (-1)^(sum I + sum J) det((u^-1)[J^c, I^c]) -- the identity the device route for more
    than eight electrons rests on."""
    u = general_u(norb, norb + k)
    T = minor_matrix(u, norb, k)
    strs = _strings(norb, k)
    full = (1 << norb) - 1
    comp = _strings(norb, norb - k)
    where = {s: i for i, s in enumerate(comp)}
    Tc = minor_matrix(np.linalg.inv(u), norb, norb - k)
    odd = np.array([bin(s & 0xAAAA).count("1") & 1 for s in strs])
    ci = np.array([where[full ^ s] for s in strs])
    want = np.linalg.det(u) * np.where((odd[:, None] + odd[None, :]) & 1, -1.0, 1.0) * Tc[np.ix_(ci, ci)].T
    assert np.abs(T - want).max() <= 1e-11 * max(1.0, np.abs(T).max())


@pytest.mark.parametrize("natm", [4, 6])
def test_rhf_orbitals_are_orthonormal_and_diagonalise_the_fock_matrix(natm):
    m = hydrogen_chain(natm, 1.8, need_grad=False)
    C, e, converged = rhf(m.S, m.hcore, m.eri, m.nelec)
    assert converged
    assert np.abs(C.T @ m.S @ C - np.eye(natm)).max() <= 1e-12
    occ = np.zeros(natm)
    occ[:m.nelec[0]] += 1.0
    occ[:m.nelec[1]] += 1.0
    D = (C * occ) @ C.T
    F = m.hcore + np.einsum("pqrs,rs->pq", m.eri, D) - 0.5 * np.einsum("prqs,rs->pq", m.eri, D)
    Fmo = C.T @ F @ C
    assert np.abs(Fmo - np.diag(np.diag(Fmo))).max() <= 1e-8
    assert np.abs(np.diag(Fmo) - e).max() <= 1e-8 and (np.diff(e) > 0).all()


def test_rhf_open_shell_uses_the_spin_averaged_density():
    m = hydrogen_chain(5, 1.8, need_grad=False)
    assert m.nelec == (3, 2)
    C, e, converged = rhf(m.S, m.hcore, m.eri, m.nelec)
    assert converged and np.abs(C.T @ m.S @ C - np.eye(5)).max() <= 1e-12


def test_rhf_that_does_not_converge_warns_and_returns_orbitals():
    m = hydrogen_chain(4, 1.8, need_grad=False)
    with pytest.warns(UserWarning, match="not converged"):
        C, _, converged = rhf(m.S, m.hcore, m.eri, m.nelec, max_cycle=1)
    assert not converged and np.abs(C.T @ m.S @ C - np.eye(4)).max() <= 1e-12


def host_integrals(mol, basis):
    return orc.integrals_oao(bundle(mol), np.asarray(basis))


@pytest.fixture
def host_container_route(monkeypatch):
    """FCI_EVCont_obj with the OAO basis and the integral rotation computed on the host (the device versions are what
    tests/test_gpu_fci_rotate.py runs)."""
    from evcont_amd import FCI_EVCont, electron_integral_utils
    real = electron_integral_utils.get_basis

    def get_basis(mol, basis_type="OAO"):
        return orc.loewdin_trafo(mol.S) if basis_type == "OAO" else real(mol, basis_type=basis_type)

    monkeypatch.setattr(FCI_EVCont, "get_basis", get_basis)
    monkeypatch.setattr(FCI_EVCont, "get_integrals", host_integrals)
    return FCI_EVCont.FCI_EVCont_obj


def test_container_grown_in_the_canonical_basis_equals_the_oao_one(host_container_route):
    make = host_container_route
    can = make(cisolver=SmallFCI(), cibasis="canonical", nroots=2, roots_train=[0, 1])
    oao = make(cisolver=SmallFCI(), cibasis="OAO", nroots=2, roots_train=[0, 1])
    for d in (1.6, 2.0):
        for c in (can, oao):
            c.append_to_rdms(hydrogen_chain(4, d, need_grad=False))
    assert len(can.fcivecs) == len(oao.fcivecs) == 4
    assert np.abs(np.array(can.ens) - np.array(oao.ens)).max() <= 1e-10
    # the sign of an eigenvector is the solver's choice in its own basis: fix each state's from its overlap with the
    # OAO-solved one, then the t-RDMs of states i, j carry the product of the two signs
    s = np.array([np.sign(np.vdot(a, b)) for a, b in zip(can.fcivecs, oao.fcivecs)])
    for a, b, sg in zip(can.fcivecs, oao.fcivecs, s):
        assert 1.0 - abs(np.vdot(a, b)) <= 1e-10 and sg != 0
    ss = s[:, None] * s[None, :]
    assert np.abs(ss * can.overlap - oao.overlap).max() <= 1e-10
    assert np.abs(ss[:, :, None, None] * can.one_rdm - oao.one_rdm).max() <= 1e-10
    assert np.abs(ss[:, :, None, None, None, None] * can.two_rdm - oao.two_rdm).max() <= 1e-10


def test_split_basis_of_an_array_mol_names_its_reason():
    from evcont_amd.electron_integral_utils import get_basis
    with pytest.raises(NotImplementedError, match="Boys"):
        get_basis(hydrogen_chain(4, 1.8, need_grad=False), "split")


def test_davidson_needs_fewer_sigma_vectors_in_the_canonical_basis():
    m = hydrogen_chain(6, 1.8, need_grad=False)
    C = rhf(m.S, m.hcore, m.eri, m.nelec)[0]
    count = {}
    energy = {}
    for name, basis in (("OAO", orc.loewdin_trafo(m.S)), ("canonical", C)):
        h1, h2 = host_integrals(m, basis)
        w, _, converged, info = davidson(NumpyOps(h1, h2, 6, m.nelec), nroots=1)
        assert converged
        count[name], energy[name] = info["nsigma"], w[0]
    print("sigma vectors:", count)
    assert abs(energy["OAO"] - energy["canonical"]) <= 1e-9
    assert count["canonical"] < count["OAO"], count
