"""Host tests of ``evcont_amd.gto_spd`` (AO integrals of s, p and real spherical d shells, numpy): against
``gto_small.sp_gaussian_mol`` on molecules of s and p shells, the normalisation of the d components, rotations, central
differences, translational invariance and a cross-check of the Cartesian d integrals against the p derivatives of the
existing statement."""
import numpy as np
import pytest

import spdgto_cases as dc
import spgto_cases as sc
from evcont_amd import gto_host
from evcont_amd import gto_small as gs
from evcont_amd import gto_spd as gd

ARRAYS = ("S", "hcore", "eri", "ipovlp", "dhcore", "eri_ip1", "gnuc")


@pytest.fixture(scope="module")
def bent():
    R, Z, shells = dc.bent_three_centre()
    return R, Z, shells, gd.spd_gaussian_mol(R, Z, shells)


def as_spd(shells):
    return [[gd.Shell(sh.l, sh.exponents, sh.coefficients) for sh in atom] for atom in shells]


@pytest.mark.parametrize("name", ["sto-3g", "6-31g", "truth_a"])
def test_reproduces_the_sp_statement(name):
    """All eight arrays and the dipole integrals of ``sp_gaussian_mol`` on molecules without d shells.  Measured
    (scaled_diff, worst array): STO-3G 1.7e-16, 6-31G 3.0e-16, case a 1.5e-16; gate ``spdgto_cases.SP_GATE``."""
    if name == "truth_a":
        T = sc.load_truth()
        ref = sc.case_mol(T, "a")
        new = gd.spd_gaussian_mol(ref.coords, ref.charges, as_spd(ref.shells), renormalize=False)
    else:
        ref, new = gs.water(name), gd.water(name)
    worst = 0.0
    for k in ARRAYS:
        d = sc.scaled_diff(getattr(new, k), getattr(ref, k))
        worst = max(worst, d)
        assert d < dc.SP_GATE, (k, d)
    assert abs(new.enuc - ref.enuc) <= dc.SP_GATE * max(1.0, abs(ref.enuc))
    o = (0.1, -0.2, 0.3)
    d = sc.scaled_diff(new.dipole_integrals(o), ref.dipole_integrals(o))
    print(name, "worst array %.1e dipole %.1e" % (worst, d))
    assert d < dc.SP_GATE
    assert np.array_equal(new.aoslices, ref.aoslices) and new.nelec == ref.nelec


def test_d_components_are_orthonormal_on_their_centre(bent):
    """Same-centre blocks: <d|s> = 0, <d_m|d_m'> = delta for a renormalised contracted d shell of two primitives, to
    1e-14; and no function is the Cartesian x^2 + y^2 + z^2 (which would overlap with s)."""
    S = bent[3].S
    assert np.abs(S[4:9, 0]).max() < 1e-14                     # d against s of the first centre
    assert np.abs(S[4:9, 1:4]).max() < 1e-14                   # d against p
    assert np.abs(S[4:9, 4:9] - np.eye(5)).max() < 1e-14
    assert np.abs(S[10:15, 10:15] - np.eye(5)).max() < 1e-14
    assert np.abs(np.diag(S) - 1.0).max() < 1e-14


def d_representation(Q):
    """The 5 x 5 real l = 2 representation D with f_m(Q x) = sum_k D[k, m] f_k(x), built by transforming the quadratic
    polynomials x^T M_m x of the five functions (``gto_spd.D_MONOMIALS``)."""
    Ms = []
    for comp in gd.D_MONOMIALS:
        M = np.zeros((3, 3))
        for (i, j, k), w in comp:
            idx = [0] * i + [1] * j + [2] * k
            M[idx[0], idx[1]] += 0.5 * w
            M[idx[1], idx[0]] += 0.5 * w
        Ms.append(M)
    D = np.zeros((5, 5))
    for m in range(5):
        T = Q.T @ Ms[m] @ Q
        for k in range(5):
            D[k, m] = np.sum(Ms[k] * T) / np.sum(Ms[k] * Ms[k])
        assert np.abs(sum(D[k, m] * Ms[k] for k in range(5)) - T).max() < 1e-14     # traceless: no s-type part
    return D


def test_rotation(bent):
    """S, hcore and eri of the rotated molecule are the originals under the rotation of the p blocks and the 5 x 5 real
    l = 2 representation.  Gate: the project's parity 1e-10 is far above what is seen (1e-15); asserted at 1e-13, the
    rounding of a four-index transform of O(1) numbers."""
    R, Z, shells, m0 = bent
    rng = np.random.default_rng(3)
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] *= -1
    m1 = gd.spd_gaussian_mol(R @ Q.T, Z, shells, need_grad=False)
    n = m0.S.shape[0]
    U = np.zeros((n, n))
    f = 0
    for atom in shells:
        for sh in atom:
            k = 2 * sh.l + 1
            U[f:f + k, f:f + k] = (np.eye(1), Q.T, d_representation(Q))[sh.l]
            f += k
    assert sc.scaled_diff(m1.S, U.T @ m0.S @ U) < 1e-13
    assert sc.scaled_diff(m1.hcore, U.T @ m0.hcore @ U) < 1e-13
    assert sc.scaled_diff(m1.eri, np.einsum("pqrs,pa,qb,rc,sd->abcd", m0.eri, U, U, U, U, optimize=True)) < 1e-13
    assert abs(m1.enuc - m0.enuc) < 1e-13


def test_derivatives_agree_with_central_differences():
    """ipovlp, dhcore, eri_ip1 and gnuc against central differences of S, hcore, eri and enuc (step and tolerance of
    tests/test_hchain_physics.py: h = 2e-4, 2e-7), for one coordinate of every centre of a bent s + p + d molecule."""
    R, Z, shells = dc.small_bent()
    m = gd.spd_gaussian_mol(R, Z, shells)
    h = 2e-4
    for at, d in ((0, 0), (1, 2), (2, 1)):
        Rp, Rm = R.copy(), R.copy()
        Rp[at, d] += h
        Rm[at, d] -= h
        mp, mm = (gd.spd_gaussian_mol(x, Z, shells, need_grad=False) for x in (Rp, Rm))
        s0, s1 = m.aoslices[at]
        dS = np.zeros_like(m.S)
        dS[s0:s1, :] -= m.ipovlp[d, s0:s1, :]
        dS[:, s0:s1] -= m.ipovlp[d, s0:s1, :].T
        g = m.eri_ip1[d]
        de = np.zeros_like(m.eri)
        de[s0:s1] -= g[s0:s1]
        de[:, s0:s1] -= g[s0:s1].transpose(1, 0, 2, 3)
        de[:, :, s0:s1] -= g[s0:s1].transpose(2, 3, 0, 1)
        de[:, :, :, s0:s1] -= g[s0:s1].transpose(2, 3, 1, 0)
        assert np.abs((mp.S - mm.S) / (2 * h) - dS).max() < 2e-7
        assert np.abs((mp.hcore - mm.hcore) / (2 * h) - m.dhcore[at, d]).max() < 2e-7
        assert np.abs((mp.eri - mm.eri) / (2 * h) - de).max() < 2e-7
        assert abs((mp.enuc - mm.enuc) / (2 * h) - m.gnuc[at, d]) < 2e-7


def test_translational_invariance(bent):
    m = bent[3]
    assert np.abs(m.dhcore.sum(axis=0)).max() < 1e-12 * max(1.0, np.abs(m.dhcore).max())
    assert np.abs(m.gnuc.sum(axis=0)).max() < 1e-13


def test_cartesian_d_against_the_p_derivative_of_the_sp_statement(monkeypatch):
    """Independent of all the above: d/dx of p_x = N_p x exp(-a r^2) is N_p (s - 2a xx).  With one-primitive shells of
    one exponent on one centre, <grad_x p_x| nu> and (grad_x p_x nu | kappa lambda) of the EXISTING ``sp_gaussian_mol``
    (ipovlp, eri_ip1; electron gradients) equal that combination of the Cartesian xx and the s integrals of the new
    module, whose d shell is switched to the monomial xx alone for this test."""
    a = 0.9
    R = np.array([[0.0, 0.0, 0.0], [0.4, -0.7, 1.1]])
    Z = np.array([2.0, 1.0])
    ref = gs.sp_gaussian_mol(R, Z, [[gs.Shell(1, [a], [1.0])], [gs.Shell(0, [0.6], [1.0]), gs.Shell(1, [1.3], [1.0])]],
                             renormalize=False)
    monkeypatch.setattr(gto_host, "D_MONOMIALS", ((((2, 0, 0), 1.0),),) * 5)     # where ``monomials`` reads it
    new = gd.spd_gaussian_mol(R, Z, [[gd.Shell(2, [a], [1.0]), gd.Shell(0, [a], [1.0])],
                                     [gd.Shell(0, [0.6], [1.0]), gd.Shell(1, [1.3], [1.0])]], need_grad=False,
                              renormalize=False)
    n_s, n_p, n_d = (float(gd.primitive_norm(l, a)) for l in (0, 1, 2))
    xx, s, rest = 0, 5, slice(6, 10)          # new: five copies of xx, then s, then the second centre
    want = n_p * (new.S[s, rest] / n_s - 2.0 * a * new.S[xx, rest] / n_d)
    assert np.abs(ref.ipovlp[0][0, 3:7] - want).max() < 1e-14
    want = n_p * (new.eri[s, rest, rest, rest] / n_s - 2.0 * a * new.eri[xx, rest, rest, rest] / n_d)
    assert np.abs(ref.eri_ip1[0][0, 3:7, 3:7, 3:7] - want).max() < 1e-14


def test_shell_limits():
    with pytest.raises(ValueError):
        gd.Shell(3, [1.0], [1.0])
    with pytest.raises(ValueError):
        gd.Shell(-1, [1.0], [1.0])
    with pytest.raises(ValueError):
        gs.Shell(2, [1.0], [1.0])                  # the s + p module keeps refusing d
    assert gd.Shell(2, [1.0], [1.0]).l == 2
    assert set(gd.BASES) == {"sto-3g", "6-31g", "cc-pvdz"} and gd.BASES["sto-3g"] is gs.STO3G
    charges, shells = gd.water_shells("cc-pvdz")
    assert sum(len(a) for a in shells) == 12
    assert sum(len(sh.exponents) for a in shells for sh in a) == 32
    assert sum(2 * sh.l + 1 for a in shells for sh in a) == 24
    # the tabulated contractions: the first O s has self-overlap 1.0010, the second (its diffuse member split off) 0.259
    o = shells[0]
    assert abs(gd.shell_self_overlap(o[0]) - 1.0010) < 5e-4 and abs(gd.shell_self_overlap(o[1]) - 0.259) < 5e-3


@pytest.fixture(scope="module")
def truth():
    return dc.load_truth()


@pytest.mark.parametrize("case", dc.TRUTH_CASES)
def test_truth_gate(truth, case):
    """The host statement against tests/golden/spdgto_truth.npz (closed s forms differentiated in mpmath, no Hermite
    expansion), per case and array; measured values: ``spdgto_cases.HOST_MEASURED``, gate: ``spdgto_cases.truth_gate``."""
    e = dc.host_truth_errors(truth, case)
    print(case, " ".join(f"{f}={e[f]:.1e}" for f in dc.TRUTH_FIELDS))
    for f in dc.TRUTH_FIELDS:
        assert e[f] < dc.truth_gate(case, f), (case, f, e[f])


def test_truth_sample_holds_every_class_and_component(truth):
    """The sample of eri / eri_ip1: in every case one element of every class of shell types the case has, (ss|ss) ...
    (dd|dd), with the three derivative directions; over the file every d component on every index position."""
    seen = set()
    for case in dc.TRUTH_CASES:
        kinds = []
        for sh_l in truth[f"{case}/shell_l"]:
            kinds += [(int(sh_l), c) for c in range(2 * int(sh_l) + 1)]
        idx = truth[f"{case}/eri_idx"]
        assert truth[f"{case}/eri_ip1_hi"].shape == (3, len(idx)) and not np.isnan(truth[f"{case}/eri_ip1_hi"]).any()
        classes = {tuple(kinds[i][0] for i in row) for row in idx}
        have = {l for l, _ in kinds}
        assert classes == {ls for ls in np.ndindex(3, 3, 3, 3) if set(ls) <= have}, case
        seen |= {(pos, kinds[i][1]) for row in idx for pos, i in enumerate(row) if kinds[i][0] == 2}
    assert seen == {(pos, c) for pos in range(4) for c in range(5)}


def test_boys_functions_on_the_grid():
    """F0 ... F9 of ``gto_small.boys`` on the 72 values of ``spdgto_cases.boys_grid`` (0 ... 1e5, the crossover from
    both sides) against mpmath at 50 digits.  Measured worst relative error per order: 2.8e-16, 2.5e-16, 4.0e-16,
    5.0e-16, 5.7e-16, 5.8e-16, 6.2e-16, 6.4e-16, 7.0e-16, 7.6e-16; gate: ten times the worst."""
    worst = dc.boys_grid_errors(9)
    print(worst)
    assert worst.max() < 7.6e-15
