"""CPU tests of S^2 and the spin penalty on the host: ``fci_small.spin_square_vector``, ``SmallFCI(spin_penalty=...)``,
``fci_tables.spin_square_through_tables`` (the numpy statement of the device kernel) and the numpy Davidson with the
penalty in its sigma vector and its diagonal.

Reference energies (electronic, OAO basis, STO-3G hydrogen chain) are those of the dense host solve; the singlet ones are
roots of the plain Hamiltonian as well, which the tests check where both are at hand."""
import warnings

import numpy as np
import pytest

from evcont_amd.fci_davidson import NumpyOps, davidson, hdiag_numpy
from evcont_amd.fci_small import SmallFCI, fix_spin_, spin_square_vector
from evcont_amd.fci_tables import spin_square_through_tables
from test_fci_davidson_host import oao_integrals

_HOST = SmallFCI()
SHAPES = [(4, (2, 2)), (5, (3, 2)), (6, (3, 3)), (6, (4, 2))]
H6_PLAIN = {1.8: [-8.077851, -7.885217, -7.690716, -7.648414], 3.0: [-5.857646, -5.816260, -5.769089, -5.752980]}
H6_SINGLETS = {1.8: [-8.077851, -7.648414, -7.623083, -7.506330], 3.0: [-5.857646, -5.752980, -5.716540, -5.663719]}


def dims(norb, nelec):
    _, _, na, nb = _HOST._ops(norb, nelec)
    return na, nb


def dense(apply, na, nb):
    dim = na * nb
    eye = np.eye(dim)
    return np.array([apply(eye[k].reshape(na, nb)).reshape(-1) for k in range(dim)]).T


@pytest.mark.parametrize("norb,nelec", SHAPES)
def test_s2_is_symmetric_commutes_with_h_and_has_the_spectrum_of_the_multiplicities(norb, nelec):
    na, nb = dims(norb, nelec)
    S2 = dense(lambda c: spin_square_vector(c, norb, nelec), na, nb)
    assert np.array_equal(S2, S2.T)
    h1, h2 = oao_integrals(norb)
    H = dense(lambda c: _HOST.contract(h1, h2, c, norb, nelec), na, nb)
    assert np.abs(H @ S2 - S2 @ H).max() < 1e-12 * max(1.0, np.abs(H).max())
    sz, n = 0.5 * (nelec[0] - nelec[1]), nelec[0] + nelec[1]
    want = sorted(s * (s + 1) for s in np.arange(abs(sz), min(n, 2 * norb - n) / 2 + 0.5))
    got = sorted(set(np.round(np.linalg.eigvalsh(S2), 9)))
    assert got == want, (got, want)
    if (norb, nelec) == (6, (3, 3)):
        assert got == [0, 2, 6, 12]
    if (norb, nelec) == (5, (3, 2)):
        assert got == [0.75, 3.75, 8.75]
    # eigenvectors of H are eigenvectors of S^2
    e, v = _HOST.kernel(h1, h2, norb, nelec, nroots=3)
    for x in v:
        ss, mult = _HOST.spin_square(x, norb, nelec)
        assert np.linalg.norm(spin_square_vector(x, norb, nelec) - ss * x) < 1e-12
        assert abs(mult - (2 * (np.sqrt(ss + 0.25) - 0.5) + 1)) < 1e-14


@pytest.mark.parametrize("norb,nelec", SHAPES + [(3, (2, 0)), (2, (1, 1))])
def test_diagonal_formula_and_the_table_statement_bit_for_bit(norb, nelec):
    na, nb = dims(norb, nelec)
    S2 = dense(lambda c: spin_square_vector(c, norb, nelec), na, nb)
    zero = np.zeros((norb, norb)), np.zeros((norb,) * 4)
    d = hdiag_numpy(*zero, norb, nelec, spin_penalty=1.0, spin_target=0.0)
    assert np.array_equal(d.reshape(-1), np.diag(S2))
    assert np.array_equal(hdiag_numpy(*zero, norb, nelec, spin_penalty=0.5, spin_target=0.75).reshape(-1),
                          0.5 * (np.diag(S2) - 0.75))
    rng = np.random.default_rng(norb)
    c = rng.integers(-3, 4, size=(na, nb)).astype(np.float64)
    o = rng.integers(-3, 4, size=(na, nb)).astype(np.float64)
    want = spin_square_vector(c, norb, nelec)
    assert np.array_equal(spin_square_through_tables(c, norb, nelec), want)
    assert np.array_equal(spin_square_through_tables(c, norb, nelec, alpha=0.5, ss=0.75, beta=1.0, out=o),
                          o + 0.5 * (want - 0.75 * c))
    x = rng.standard_normal((na, nb))
    assert np.abs(spin_square_through_tables(x, norb, nelec) - spin_square_vector(x, norb, nelec)).max() < 1e-13


def test_known_answers():
    # a closed-shell determinant is a singlet
    norb, nelec = 4, (2, 2)
    na, nb = dims(norb, nelec)
    c = np.zeros((na, nb))
    c[0, 0] = 1.0                                   # orbitals 0, 1 doubly occupied
    assert np.array_equal(spin_square_vector(c, norb, nelec), np.zeros((na, nb)))
    assert np.array_equal(spin_square_through_tables(c, norb, nelec), np.zeros((na, nb)))
    # no beta electron: every state has S = Sz
    rng = np.random.default_rng(1)
    for norb, n in ((4, 2), (5, 3), (6, 3)):
        na, nb = dims(norb, (n, 0))
        assert nb == 1
        c = rng.integers(-3, 4, size=(na, 1)).astype(np.float64)
        k = 0.5 * n * (0.5 * n + 1)
        assert np.array_equal(spin_square_vector(c, norb, (n, 0)), k * c)
        assert np.array_equal(spin_square_through_tables(c, norb, (n, 0)), k * c)


@pytest.mark.parametrize("d", [1.8, 3.0])
def test_h6_penalty_gives_the_singlets_and_the_plain_solver_a_mix(d):
    h1, h2 = oao_integrals(6, d)
    plain = SmallFCI()
    e, v = plain.kernel(h1, h2, 6, (3, 3), nroots=4)
    assert np.abs(np.array(e) - H6_PLAIN[d]).max() < 6e-7
    assert plain.spin_squares is None
    assert np.abs(np.array([plain.spin_square(x, 6, (3, 3))[0] for x in v]) - [0, 2, 2, 0]).max() < 1e-8
    pure = SmallFCI(spin_penalty=0.2)
    es, vs = pure.kernel(h1, h2, 6, (3, 3), nroots=4)
    assert np.abs(np.array(es) - H6_SINGLETS[d]).max() < 6e-7                    # the recorded figures, six decimals
    assert np.abs(np.array(pure.spin_squares)).max() < 1e-8
    # to 1e-9: the singlets among the eigenvalues of the plain dense matrix
    w, u = np.linalg.eigh(dense(lambda c: plain.contract(h1, h2, c, 6, (3, 3)), 20, 20))
    ss = np.array([plain.spin_square(u[:, k], 6, (3, 3))[0] for k in range(60)])
    singlets = w[:60][np.abs(ss) < 1e-8][:4]
    assert np.abs(np.array(es) - singlets).max() < 1e-9
    assert abs(es[1] - e[3]) < 1e-9 and abs(es[0] - e[0]) < 1e-9
    for x in vs:
        assert abs(pure.spin_square(x, 6, (3, 3))[1] - 1.0) < 1e-7


def test_ms1_roots_are_the_plain_triplets():
    h1, h2 = oao_integrals(6, 1.8)
    e0, _ = SmallFCI().kernel(h1, h2, 6, (3, 3), nroots=3)
    for solver in (SmallFCI(), SmallFCI(spin_penalty=0.2)):
        e1, v1 = solver.kernel(h1, h2, 6, (4, 2), nroots=2)
        assert np.abs(np.array(e1) - [-7.885217, -7.690716]).max() < 6e-7
        assert np.abs(np.array(e1) - e0[1:3]).max() < 1e-9
        assert np.abs(np.array([solver.spin_square(x, 6, (4, 2))[0] for x in v1]) - 2.0).max() < 1e-8


def test_h4_fourth_root_is_a_triplet_returned_with_its_energy_and_a_warning():
    h1, h2 = oao_integrals(4, 1.8)
    solver = SmallFCI(spin_penalty=0.2)
    with pytest.warns(RuntimeWarning, match="root 3") as rec:
        e, v = solver.kernel(h1, h2, 4, (2, 2), nroots=4)
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert "larger spin_penalty" in str(rec[0].message) and "fewer roots" in str(rec[0].message)
    assert abs(e[3] - (-4.325077)) < 6e-7
    assert abs(solver.spin_squares[3] - 2.0) < 1e-8 and np.abs(solver.spin_squares[:3]).max() < 1e-8
    assert abs(e[3] - solver.energy(h1, h2, v[3], 4, (2, 2))) < 1e-10            # the energy of H, not the shifted one
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        solver.kernel(h1, h2, 4, (2, 2), nroots=3)


def test_numpy_davidson_with_the_penalty_h8():
    h1, h2 = oao_integrals(8, 1.8)
    solver = SmallFCI(spin_penalty=0.2)
    ops = NumpyOps(h1, h2, 8, (4, 4), solver=solver)
    e, v, conv, info = davidson(ops, nroots=3, conv_tol=1e-8)
    assert conv
    assert np.abs(e - [-11.950523, -11.606001, -11.562580]).max() < 6e-7
    for x in v:
        assert abs(solver.spin_square(x / np.linalg.norm(x), 8, (4, 4))[0]) < 1e-8
    # the diagonal the preconditioner used is that of the operator contracted
    k = int(np.argmin(ops.hdiag))
    unit = np.zeros(ops.dim)
    unit[k] = 1.0
    assert abs(solver.contract(h1, h2, unit.reshape(70, 70), 8, (4, 4)).reshape(-1)[k] - ops.hdiag[k]) < 1e-12


def test_a_target_that_is_no_s_s_plus_1_is_refused():
    h1, h2 = oao_integrals(4, 1.8)
    for target, nelec in ((1.0, (2, 2)), (0.0, (3, 1)), (0.75, (2, 2)), (12.0, (2, 2))):
        with pytest.raises(ValueError, match="spin_target"):
            SmallFCI(spin_penalty=0.2, spin_target=target).kernel(h1, h2, 4, nelec)
    e, _ = SmallFCI(spin_penalty=0.2, spin_target=2.0).kernel(h1, h2, 4, (3, 1))
    e2, _ = fix_spin_(SmallFCI(), shift=0.2, ss=2.0).kernel(h1, h2, 4, (3, 1))
    assert e == e2
    s = fix_spin_(SmallFCI())
    assert s.spin_penalty == 0.2 and s.spin_target is None


def test_penalty_zero_changes_no_bit():
    h1, h2 = oao_integrals(6, 1.8)
    for nelec in ((3, 3), (4, 2)):
        e0, v0 = SmallFCI().kernel(h1, h2, 6, nelec, nroots=3)
        e1, v1 = SmallFCI(spin_penalty=0.0, spin_target=None).kernel(h1, h2, 6, nelec, nroots=3)
        assert np.array_equal(e0, e1) and all(np.array_equal(a, b) for a, b in zip(v0, v1))
        c = np.random.default_rng(0).standard_normal(v0[0].shape)
        assert np.array_equal(SmallFCI().contract(h1, h2, c, 6, nelec),
                              SmallFCI(spin_penalty=0.0).contract(h1, h2, c, 6, nelec))
        assert np.array_equal(hdiag_numpy(h1, h2, 6, nelec), hdiag_numpy(h1, h2, 6, nelec, 0.0, 0.0))
