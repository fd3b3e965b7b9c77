"""The numpy statement of the observables (evcont_amd/properties.py, HChainMol.dipole_integrals) against independent
answers: Gauss-Hermite quadrature for the s-Gaussian dipole integrals, sum rules, the origin shift, and the
Hellmann-Feynman theorem (the dipole is the derivative of the energy with respect to a uniform field).  No device."""
import dataclasses

import numpy as np
import pytest

from evcont_amd import properties as pr
from evcont_amd.hchain import (STO3G_H_COEFFICIENTS, STO3G_H_EXPONENTS, STO6G_H_COEFFICIENTS, STO6G_H_EXPONENTS,
                               s_gaussian_mol)
from oracle import evcont_oracle as orc

# the hetero-charged bent H4 of the device tests: no symmetry makes a dipole component vanish
H4_COORDS = np.array([[0.0, 0.0, 0.0], [1.7, 0.3, 0.0], [2.9, 1.6, 0.4], [4.4, 1.9, -0.7]])
H4_CHARGES = (1.0, 2.0, 0.5, 1.0)
# Field strength of the central difference and its tolerance, from the scan of this file's run (`python
# tests/test_properties_host.py`, scan_field below, the larger gap of roots 0 and 1):
#     F      1e-2     1e-3     1e-4     1e-5     1e-6     1e-7
#     gap    2.04e-5  2.04e-7  2.04e-9  1.7e-11  1.7e-10  2.3e-9
# Down to 1e-5 the gap is the truncation error of the central difference, 0.204 F^2; below, the rounding of the energies
# divided by 2 F takes over (the numpy oracle's energies carry ~2e-16: 2e-16 / F).  The device route of the same check
# (tests/test_gpu_properties.py) differences energies that carry the tolerance of the device eigensolvers, ~1e-14
# relative (README.md), ~1e-13 absolute here: 5e-9 at F = 1e-5 but 5e-10 at F = 1e-4.  So F = 1e-4, the smallest field of
# the scan at which the truncation error (2.04e-9, known from the F^2 law) still dominates the rounding of both routes,
# and the tolerance is that truncation error with a factor of 2.5.
HF_FIELD = 1.0e-4
HF_TOL = 5.0e-9


def quadrature_dipole(coords, exponents, coefficients, origin, nodes=12):
    """<mu| r - O |nu> of contracted s Gaussians by Gauss-Hermite quadrature in each Cartesian direction: per primitive
    pair the exponent -a (x - A)^2 - b (x - B)^2 is a parabola -p (x - x0)^2 + q0; with x = x0 + t / sqrt(p) the
    integrand is exp(-t^2) times a polynomial of degree <= 1, for which the rule is exact."""
    t, w = np.polynomial.hermite.hermgauss(nodes)
    R = np.asarray(coords, dtype=np.float64)
    ex, co = np.asarray(exponents), np.asarray(coefficients)
    cn = co * (2.0 * ex / np.pi) ** 0.75
    n = R.shape[0]
    out = np.zeros((3, n, n))
    for i in range(n):
        for j in range(n):
            for a, ca in zip(ex, cn):
                for b, cb in zip(ex, cn):
                    p = a + b
                    m0, m1 = np.zeros(3), np.zeros(3)     # int g dx and int (x - O) g dx per direction
                    for d in range(3):
                        A, B = R[i, d], R[j, d]
                        x0 = (a * A + b * B) / p
                        x = x0 + t / np.sqrt(p)
                        g = np.exp(-a * (x - A) ** 2 - b * (x - B) ** 2 + t * t) * w / np.sqrt(p)
                        m0[d], m1[d] = np.sum(g), np.sum(g * (x - origin[d]))
                    for d in range(3):
                        out[d, i, j] += ca * cb * m1[d] * np.prod(np.delete(m0, d))
    return out


@pytest.mark.parametrize("basis", ["sto3g", "sto6g"])
@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (0.7, -1.3, 2.1)])
def test_dipole_integrals_against_quadrature(basis, origin):
    ex, co = ((STO3G_H_EXPONENTS, STO3G_H_COEFFICIENTS) if basis == "sto3g" else
              (STO6G_H_EXPONENTS, STO6G_H_COEFFICIENTS))
    mol = s_gaussian_mol(H4_COORDS, H4_CHARGES, ex, co, need_grad=False)
    got = mol.dipole_integrals(origin)
    want = quadrature_dipole(H4_COORDS, ex, co, origin)
    assert got.shape == (3, 4, 4)
    assert np.abs(got - want).max() < 1e-13, np.abs(got - want).max()
    assert np.array_equal(got, got.transpose(0, 2, 1))
    # <mu| r - O |nu> = <mu| r |nu> - O S
    np.testing.assert_allclose(got, mol.dipole_integrals() - np.asarray(origin)[:, None, None] * mol.S, atol=1e-14)


def test_dipole_integrals_two_functions_on_one_centre():
    """Coincident centres: the pair centre is the centre exactly, so the block is (R - O) S to the last bit."""
    coords = H4_COORDS.copy()
    mol = s_gaussian_mol(coords, H4_CHARGES, need_grad=False)
    coords[2] = coords[1]
    two = dataclasses.replace(mol, coords=coords)
    origin = (0.25, 0.5, -1.0)
    got = two.dipole_integrals(origin)
    want = quadrature_dipole(coords, STO3G_H_EXPONENTS, STO3G_H_COEFFICIENTS, origin)
    assert np.abs(got - want).max() < 1e-13
    s12 = got[:, 1, 2] / (coords[1] - np.asarray(origin))
    assert np.abs(s12 - s12[0]).max() < 1e-15 and abs(s12[0] - 1.0) < 1e-7      # STO-3G is normalised to ~1e-8
    assert np.array_equal(got[:, 1, 1], got[:, 1, 2]) and np.array_equal(got[:, 1, 1], got[:, 2, 2])


def test_population_sums_on_a_golden_case(load_golden):
    """Any 1-RDM: the Mulliken and the Loewdin populations both add up to tr D (X S X = 1)."""
    g = load_golden("n5t4a2")
    C = g["ms_C_full6_h"]
    pairs = [(0, 0), (0, 1), (1, 1), (1, 2), (2, 2)]
    rng = np.random.default_rng(3)
    dip = rng.standard_normal((3, 5, 5))
    res = pr.properties_host(g["one_RDM"], g["X"], C, pairs, g["S"], dip + dip.transpose(0, 2, 1), g["aoslices"],
                             np.array([3.0, 2.0]), rng.standard_normal((2, 3)))
    for p in range(len(pairs)):
        tr = np.trace(res["d_oao"][p])
        assert abs(res["mulliken"][p].sum() - tr) < 1e-12 and abs(res["loewdin"][p].sum() - tr) < 1e-12
        assert abs(np.trace(res["d_ao"][p] @ g["S"]) - tr) < 1e-12
    np.testing.assert_allclose(res["d_oao"][0], pr.predicted_one_rdm(g["one_RDM"], C[0]), atol=0)
    np.testing.assert_allclose(res["d_ao"][1], pr.predicted_one_rdm_ao(g["one_RDM"], g["X"], C[0], C[1]), atol=0)


@pytest.fixture(scope="module")
def h10(h10_fci):
    """Physical training data (H10 / STO-3G, 5 FCI states): tr one_rdm[a,b] = N_elec S_train[a,b]."""
    mol = s_gaussian_mol(h10_fci["R_test"], need_grad=False)
    b = orc.AOBundle(mol.S, mol.hcore, mol.eri, mol.ipovlp, mol.dhcore, mol.eri_ip1, mol.aoslices, mol.enuc, mol.gnuc)
    E, C = orc.approximate_multistate_OAO(b, h10_fci["one_rdm"], h10_fci["two_rdm_pack2"], h10_fci["overlap"], 3)
    return mol, h10_fci["one_rdm"], orc.loewdin_trafo(mol.S), C


def h10_props(h10, pairs, origin=(0.0, 0.0, 0.0), charges=None):
    mol, one, X, C = h10
    return pr.properties_host(one, X, C, pairs, mol.S, mol.dipole_integrals(origin), mol.aoslices,
                              mol.charges if charges is None else charges, mol.coords, origin)


def test_electron_count_sum_rules(h10):
    """Physical t-RDMs: a state's populations add up to the electrons, a transition density's between S-orthonormal
    roots to zero; Mulliken and Loewdin sums agree."""
    pairs = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]
    res = h10_props(h10, pairs)
    for p, (k, l) in enumerate(pairs):
        want = 10.0 if k == l else 0.0
        assert abs(res["mulliken"][p].sum() - want) < 1e-10, (k, l, res["mulliken"][p].sum())
        assert abs(res["loewdin"][p].sum() - want) < 1e-10
        assert abs(res["mulliken"][p].sum() - res["loewdin"][p].sum()) < 1e-11
    q = pr.charges_from_populations(res["mulliken"], h10[0].charges, pairs)
    assert np.abs(q.sum(axis=-1)).max() < 1e-10       # neutral molecule, traceless transition densities


@pytest.mark.parametrize("charged", [False, True])
def test_origin_shift(h10, charged):
    """mu(O + d) - mu(O) = -q_total d on the diagonal slots, 0 on the transition slots."""
    mol = h10[0]
    Z = np.array(mol.charges, dtype=np.float64)
    if charged:
        Z[3] += 1.0            # the cation's nuclear frame with the neutral density: q_total = +1
    pairs = [(0, 0), (1, 1), (0, 1), (1, 2)]
    O, d = np.array([0.3, -0.2, 0.9]), np.array([1.1, 0.4, -2.0])
    a, b = h10_props(h10, pairs, O, Z), h10_props(h10, pairs, O + d, Z)
    q_total = Z.sum() - 10.0
    assert q_total == (1.0 if charged else 0.0)
    for p, (k, l) in enumerate(pairs):
        want = -q_total * d if k == l else np.zeros(3)
        assert np.abs(b["dipole"][p] - a["dipole"][p] - want).max() < 1e-10, (k, l)


def test_dip_moment_units_and_oscillator_strength():
    rng = np.random.default_rng(5)
    P = rng.standard_normal((4, 4))
    r = rng.standard_normal((3, 4, 4))
    Z, R = np.array(H4_CHARGES), H4_COORDS
    au = pr.dip_moment(Z, R, r, P)
    np.testing.assert_allclose(au, Z @ R - np.array([np.trace(P @ r[x]) for x in range(3)]), atol=1e-13)
    np.testing.assert_allclose(pr.dip_moment(Z, R, r, P, unit="Debye"), au * 2.541746473, rtol=1e-15)
    np.testing.assert_allclose(pr.dip_moment(Z, R, r, P, transition=True),
                               -np.array([np.trace(P @ r[x]) for x in range(3)]), atol=1e-13)
    with pytest.raises(ValueError):
        pr.dip_moment(Z, R, r, P, unit="esu")
    assert pr.oscillator_strength(-1.0, -0.5, [0.3, 0.0, 0.4]) == pytest.approx(2.0 / 3.0 * 0.5 * 0.25)
    np.testing.assert_allclose(pr.mulliken_pop(P, np.eye(4), [[0, 1], [1, 4]]), [P[0, 0], np.trace(P[1:, 1:])])
    np.testing.assert_allclose(pr.loewdin_pop(P, [[0, 3], [3, 4]]), [np.trace(P[:3, :3]), P[3, 3]])


def h4_problem():
    """The hetero-charged bent H4 with a synthetic (bra<->ket symmetric) training set of 3 states."""
    from evcont_amd.synthetic import make_trdms
    mol = s_gaussian_mol(H4_COORDS, H4_CHARGES)
    S_train, one, two = make_trdms(4, 3, 41)
    return mol, S_train, one, two


def in_field(mol, F, x=0):
    """hcore -> hcore + F r_x (origin 0): the molecule in a uniform field along x."""
    return dataclasses.replace(mol, hcore=mol.hcore + F * mol.dipole_integrals()[x])


def oracle_electronic(mol, one, two, S_train, nroots):
    b = orc.AOBundle(mol.S, mol.hcore, mol.eri, mol.ipovlp, mol.dhcore, mol.eri_ip1, mol.aoslices, 0.0, mol.gnuc)
    return orc.approximate_multistate_OAO(b, one, two, S_train, nroots)


def scan_field(fields=(1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7)):
    """|central difference of the oracle's electronic energy - tr(P r_x)| for roots 0 and 1, per field strength."""
    mol, S_train, one, two = h4_problem()
    _, C = oracle_electronic(mol, one, two, S_train, 2)
    X, r = orc.loewdin_trafo(mol.S), mol.dipole_integrals()
    want = np.array([np.trace(pr.predicted_one_rdm_ao(one, X, C[k]) @ r[0]) for k in range(2)])
    gaps = {}
    for F in fields:
        ep = oracle_electronic(in_field(mol, +F), one, two, S_train, 2)[0]
        em = oracle_electronic(in_field(mol, -F), one, two, S_train, 2)[0]
        gaps[F] = float(np.abs((ep - em) / (2.0 * F) - want).max())
    return gaps, want


def test_hellmann_feynman_on_the_oracle():
    """The dipole is a derivative of the energy: the central difference of the oracle's electronic energy in the field
    hcore +- F r_x equals tr(P r_x) of the predicted AO 1-RDM, for roots 0 and 1."""
    gaps, want = scan_field((HF_FIELD,))
    print("Hellmann-Feynman gap at F = %g: %.3e (tr(P r_x) = %s)" % (HF_FIELD, gaps[HF_FIELD], want))
    assert np.abs(want).min() > 1e-2                 # not zero by symmetry
    assert gaps[HF_FIELD] < HF_TOL, gaps


if __name__ == "__main__":
    for F, gap in scan_field()[0].items():
        print(f"F = {F:8.1e}   gap = {gap:.3e}")
