"""CPU tests of the host statement with f shells (``evcont_amd.gto_spdf``, the l = 3 additions to ``gto_host``): the
monomial table against real solid harmonics, unit self-overlap, rotation through the numerically fitted 7 x 7
representation, translation, central differences, the Boys functions F0 ... F13 on the grid and the shell limits."""
import numpy as np
import pytest

import spdfgto_cases as fc
import spgto_cases as sc
from evcont_amd import gto_host
from evcont_amd import gto_spdf as gf


def table_functions(l, pts):
    """(npts, 2l+1): the functions of ``gto_host.monomials(l, .)`` at the points, without radial part and norm."""
    return np.stack([sum(w * pts[:, 0] ** i * pts[:, 1] ** j * pts[:, 2] ** k for (i, j, k), w in gto_host.monomials(l, c))
                     for c in range(2 * l + 1)], axis=1)


def real_solid_harmonics(l, pts):
    """(npts, 2l+1) r^l times the real spherical harmonics, m = -l ... l, from scipy (Condon-Shortley phase):
    m > 0: sqrt(2) (-1)^m Re Y_l^m, m < 0: sqrt(2) (-1)^m Im Y_l^|m|."""
    from scipy import special
    r = np.linalg.norm(pts, axis=1)
    polar, azim = np.arccos(pts[:, 2] / r), np.arctan2(pts[:, 1], pts[:, 0])
    if hasattr(special, "sph_harm_y"):
        Y = lambda m: special.sph_harm_y(l, m, polar, azim)
    else:
        Y = lambda m: special.sph_harm(m, l, azim, polar)
    cols = []
    for m in range(-l, l + 1):
        if m == 0:
            cols.append(Y(0).real)
        elif m > 0:
            cols.append(np.sqrt(2.0) * (-1) ** m * Y(m).real)
        else:
            cols.append(np.sqrt(2.0) * (-1) ** m * Y(-m).imag)
    return np.stack(cols, axis=1) * (r ** l)[:, None]


def test_monomial_table_is_the_real_solid_harmonics():
    """Order m = -3 ... 3, signs and relative weights: every column of the table is ONE positive constant times the
    real solid harmonic of its m (the constant is the norm of x y z exp(-a r^2) against that of the harmonic)."""
    pts = np.random.default_rng(0).standard_normal((40, 3))
    F, Y = table_functions(3, pts), real_solid_harmonics(3, pts)
    ratio = F / Y
    assert ratio.min() > 0 and np.abs(ratio / ratio[0, 0] - 1.0).max() < 1e-12
    # xyz has weight 1: r^3 Y_{3,-2} = sqrt(105 / 4 pi) x y z
    assert abs(ratio[0, 0] - 1.0 / np.sqrt(105.0 / (4.0 * np.pi))) < 1e-14
    assert max(len(gto_host.monomials(3, c)) for c in range(7)) == 3


@pytest.fixture(scope="module")
def small():
    R, Z, shells = fc.small_f()
    return R, Z, shells, gf.spdf_gaussian_mol(R, Z, shells)


def test_self_overlap_is_one(small):
    S = small[3].S
    assert np.abs(S[1:8, 1:8] - np.eye(7)).max() < 1e-14
    assert np.abs(np.diag(S) - 1.0).max() < 1e-14
    two = gf.Shell(3, [1.4, 0.5], [0.6, 0.5])
    c = gto_host.contraction_coefficients([[two]])[0][0]
    assert abs(gto_host.shell_self_overlap(gf.Shell(3, two.exponents, c)) - 1.0) < 1e-14
    m = gf.spdf_gaussian_mol(np.zeros((1, 3)), [1.0], [[two]], need_grad=False)
    assert np.abs(m.S - np.eye(7)).max() < 1e-14


def test_rotation(small):
    """S, hcore and eri of the rotated molecule are the originals under the rotation of the p block and the 7 x 7 real
    l = 3 representation, fitted from the functions at random points.  1e-13: the rounding of a four-index transform
    of O(1) numbers (tests/test_gto_spd_host.py)."""
    R, Z, shells, m0 = small
    rng = np.random.default_rng(3)
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] *= -1
    pts = rng.standard_normal((60, 3))
    # f_m(Q x) = sum_k D[k, m] f_k(x)
    D, res = np.linalg.lstsq(table_functions(3, pts), table_functions(3, pts @ Q.T), rcond=None)[:2]
    assert np.abs(res).max() < 1e-24 and np.abs(D.T @ D - np.eye(7)).max() < 1e-13
    m1 = gf.spdf_gaussian_mol(R @ Q.T, Z, shells, need_grad=False)
    n = m0.S.shape[0]
    U = np.zeros((n, n))
    f = 0
    for atom in shells:
        for sh in atom:
            k = 2 * sh.l + 1
            U[f:f + k, f:f + k] = {0: np.eye(1), 1: Q.T, 3: D}[sh.l]
            f += k
    assert sc.scaled_diff(m1.S, U.T @ m0.S @ U) < 1e-13
    assert sc.scaled_diff(m1.hcore, U.T @ m0.hcore @ U) < 1e-13
    assert sc.scaled_diff(m1.eri, np.einsum("pqrs,pa,qb,rc,sd->abcd", m0.eri, U, U, U, U, optimize=True)) < 1e-13
    assert abs(m1.enuc - m0.enuc) < 1e-13


def test_translation(small):
    R, Z, shells, m0 = small
    m1 = gf.spdf_gaussian_mol(R + np.array([0.4, -1.3, 0.8]), Z, shells)
    for k in sc.NAMES:
        assert sc.scaled_diff(getattr(m1, k), getattr(m0, k)) < 1e-13, k
    assert np.abs(m0.dhcore.sum(axis=0)).max() < 1e-12 * max(1.0, np.abs(m0.dhcore).max())


def test_derivatives_agree_with_central_differences(small):
    """ipovlp, dhcore, eri_ip1 and gnuc against central differences of S, hcore, eri and enuc (step and tolerance of
    tests/test_hchain_physics.py: h = 2e-4, 2e-7), for one coordinate of either centre; the dipole gradient against a
    central difference of the dipole integrals."""
    R, Z, shells, m = small
    h = 2e-4
    O = fc.REF_ORIGIN
    ipdip = m.dipole_grad_integrals(O)
    for at, d in ((0, 1), (1, 2)):
        Rp, Rm = R.copy(), R.copy()
        Rp[at, d] += h
        Rm[at, d] -= h
        mp, mm = (gf.spdf_gaussian_mol(x, Z, shells, need_grad=False) for x in (Rp, Rm))
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
        dd = np.zeros((3,) + m.S.shape)
        dd[:, s0:s1, :] -= ipdip[d, :, s0:s1, :]
        dd[:, :, s0:s1] -= ipdip[d, :, s0:s1, :].transpose(0, 2, 1)
        assert np.abs((mp.dipole_integrals(O) - mm.dipole_integrals(O)) / (2 * h) - dd).max() < 2e-7


def test_the_l2_entry_points_keep_their_limits():
    from evcont_amd import gto_spd as gd
    from evcont_amd import gto_spd_device, gto_spdf_device
    assert gf.Shell(3, [1.0], [1.0]).l == 3 and isinstance(gf.Shell(2, [1.0], [1.0]), gto_host.Shell)
    for bad in (4, -1):
        with pytest.raises(ValueError, match=f"l={bad}"):
            gf.Shell(bad, [1.0], [1.0])
    with pytest.raises(ValueError, match="l=3"):
        gd.Shell(3, [1.0], [1.0])
    assert sorted(gd.BASES) == ["6-31g", "cc-pvdz", "sto-3g"]
    with pytest.raises(ValueError, match="l=3"):
        gd.spd_gaussian_mol(np.zeros((1, 3)), [1.0], [[gf.Shell(3, [1.0], [1.0])]])
    assert gto_spd_device.DeviceSpdGaussians._LS == (0, 1, 2)
    assert gto_spdf_device.DeviceSpdfGaussians._LS == (0, 1, 2, 3)
    assert issubclass(gto_spdf_device.DeviceSpdfGaussians, gto_spd_device.DeviceSpdGaussians)
    assert gto_spdf_device.DeviceSpdfGaussians._DIPOLE_GRAD == "evc_spdfgto_dipole_grad_batch"


def test_device_producer_routing_by_shells():
    """A molecule with an f shell goes to the new class, tested before the l = 2 branch; the others keep their routes."""
    from types import SimpleNamespace
    from evcont_amd import gto_small as gs
    from evcont_amd.MD_utils import _device_producer
    mol = lambda shells: SimpleNamespace(shells=shells, charges=np.ones(len(shells)))
    f, d, p = gf.Shell(3, [1.0], [1.0]), gf.Shell(2, [1.0], [1.0]), gs.Shell(1, [1.0], [1.0])
    assert _device_producer(mol([[d, f], [p]])).__name__ == "DeviceSpdfGaussians"
    assert _device_producer(mol([[f]])).__name__ == "DeviceSpdfGaussians"
    assert _device_producer(mol([[d], [p]])).__name__ == "DeviceSpdGaussians"
    assert _device_producer(mol([[p]])).__name__ == "DeviceGaussians"


def test_tz_shape_water():
    table, R, Z, shells = fc.tz_shape_water()
    flat = gto_host.flatten_shells(shells, gto_host.contraction_coefficients(shells))
    assert flat[-1] == 58 and flat[3].shape[0] == 42
    assert sorted(sh.l for sh in shells[0]) == [0] * 4 + [1] * 3 + [2] * 2 + [3]
    assert sorted(sh.l for sh in shells[1]) == [0] * 3 + [1] * 2 + [2]
    assert [len(sh.exponents) for sh in shells[0][:2]] == [8, 8]
    assert "not" in fc.tz_shape_water.__doc__.lower() and "dunning" in fc.tz_shape_water.__doc__.lower()


def test_hermite_R_order_by_order_has_the_bits_of_the_recursion():
    """The level-by-level ``hermite_R`` against the plain recursion on every (t, u, v) up to total order 5, bit for bit."""
    rng = np.random.default_rng(4)
    alpha, X, Y, Z = rng.uniform(0.2, 3.0, 6), *rng.standard_normal((3, 6))
    L = 5
    F = gto_host.boys(L, alpha * (X * X + Y * Y + Z * Z))

    def R(t, u, v, n):
        if t == u == v == 0:
            return (-2.0 * alpha) ** n * F[n]
        if t > 0:
            r = X * R(t - 1, u, v, n + 1)
            return r + (t - 1) * R(t - 2, u, v, n + 1) if t > 1 else r
        if u > 0:
            r = Y * R(t, u - 1, v, n + 1)
            return r + (u - 1) * R(t, u - 2, v, n + 1) if u > 1 else r
        r = Z * R(t, u, v - 1, n + 1)
        return r + (v - 1) * R(t, u, v - 2, n + 1) if v > 1 else r

    got = gto_host.hermite_R(L, alpha, X, Y, Z)
    assert len(got) == (L + 1) * (L + 2) * (L + 3) // 6
    for (t, u, v), val in got.items():
        assert np.array_equal(val, R(t, u, v, 0)), (t, u, v)


def test_boys_functions_on_the_grid():
    """F0 ... F13 over ``spdfgto_cases.boys_grid`` against mpmath at 50 digits: within ten times the values measured on
    a CPU (``spdfgto_cases.BOYS_MEASURED``); no new crossover for the orders of f shells."""
    worst = fc.boys_grid_errors(13)
    print("boys F0..F13:", " ".join(f"{e:.1e}" for e in worst))
    assert np.all(worst <= 10 * np.array(fc.BOYS_MEASURED)), worst


@pytest.fixture(scope="module")
def truth():
    return fc.load_truth()


@pytest.mark.parametrize("case", fc.TRUTH_CASES)
def test_truth_gate(truth, case):
    """The host statement against tests/golden/spdfgto_truth.npz (closed s forms differentiated in mpmath, no
    McMurchie-Davidson), per array within ``spdfgto_cases.truth_gate``."""
    err = fc.host_truth_errors(truth, case)
    print(case, " ".join(f"{k} {v:.1e}" for k, v in err.items()))
    for k, v in err.items():
        assert v < fc.truth_gate(case, k), (case, k, v)


def test_truth_sample_holds_every_class_and_component(truth):
    """The eri sample: case b_flat holds one element of EVERY class of shell types with an f shell (175 of them), and
    over the file every f component stands on every index position."""
    seen = {pos: set() for pos in range(4)}
    for case in fc.TRUTH_CASES:
        shells = fc.truth_shells(truth, case)
        ls = np.concatenate([np.full(2 * sh.l + 1, sh.l) for atom in shells for sh in atom])
        comp = np.concatenate([np.arange(2 * sh.l + 1) for atom in shells for sh in atom])
        idx = truth[f"{case}/eri_idx"]
        classes = {tuple(ls[q]) for q in idx}
        assert all(3 in c for c in classes)
        have = sorted(set(ls))
        want = {c for c in __import__("itertools").product(have, repeat=4) if 3 in c}
        if case == "a":
            want = {c for c in want if c.count(3) <= 2}
        assert classes == want, (case, sorted(want - classes))
        for q in idx:
            for pos in range(4):
                if ls[q[pos]] == 3:
                    seen[pos].add(int(comp[q[pos]]))
        assert truth[f"{case}/ipdip_hi"].shape == (3, 3, len(ls), len(ls))
    assert all(seen[pos] == set(range(7)) for pos in range(4)), seen
    assert len({tuple(q) for q in truth["b_flat/eri_idx"]}) == 175
    assert __import__("os").path.getsize(fc.TRUTH) < 500_000
