"""CPU tests of the reference statements the s-Gaussian device integrals are held to (tests/sgto_reference.py): the plain
loops against ``hchain.s_gaussian_mol`` within the derived bound 2^-53 (n_terms + 432) sum|terms| per element, and the
vectorised sums of absolute addends (sum|terms|, cancel, cond) against those of the loops, and ``one_electron`` /
``eri_rows`` against both."""
import numpy as np
import pytest

import sgto_reference as ref
from evcont_amd.hchain import s_gaussian_mol

CASES = ref.host_cases()


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    R, Z, ex, co = CASES[request.param]
    return R, Z, ex, co, ref.loop_reference(R, Z, ex, co), s_gaussian_mol(R, Z, ex, co)


def _close(got, want):
    return got.shape == want.shape and np.all(np.abs(got - want) <= 1e-12 * np.abs(want))


def test_loops_agree_with_s_gaussian_mol(case):
    R, Z, ex, co, loops, mol = case
    A, K = len(Z), len(ex)
    for name in ref.NAMES:
        value, sums = loops[name]
        ratio = ref.worst_ratio(name, A, K, getattr(mol, name), value, sums)
        print(f"{name}: worst |loops - s_gaussian_mol| = {ratio:.1f} x 2^-53 sum|terms| "
              f"(bound {ref.n_terms(name, A, K) + ref.ROUNDINGS})")
        assert ratio <= ref.n_terms(name, A, K) + ref.ROUNDINGS, name
        assert np.all(np.abs(np.asarray(getattr(mol, name)) - value) <= ref.allowed(name, A, K, sums)), name


def test_vectorised_abs_sums_agree_with_the_loops(case):
    R, Z, ex, co, loops, _ = case
    sums = ref.abs_sums(R, Z, ex, co)
    for name in ref.NAMES:
        want = loops[name][1]
        assert sums[name].shape == want.shape, name
        assert np.all(np.abs(sums[name] - want) <= 1e-12 * np.abs(want)), name


def test_vectorised_cancel_and_cond_agree_with_the_loops(case):
    R, Z, ex, co, _, _ = case
    _, cancel_l, cond_l = ref.loop_reference(R, Z, ex, co, with_cancel=True)
    _, cancel_v, cond_v = ref.abs_sums(R, Z, ex, co, with_cancel=True)
    assert sorted(cancel_l) == sorted(cancel_v) == sorted(ref.CANCEL_FIELDS)
    for name in ref.CANCEL_FIELDS:
        assert _close(cancel_v[name], cancel_l[name]), name
        assert np.any(cancel_l[name] > 0.0), name
    for name in ref.NAMES:
        assert _close(cond_v[name], cond_l[name]), name


def test_one_electron_and_eri_rows_agree_with_s_gaussian_mol_and_abs_sums(case):
    R, Z, ex, co, _, mol = case
    A, K = len(Z), len(ex)
    sums, cancel, cond = ref.abs_sums(R, Z, ex, co, with_cancel=True)
    zero = lambda name: np.zeros_like(sums[name])
    for name, (value, ab, cc, kd) in ref.one_electron(R, Z, ex, co).items():
        assert np.all(np.abs(value - np.asarray(getattr(mol, name))) <= ref.allowed(name, A, K, sums[name])), name
        assert _close(ab, sums[name]) and _close(cc, cancel.get(name, zero(name))) and _close(kd, cond[name]), name
    pairs = [(i, j) for i in range(A) for j in range(A)]
    rows = ref.eri_rows(R, ex, co, pairs)
    flat = {"eri": lambda X: X.reshape(A * A, A, A), "eri_ip1": lambda X: np.moveaxis(X.reshape(3, A * A, A, A), 0, 1)}
    for name, (value, ab, cc, kd) in rows.items():
        f = flat[name]
        assert np.all(np.abs(value - f(np.asarray(getattr(mol, name)))) <= f(ref.allowed(name, A, K, sums[name]))), name
        assert _close(ab, f(sums[name])) and _close(cc, f(cancel.get(name, zero(name)))) and _close(kd, f(cond[name])), name


def test_one_electron_and_eri_rows_at_five_centres():
    """Beyond the four centres of the loops: a perturbed chain of five, STO-3G, charges 1, 2, 0.5 in turn."""
    from evcont_amd.hchain import STO3G_H_COEFFICIENTS as co, STO3G_H_EXPONENTS as ex
    R, Z, A, K = ref._perturbed_chain(5, 1, 7)[0], [1.0, 2.0, 0.5, 1.0, 2.0], 5, 3
    mol = s_gaussian_mol(R, Z, ex, co)
    sums, cancel, cond = ref.abs_sums(R, Z, ex, co, with_cancel=True)
    for name, (value, ab, cc, kd) in ref.one_electron(R, Z, ex, co).items():
        assert np.all(np.abs(value - np.asarray(getattr(mol, name))) <= ref.allowed(name, A, K, sums[name])), name
        assert _close(ab, sums[name]) and _close(kd, cond[name]), name
    pairs = [(0, 0), (4, 4), (4, 0), (0, 4), (2, 3), (3, 2)]
    rows = ref.eri_rows(R, ex, co, pairs)
    for b, (i, j) in enumerate(pairs):
        assert np.all(np.abs(rows["eri"][0][b] - mol.eri[i, j]) <= ref.allowed("eri", A, K, sums["eri"][i, j]))
        assert np.all(np.abs(rows["eri_ip1"][0][b] - mol.eri_ip1[:, i, j]) <=
                      ref.allowed("eri_ip1", A, K, sums["eri_ip1"][:, i, j]))
        assert _close(rows["eri"][1][b], sums["eri"][i, j]) and _close(rows["eri_ip1"][1][b], sums["eri_ip1"][:, i, j])
        assert _close(rows["eri_ip1"][2][b], cancel["eri_ip1"][:, i, j])
        assert _close(rows["eri"][3][b], cond["eri"][i, j]) and _close(rows["eri_ip1"][3][b], cond["eri_ip1"][:, i, j])
