"""CPU test of ``hchain.s_gaussian_mol`` against the exact values of tests/golden/sgto_truth.npz (mpmath,
tests/golden/make_sgto_truth.py): every array of every case within the bound of tests/sgto_reference.py,

    2^-53 [ (n_terms + 32) sum|terms| + c cancel + cond ],   c = C_CANCEL / 2,

elements whose addends all vanish exactly 0; and the constant ``c`` that bound is built on, measured here, is the one
written into sgto_reference.py."""
import math
import os

import numpy as np
import pytest

import sgto_reference as ref
from evcont_amd.hchain import s_gaussian_mol

TRUTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sgto_truth.npz")
CASES = ("3c_spread1.5_K3", "4c_K1", "K8", "far", "far_K1", "switch_K1", "switch_K3")


def load_case(T, case):
    """(R, Z, ex, co, {name: (hi, lo, sum|terms|, cancel, cond)}) of one case of the fixture."""
    R, Z, ex, co = (T[f"{case}/{k}"] for k in ("R", "Z", "ex", "co"))
    fields = {}
    for name in ref.NAMES:
        hi, lo, ab = T[f"{case}/{name}_hi"], T[f"{case}/{name}_lo"].astype(np.float64), T[f"{case}/{name}_abs"]
        zero = np.zeros_like(ab)
        fields[name] = (hi, lo, ab, T[f"{case}/{name}_cancel"] if name in ref.CANCEL_FIELDS else zero,
                        T[f"{case}/{name}_cond"] if f"{case}/{name}_cond" in T.files else zero)
    return R, Z, ex, co, fields


@pytest.fixture(scope="module")
def host():
    """case -> (A, K, fields, [s_gaussian_mol of every geometry]), computed once."""
    out = {}
    with np.load(TRUTH) as T:
        assert sorted({k.split("/")[0] for k in T.files}) == sorted(CASES)
        for case in CASES:
            R, Z, ex, co, fields = load_case(T, case)
            out[case] = (R.shape[1], len(ex), fields, [s_gaussian_mol(r, Z, ex, co) for r in R])
    return out


def test_fixture_holds_the_cases_of_sgto_reference():
    cases = ref.truth_cases()
    assert sorted(cases) == sorted(CASES)
    with np.load(TRUTH) as T:
        for case, (R, Z, ex, co) in cases.items():
            for key, want in (("R", R), ("Z", Z), ("ex", ex), ("co", co)):
                assert np.array_equal(T[f"{case}/{key}"], np.asarray(want, dtype=np.float64)), (case, key)


@pytest.mark.parametrize("case", CASES)
def test_s_gaussian_mol_within_half_the_device_bound(host, case):
    A, K, fields, mols = host[case]
    for name in ref.NAMES:
        hi, lo, ab, cancel, cond = fields[name]
        got = np.stack([np.asarray(getattr(m, name)) for m in mols])
        assert np.all(np.isfinite(got)), name
        assert np.all(got[ab == 0.0] == 0.0), (name, "an element whose addends all vanish is not exactly 0")
        ratio = ref.truth_ratio(name, A, K, got, hi, lo, ab, cancel, cond, c=ref.C_CANCEL / 2)
        print(f"{case} {name}: worst |s_gaussian_mol - truth| = {ratio:.3f} x bound(c = {ref.C_CANCEL / 2:g})")
        assert ratio <= 1.0, name


def test_the_measured_constant_is_the_recorded_one(host):
    need = 0.0
    for case in CASES:
        A, K, fields, mols = host[case]
        for name in ref.CANCEL_FIELDS:
            hi, lo, ab, cancel, cond = fields[name]
            got = np.stack([np.asarray(getattr(m, name)) for m in mols])
            c = ref.needed_c(name, A, K, np.abs((got - hi) - lo), ab, cancel, cond)
            print(f"{case} {name}: s_gaussian_mol needs c = {c:.3f}")
            need = max(need, c)
    print(f"measured c = {need:.3f}; recorded C_MEASURED = {ref.C_MEASURED}, chosen C_CANCEL = {ref.C_CANCEL}")
    assert need <= ref.C_MEASURED                      # erf / exp of another libm may need less, never more than recorded
    assert ref.C_CANCEL == math.ceil(2.0 * ref.C_MEASURED)
