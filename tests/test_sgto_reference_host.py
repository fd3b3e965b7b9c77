"""CPU tests of the reference statements the s-Gaussian device integrals are held to (tests/sgto_reference.py): the plain
loops against ``hchain.s_gaussian_mol`` within the derived bound 2^-53 (n_terms + 432) sum|terms| per element, and the
vectorised sums of absolute addends against those of the loops."""
import numpy as np
import pytest

import sgto_reference as ref
from evcont_amd.hchain import s_gaussian_mol

CASES = ref.host_cases()


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    R, Z, ex, co = CASES[request.param]
    return R, Z, ex, co, ref.loop_reference(R, Z, ex, co), s_gaussian_mol(R, Z, ex, co)


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
