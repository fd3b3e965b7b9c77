"""GPU tests of the device AO integrals of s, p, d and f shells (csrc/spdfgto.hip) through the C calls, on NaN-poisoned
fenced buffers (tests/spdfgto_harness.py): against the host statement ``gto_spdf.spdf_gaussian_mol`` in the full, s4
and s2kl forms with and without EVC_FLAG_ENERGY_ONLY -- recorded host arrays (tests/golden/spdfgto_host_refs.npz) for the
N = 23 molecule whose kets span five blocks and which has every class of pair, and for the one-centre atom; the host
statement itself on the N = 11 molecule --, the dipole integrals and their gradient, the bit guarantees (run to run,
batch against single, packed against full, the exact symmetries), and an s + p + d molecule against ``evc_spdgto_*``.

Gate: ``spgto_cases.DEVICE_HOST_GATE`` (1e-10) under ``scaled_diff``, max |x - ref| / max(1, max |ref|) per array."""
import numpy as np
import pytest

import spdfgto_cases as fc
from spdfgto_harness import ENERGY, S2KL, S4, Basis, pack_eri, pack_ip1, run, run_dipole, run_dipole_grad

pytestmark = pytest.mark.gpu

FORMS = [0, S4, S2KL, S4 | S2KL, ENERGY, ENERGY | S4]


@pytest.fixture(scope="module")
def refs():
    return fc.load_host_refs()


def full_forms(arrays, n, flags):
    out = {k: v[0] for k, v in arrays.items()}
    if flags & S4:
        out["eri"] = fc.unpack_eri(out["eri"], n)
    if flags & S2KL and "eri_ip1" in out:
        out["eri_ip1"] = fc.unpack_ip1(out["eri_ip1"], n)
    return out


@pytest.mark.parametrize("flags", FORMS, ids=lambda f: f"flags{f}")
@pytest.mark.parametrize("name", sorted(fc.HOST_REF_CASES))
def test_device_against_the_recorded_host_statement(refs, name, flags):
    R, Z, shells = fc.HOST_REF_CASES[name]()
    basis = Basis(Z, shells)
    rc, arrays, intact, _ = run(R, basis, flags)
    assert rc == 0 and intact
    got = full_forms(arrays, basis.nao, flags)
    names = ("enuc", "S", "hcore", "eri") if flags & ENERGY else fc.NAMES
    for k in names:
        assert not np.isnan(got[k]).any(), k
    for k, d in fc.ref_diffs(got, refs, name, names).items():
        print(name, flags, k, "%.1e" % d)
        assert d < fc.DEVICE_HOST_GATE, (k, d)
    if flags & ENERGY:
        # the gradient arrays of an energy-only call stay untouched
        for k in ("ipovlp", "dhcore", "eri_ip1", "gnuc"):
            assert np.isnan(arrays[k]).all(), k


@pytest.mark.parametrize("name", sorted(fc.HOST_REF_CASES))
def test_dipoles_against_the_recorded_host_statement(refs, name):
    R, Z, shells = fc.HOST_REF_CASES[name]()
    basis = Basis(Z, shells)
    rc, dip, intact, _ = run_dipole(R, basis, fc.REF_ORIGIN)
    assert rc == 0 and intact and not np.isnan(dip).any()
    d = fc.scaled_diff(dip[0], refs[f"{name}/dip"])
    rc, ipdip, intact = run_dipole_grad(R, basis, fc.REF_ORIGIN)
    assert rc == 0 and intact and not np.isnan(ipdip).any()
    dg = fc.scaled_diff(ipdip[0], refs[f"{name}/ipdip"])
    print(name, "dip %.1e ipdip %.1e" % (d, dg))
    assert d < fc.DEVICE_HOST_GATE and dg < fc.DEVICE_HOST_GATE
    assert np.array_equal(dip[0], dip[0].transpose(0, 2, 1))


@pytest.fixture(scope="module")
def truth():
    return fc.load_truth()


@pytest.mark.parametrize("flags", FORMS, ids=lambda f: f"flags{f}")
@pytest.mark.parametrize("case", fc.TRUTH_CASES)
def test_truth_cases(truth, case, flags):
    """Every case of tests/golden/spdfgto_truth.npz within its gate (``spdfgto_cases.truth_gate``), per array."""
    basis = Basis(truth[f"{case}/Z"], fc.truth_shells(truth, case), renormalize=False)
    rc, arrays, intact, _ = run(truth[f"{case}/R"], basis, flags)
    assert rc == 0 and intact
    got = full_forms(arrays, basis.nao, flags)
    for k in (("enuc", "S", "hcore", "eri") if flags & ENERGY else fc.NAMES):
        e = fc.truth_err(got[k], truth, case, k)
        print("truth", case, flags, k, "%.1e" % e)
        assert e < fc.truth_gate(case, k), (case, k, e)
    rc, dip, intact, _ = run_dipole(truth[f"{case}/R"], basis, truth[f"{case}/origin"])
    e = fc.truth_err(dip[0], truth, case, "dip")
    print("truth", case, "dip", "%.1e" % e)
    assert rc == 0 and intact and e < fc.truth_gate(case, "dip"), e
    rc, ipdip, intact = run_dipole_grad(truth[f"{case}/R"], basis, truth[f"{case}/origin"])
    e = fc.truth_err(ipdip[0], truth, case, "ipdip")
    print("truth", case, "ipdip", "%.1e" % e)
    assert rc == 0 and intact and e < fc.truth_gate(case, "ipdip"), e


@pytest.fixture(scope="module")
def small():
    """(R, Basis, host molecule) of the N = 11 molecule: the host statement takes three seconds."""
    from evcont_amd.gto_spdf import spdf_gaussian_mol
    R, Z, shells = fc.small_f()
    return R, Basis(Z, shells), spdf_gaussian_mol(R, Z, shells)


@pytest.mark.parametrize("flags", [0, S4 | S2KL, ENERGY | S4], ids=lambda f: f"flags{f}")
def test_every_element_against_the_host_statement(small, flags):
    """All of eri and eri_ip1, not a sample."""
    R, basis, mol = small
    rc, arrays, intact, _ = run(R, basis, flags)
    assert rc == 0 and intact
    got = full_forms(arrays, basis.nao, flags)
    for k in (("enuc", "S", "hcore", "eri") if flags & ENERGY else fc.NAMES):
        d = fc.scaled_diff(got[k], getattr(mol, k))
        print("small_f", flags, k, "%.1e" % d)
        assert not np.isnan(got[k]).any() and d < fc.DEVICE_HOST_GATE, (k, d)


def test_bit_guarantees():
    """Run to run, geometry g of a batch against the call on it alone, packed against full, and the exact symmetries,
    on the two-centre molecule (Ms = 276: the kets span five blocks of 64, waves straddle the class boundaries)."""
    R0, Z, shells = fc.two_centre()
    basis = Basis(Z, shells)
    rng = np.random.default_rng(11)
    R = np.stack([R0 + 0.1 * rng.standard_normal(R0.shape) for _ in range(3)])
    rc, a, intact, _ = run(R, basis, 0)
    assert rc == 0 and intact
    rc, b, intact, _ = run(R, basis, 0)
    assert rc == 0 and intact
    for k in fc.NAMES:
        assert not np.isnan(a[k]).any() and np.array_equal(a[k], b[k]), k
    rc, one, intact, _ = run(R[1], basis, 0)
    assert rc == 0 and intact
    for k in fc.NAMES:
        assert np.array_equal(a[k][1:2], one[k]), k
    rc, p, intact, _ = run(R, basis, S4 | S2KL)
    assert rc == 0 and intact
    assert np.array_equal(p["eri"], pack_eri(a["eri"])) and np.array_equal(p["eri_ip1"], pack_ip1(a["eri_ip1"]))
    for k in ("enuc", "S", "hcore", "ipovlp", "dhcore", "gnuc"):
        assert np.array_equal(p[k], a[k]), k
    rc, e, intact, _ = run(R, basis, ENERGY)
    rc2, ep, intact2, _ = run(R, basis, ENERGY | S4)
    assert rc == 0 and rc2 == 0 and intact and intact2
    assert np.array_equal(ep["eri"], pack_eri(e["eri"]))
    # (an energy-only call runs other instantiations of the kernels, with Boys functions of another highest order: its
    # arrays equal those of the gradient call to rounding, which the comparisons with the host statement hold, not to
    # the bit; its own packed and full forms are the same bits)
    for k in ("enuc", "S", "hcore"):
        assert np.array_equal(ep[k], e[k]), k
        assert fc.scaled_diff(e[k], a[k]) < 1e-13, k
    assert np.array_equal(a["S"], a["S"].transpose(0, 2, 1)) and np.array_equal(a["hcore"], a["hcore"].transpose(0, 2, 1))
    assert np.array_equal(a["dhcore"], a["dhcore"].transpose(0, 1, 2, 4, 3))
    assert np.array_equal(a["eri"], a["eri"].transpose(0, 2, 1, 3, 4))
    assert np.array_equal(a["eri"], a["eri"].transpose(0, 1, 2, 4, 3))
    assert np.array_equal(a["eri_ip1"], a["eri_ip1"].transpose(0, 1, 2, 3, 5, 4))
    d0 = run_dipole(R, basis, fc.REF_ORIGIN)[1]
    assert np.array_equal(d0, run_dipole(R, basis, fc.REF_ORIGIN)[1])
    assert np.array_equal(d0[2:3], run_dipole(R[2], basis, fc.REF_ORIGIN)[1])
    g0 = run_dipole_grad(R, basis, fc.REF_ORIGIN)[1]
    assert np.array_equal(g0, run_dipole_grad(R, basis, fc.REF_ORIGIN)[1])
    assert np.array_equal(g0[2:3], run_dipole_grad(R[2], basis, fc.REF_ORIGIN)[1])


def test_spd_molecule_against_the_spd_kernels():
    """A molecule of s, p and d shells through ``evc_spdfgto_*`` against ``evc_spdgto_*``: the same arrays to rounding
    (``spdfgto_cases.SPD_GATE``; the class bodies sum in the order of the d route but stop at the orders of the class)."""
    import spdgto_cases as dc
    import spdgto_harness as dh
    R0, Z, shells = dc.two_centre()
    R = np.stack([R0, R0 + 0.05 * np.random.default_rng(2).standard_normal(R0.shape)])
    old, new = dh.Basis(Z, shells), Basis(Z, shells)
    assert np.array_equal(old.coefficients, new.coefficients)
    worst = 0.0
    for flags in (0, S4 | S2KL):
        rc0, a, ok0, _ = dh.run(R, old, flags)
        rc1, b, ok1, _ = run(R, new, flags)
        assert rc0 == 0 and rc1 == 0 and ok0 and ok1
        for k in fc.NAMES:
            d = fc.scaled_diff(b[k], a[k])
            print("spdf against spd", flags, k, "%.1e" % d)
            worst = max(worst, d)
    rc0, a, ok0, _ = dh.run_dipole(R, old, fc.REF_ORIGIN)
    rc1, b, ok1, _ = run_dipole(R, new, fc.REF_ORIGIN)
    assert rc0 == 0 and rc1 == 0 and ok0 and ok1
    worst = max(worst, fc.scaled_diff(b, a))
    print("spdf against spd, worst array: %.1e (gate %.1e)" % (worst, fc.SPD_GATE))
    assert worst < fc.SPD_GATE
