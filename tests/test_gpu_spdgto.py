"""GPU tests of the device AO integrals of s, p and real spherical d shells (csrc/spdgto.hip) through the C calls, on
NaN-poisoned fenced buffers (tests/spdgto_harness.py): against the independent truth file and against the host
statement ``gto_spd.spd_gaussian_mol`` in the full, s4 and s2kl forms with and without EVC_FLAG_ENERGY_ONLY, the bit guarantees (run to run, batch against single,
packed against full, the exact symmetries), and water / STO-3G against ``evc_spgto_*``.

Gate: ``spgto_cases.DEVICE_HOST_GATE`` (1e-10) under ``scaled_diff``, max |x - ref| / max(1, max |ref|) per array."""
import numpy as np
import pytest

import spdgto_cases as dc
from spdgto_harness import ENERGY, S2KL, S4, Basis, pack_eri, pack_ip1, run, run_dipole

pytestmark = pytest.mark.gpu

ORIGIN = (0.1, -0.2, 0.3)
MOLECULES = {"two_centre": dc.two_centre, "bent": dc.bent_three_centre}


@pytest.fixture(scope="module")
def host():
    """name -> (R, Basis, host molecule), the host statement computed once."""
    from evcont_amd.gto_spd import spd_gaussian_mol
    out = {}
    for name, make in MOLECULES.items():
        R, Z, shells = make()
        out[name] = (R, Basis(Z, shells), spd_gaussian_mol(R, Z, shells))
    return out


def full_forms(arrays, n, flags):
    out = {k: v[0] for k, v in arrays.items()}
    if flags & S4:
        out["eri"] = dc.unpack_eri(out["eri"], n)
    if flags & S2KL and "eri_ip1" in out:
        out["eri_ip1"] = dc.unpack_ip1(out["eri_ip1"], n)
    return out


@pytest.mark.parametrize("flags", [0, S4, S2KL, S4 | S2KL, ENERGY, ENERGY | S4], ids=lambda f: f"flags{f}")
@pytest.mark.parametrize("name", sorted(MOLECULES))
def test_device_against_the_host_statement(host, name, flags):
    R, basis, mol = host[name]
    rc, arrays, intact, _ = run(R, basis, flags)
    assert rc == 0 and intact
    got = full_forms(arrays, basis.nao, flags)
    names = ("enuc", "S", "hcore", "eri") if flags & ENERGY else dc.NAMES
    for k in names:
        assert not np.isnan(got[k]).any(), k
        d = dc.scaled_diff(got[k], getattr(mol, k))
        print(name, flags, k, "%.1e" % d)
        assert d < dc.DEVICE_HOST_GATE, (k, d)
    if flags & ENERGY:
        # the gradient arrays of an energy-only call stay untouched
        for k in ("ipovlp", "dhcore", "eri_ip1", "gnuc"):
            assert np.isnan(arrays[k]).all(), k


@pytest.fixture(scope="module")
def truth():
    return dc.load_truth()


@pytest.mark.parametrize("flags", [0, S4, S2KL, S4 | S2KL, ENERGY, ENERGY | S4], ids=lambda f: f"flags{f}")
@pytest.mark.parametrize("case", dc.TRUTH_CASES)
def test_truth_cases(truth, case, flags):
    """Every case of tests/golden/spdgto_truth.npz within its gate (``spdgto_cases.truth_gate``), per array."""
    basis = Basis(truth[f"{case}/Z"], dc.truth_shells(truth, case), renormalize=False)
    rc, arrays, intact, _ = run(truth[f"{case}/R"], basis, flags)
    assert rc == 0 and intact
    got = full_forms(arrays, basis.nao, flags)
    for k in (("enuc", "S", "hcore", "eri") if flags & ENERGY else dc.NAMES):
        e = dc.truth_err(got[k], truth, case, k)
        print("truth", case, flags, k, "%.1e" % e)
        assert e < dc.truth_gate(case, k), (case, k, e)
    rc, dip, intact, _ = run_dipole(truth[f"{case}/R"], basis, truth[f"{case}/origin"])
    e = dc.truth_err(dip[0], truth, case, "dip")
    assert rc == 0 and intact and e < dc.truth_gate(case, "dip"), e


@pytest.mark.parametrize("name", sorted(MOLECULES))
def test_dipole_against_the_host_statement(host, name):
    R, basis, mol = host[name]
    rc, dip, intact, _ = run_dipole(R, basis, ORIGIN)
    assert rc == 0 and intact and not np.isnan(dip).any()
    assert dc.scaled_diff(dip[0], mol.dipole_integrals(ORIGIN)) < dc.DEVICE_HOST_GATE
    assert np.array_equal(dip[0], dip[0].transpose(0, 2, 1))


def test_bit_guarantees(host):
    """Run to run, geometry g of a batch against the call on it alone, packed against full, and the exact symmetries,
    on the two-centre molecule (Ms = 171: the kets span three blocks of 64)."""
    R0, basis, _ = host["two_centre"]
    rng = np.random.default_rng(11)
    R = np.stack([R0 + 0.1 * rng.standard_normal(R0.shape) for _ in range(3)])
    rc, a, intact, _ = run(R, basis, 0)
    assert rc == 0 and intact
    rc, b, intact, _ = run(R, basis, 0)
    assert rc == 0 and intact
    for k in dc.NAMES:
        assert np.array_equal(a[k], b[k]), k
    rc, one, intact, _ = run(R[1], basis, 0)
    assert rc == 0 and intact
    for k in dc.NAMES:
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
    for k in ("enuc", "S"):                    # (hcore and eri use Boys functions of another highest order: rounding)
        assert np.array_equal(e[k], a[k]) and np.array_equal(ep[k], a[k]), k
    assert np.array_equal(ep["hcore"], e["hcore"])
    assert np.array_equal(a["S"], a["S"].transpose(0, 2, 1)) and np.array_equal(a["hcore"], a["hcore"].transpose(0, 2, 1))
    assert np.array_equal(a["dhcore"], a["dhcore"].transpose(0, 1, 2, 4, 3))
    assert np.array_equal(a["eri"], a["eri"].transpose(0, 2, 1, 3, 4))
    assert np.array_equal(a["eri"], a["eri"].transpose(0, 1, 2, 4, 3))
    assert np.array_equal(a["eri_ip1"], a["eri_ip1"].transpose(0, 1, 2, 3, 5, 4))
    d0 = run_dipole(R, basis, ORIGIN)[1]
    assert np.array_equal(d0, run_dipole(R, basis, ORIGIN)[1])
    assert np.array_equal(d0[2:3], run_dipole(R[2], basis, ORIGIN)[1])


def test_water_sto3g_against_the_sp_kernels():
    """A molecule of s and p shells through ``evc_spdgto_*`` against ``evc_spgto_*``: the same arrays to rounding."""
    import spgto_harness as sp
    from evcont_amd import gto_small as gs
    from evcont_amd import gto_spd as gd
    m = gs.water("sto-3g", need_grad=False)
    R = np.stack([m.coords, m.coords + 0.05 * np.random.default_rng(2).standard_normal((3, 3))])
    old = sp.Basis(m.charges, m.shells)
    new = Basis(m.charges, [[gd.Shell(s.l, s.exponents, s.coefficients) for s in atom] for atom in m.shells])
    assert np.array_equal(old.coefficients, new.coefficients)
    for flags in (0, S4 | S2KL):
        rc0, a, ok0, _ = sp.run(R, old, flags)
        rc1, b, ok1, _ = run(R, new, flags)
        assert rc0 == 0 and rc1 == 0 and ok0 and ok1
        for k in dc.NAMES:
            assert dc.scaled_diff(b[k], a[k]) < dc.DEVICE_HOST_GATE, k
    assert dc.scaled_diff(run_dipole(R, new, ORIGIN)[1], sp.run_dipole(R, old, ORIGIN)[1]) < dc.DEVICE_HOST_GATE
