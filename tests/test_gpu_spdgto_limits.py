"""GPU tests of csrc/spdgto.hip at the limits of the call, through NaN-poisoned, fenced output buffers and workspace
(tests/spdgto_harness.py): N = 64 with 128 primitives, a d shell of eight primitives, nuclei without functions, and the
forms per flag.

The oracle of the limit shape is the device itself on sub-molecules (as in tests/test_gpu_spgto_limits.py): no sum is
split between threads and every thread walks its primitives and monomials in one fixed order, so a block of the large
call has the BITS of the call on its atoms alone (S, ipovlp, eri, eri_ip1, dipole) or of the call that keeps the other
nuclei without functions (hcore, dhcore, enuc, gnuc).  Two pairs of centres of the limit shape, and the molecule with a d
shell of eight primitives, are held to the HOST statement through recorded arrays (tests/golden/spdgto_host_refs.npz,
written by make_spdgto_host_refs.py: the numpy statement takes half a minute to minutes on them).  The recorded pairs
hold S, hcore, eri and enuc: the derivative arrays of 8-primitive s and p shells beside d shells are reached through the
bit-equality with the sub-molecule calls alone.  Gate:
``spgto_cases.DEVICE_HOST_GATE``."""
import numpy as np
import pytest

import spdgto_cases as dc
from evcont_amd.gto_spd import spd_gaussian_mol
from spdgto_harness import ENERGY, S2KL, S4, Basis, run, run_dipole

pytestmark = pytest.mark.gpu

ORIGIN = (0.3, 0.1, -0.2)
PACKED = S4 | S2KL


@pytest.fixture(scope="module")
def limit():
    R, Z, shells = dc.limit_molecule()
    basis = Basis(Z, shells)
    assert (basis.nao, basis.nprim, basis.nshell) == (64, 128, 22) and basis.shell_prim_offset[-2] == 120
    rc, arrays, intact, bufs = run(R, basis, PACKED)
    assert rc == 0 and intact
    return R, Z, shells, basis, arrays


def blocks(basis, atoms):
    return np.concatenate([np.arange(*basis.aoslices[a]) for a in atoms])


def test_limit_every_element_written(limit):
    arrays = limit[4]
    for k, v in arrays.items():
        assert not np.isnan(v).any(), k


@pytest.mark.parametrize("atoms", dc.LIMIT_PAIRS, ids=str)
def test_limit_blocks_have_the_bits_of_the_sub_molecule(limit, atoms):
    R, Z, shells, basis, big = limit
    idx = blocks(basis, atoms)
    n = len(idx)
    iu, ju = np.tril_indices(64)
    pair_of = {(i, j): t for t, (i, j) in enumerate(zip(iu, ju))}
    su, tu = np.tril_indices(n)
    cols = np.array([pair_of[idx[i], idx[j]] for i, j in zip(su, tu)])
    # the call on the atoms alone
    sub = Basis(Z[list(atoms)], [shells[a] for a in atoms])
    rc, small, intact, _ = run(R[list(atoms)], sub, PACKED)
    assert rc == 0 and intact
    assert np.array_equal(small["S"][0], big["S"][0][np.ix_(idx, idx)])
    assert np.array_equal(small["ipovlp"][0], big["ipovlp"][0][:, idx][:, :, idx])
    assert np.array_equal(small["eri"][0], big["eri"][0][np.ix_(cols, cols)])
    assert np.array_equal(small["eri_ip1"][0], big["eri_ip1"][0][:, idx][:, :, idx][..., cols])
    dsmall = run_dipole(R[list(atoms)], sub, ORIGIN)[1]
    rc, dbig, intact, _ = run_dipole(R, basis, ORIGIN)
    assert rc == 0 and intact and not np.isnan(dbig).any()
    assert np.array_equal(dsmall[0], dbig[0][:, idx][:, :, idx])
    # the call that keeps the other nuclei, without functions
    bare = Basis(Z, [shells[a] if a in atoms else [] for a in range(8)])
    rc, kept, intact, _ = run(R, bare, PACKED)
    assert rc == 0 and intact
    assert np.array_equal(kept["hcore"][0], big["hcore"][0][np.ix_(idx, idx)])
    assert np.array_equal(kept["dhcore"][0], big["dhcore"][0][:, :, idx][:, :, :, idx])
    assert np.array_equal(kept["enuc"], big["enuc"]) and np.array_equal(kept["gnuc"], big["gnuc"])
    # and the host statement on that molecule (recorded: tests/golden/make_spdgto_host_refs.py): S, hcore, eri, enuc
    tag = "pair" + "_".join(str(a) for a in atoms)
    with np.load(dc.HOST_REFS) as ref:
        assert dc.scaled_diff(kept["S"][0], ref[f"{tag}/S"]) < dc.DEVICE_HOST_GATE
        assert dc.scaled_diff(kept["hcore"][0], ref[f"{tag}/hcore"]) < dc.DEVICE_HOST_GATE
        assert dc.scaled_diff(dc.unpack_eri(kept["eri"][0], n), ref[f"{tag}/eri"]) < dc.DEVICE_HOST_GATE
        assert abs(kept["enuc"][0] - float(ref[f"{tag}/enuc"])) < dc.DEVICE_HOST_GATE * abs(float(ref[f"{tag}/enuc"]))


def test_d_shell_of_eight_primitives():
    """A contracted d shell of eight primitives beside an s function against the host statement, all eight arrays and
    the dipole integrals (the host statement takes minutes on it: recorded by tests/golden/make_spdgto_host_refs.py)."""
    R, Z, shells = dc.eight_primitive_d()
    basis = Basis(Z, shells)
    rc, arrays, intact, _ = run(R, basis, 0)
    assert rc == 0 and intact
    with np.load(dc.HOST_REFS) as ref:
        for k in dc.NAMES:
            assert not np.isnan(arrays[k]).any(), k
            d = dc.scaled_diff(arrays[k][0], ref[f"d8/{k}"])
            print("d8", k, "%.1e" % d)
            assert d < dc.DEVICE_HOST_GATE, (k, d)
        rc, dip, intact, _ = run_dipole(R, basis, ref["origin"])
        assert rc == 0 and intact and dc.scaled_diff(dip[0], ref["d8/dip"]) < dc.DEVICE_HOST_GATE
    assert np.abs(arrays["S"][0][:5, :5] - np.eye(5)).max() < 1e-13


def test_nucleus_without_functions_in_the_middle_and_last():
    R0, Z0, sh0 = dc.small_bent()
    R = np.vstack([R0[:1], [[0.8, 0.8, 0.8]], R0[1:], [[-0.5, 1.9, 0.2]]])
    Z = np.array([Z0[0], 1.0, Z0[1], Z0[2], 2.0])
    shells = [sh0[0], [], sh0[1], sh0[2], []]
    mol = spd_gaussian_mol(R, Z, shells)
    basis = Basis(Z, shells)
    rc, arrays, intact, _ = run(R, basis, 0)
    assert rc == 0 and intact
    for k in dc.NAMES:
        assert not np.isnan(arrays[k]).any(), k
        d = dc.scaled_diff(arrays[k][0], getattr(mol, k))
        assert d < dc.DEVICE_HOST_GATE, (k, d)
    rc, dip, intact, _ = run_dipole(R, basis, ORIGIN)
    assert rc == 0 and intact and dc.scaled_diff(dip[0], mol.dipole_integrals(ORIGIN)) < dc.DEVICE_HOST_GATE


@pytest.mark.parametrize("flags", [S4, S2KL, ENERGY, ENERGY | S4 | S2KL], ids=lambda f: f"flags{f}")
def test_flags_one_by_one(flags):
    """Each packed array is the packing of the full one, arrays a flag does not concern keep their bits, and null
    gradient pointers are accepted under EVC_FLAG_ENERGY_ONLY."""
    from spdgto_harness import pack_eri, pack_ip1
    R0, Z, shells = dc.small_bent()
    R = np.stack([R0, R0 * 1.03])
    basis = Basis(Z, shells)
    base = ENERGY if flags & ENERGY else 0
    rc, full, intact, _ = run(R, basis, base)
    assert rc == 0 and intact
    rc, got, intact, _ = run(R, basis, flags, null_grad=bool(flags & ENERGY))
    assert rc == 0 and intact
    assert np.array_equal(got["eri"], pack_eri(full["eri"]) if flags & S4 else full["eri"])
    for k in ("enuc", "S", "hcore"):
        assert np.array_equal(got[k], full[k]), k
    if flags & ENERGY:
        assert set(got) == {"enuc", "S", "hcore", "eri"}
        for k in ("ipovlp", "dhcore", "eri_ip1", "gnuc"):
            assert np.isnan(full[k]).all(), k                   # untouched by the energy-only call with buffers
    else:
        assert np.array_equal(got["eri_ip1"], pack_ip1(full["eri_ip1"]) if flags & S2KL else full["eri_ip1"])
        for k in ("ipovlp", "dhcore", "gnuc"):
            assert np.array_equal(got[k], full[k]), k
