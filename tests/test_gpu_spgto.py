"""GPU tests of the device AO integrals of s and p Gaussian shells (``gto_device.DeviceGaussians``, csrc/spgto.hip):
against the independent truth file and against the host statement on the cases of tests/spgto_cases.py and on STO-3G
water, in the full and packed forms, with and without the gradient arrays; the bit-level properties the header states;
no allocation on a second call of a shape."""
import numpy as np
import pytest
import torch

import spgto_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def truth():
    return sc.load_truth()


@pytest.fixture(scope="module")
def molecules(truth):
    """name -> the host statement at the case's geometry (computed once, never changed)."""
    from evcont_amd import gto_small
    mols = {name: sc.case_mol(truth, name) for name in sc.CASES}
    mols["water"] = gto_small.water("sto-3g")
    return mols


def to_numpy(aob, n):
    """The arrays of a DeviceAOBatch on the host, geometry first, in the full forms."""
    out = {k: getattr(aob, k).cpu().numpy() for k in sc.NAMES if getattr(aob, k) is not None}
    if aob.eri_s4:
        out["eri"] = np.stack([sc.unpack_eri(e, n) for e in out["eri"]])
    if aob.ip1_s2kl:
        out["eri_ip1"] = np.stack([sc.unpack_ip1(p, n) for p in out["eri_ip1"]])
    return out


@pytest.mark.parametrize("name", sc.CASES + ("water",))
def test_device_against_truth_and_host(truth, molecules, name):
    """Measured on MI355X (max error relative to max(1, max |array|), all forms): against the truth 1.1e-14 (dhcore of
    case "c"), every other array of every case at most 7.6e-16 (dhcore of "b"), at the crossover cases "e_lo" / "e_hi" at
    most 3.5e-16; against the host statement 2.1e-12 (the host's own error in dhcore of "c").  Gate against the truth: per
    case and array, ``spgto_cases.truth_gate``."""
    from evcont_amd.gto_device import DeviceGaussians
    mol = molecules[name]
    dg = DeviceGaussians.from_mol(mol, device=DEV)
    worst_truth, worst_host = {}, 0.0
    for need_grad in (True, False):
        for packed in (False, True):
            aob = dg.integrals(mol.atom_coords(), need_grad=need_grad, packed=packed)
            assert aob.natm == mol.natm and np.array_equal(aob.aoslices.cpu().numpy(), mol.aoslices)
            assert aob.eri_s4 == packed and aob.ip1_s2kl == (packed and need_grad)
            got = to_numpy(aob, mol.nao)
            assert set(got) == set(sc.NAMES if need_grad else ("enuc", "S", "hcore", "eri"))
            for f, x in got.items():
                assert x.shape[1:] == np.shape(getattr(mol, f)), f
                worst_host = max(worst_host, sc.scaled_diff(x[0], getattr(mol, f)))
                if name != "water":
                    worst_truth[f] = max(worst_truth.get(f, 0.0), sc.rel_err(x[0], truth, name, f))
    origin = truth[f"{name}/origin"] if name != "water" else (0.1, -0.2, 0.3)
    dip = dg.dipole_integrals(mol.atom_coords(), origin).cpu().numpy()[0]
    worst_host = max(worst_host, sc.scaled_diff(dip, mol.dipole_integrals(origin)))
    if name != "water":
        worst_truth["dip"] = sc.rel_err(dip, truth, name, "dip")
    print(f"{name}: device against truth " + ", ".join(f"{f} {v:.1e}" for f, v in worst_truth.items())
          + f"; against the host statement {worst_host:.1e}")
    over = {f: (v, sc.truth_gate(name, f)) for f, v in worst_truth.items() if not v < sc.truth_gate(name, f)}
    assert not over, over
    assert worst_host < sc.DEVICE_HOST_GATE


@pytest.mark.parametrize("name", ["a", "water"])
def test_bits(molecules, name):
    """G = 3 equals three calls of G = 1, two runs are equal, the full forms are the unpacked packed forms, and the
    symmetries hold exactly."""
    from evcont_amd.gto_device import DeviceGaussians
    mol = molecules[name]
    n = mol.nao
    dg = DeviceGaussians.from_mol(mol, device=DEV)
    rng = np.random.default_rng(12)
    R = mol.atom_coords()[None] + 0.1 * rng.standard_normal((3,) + mol.atom_coords().shape)
    keep = lambda aob: {k: getattr(aob, k).clone() for k in sc.NAMES if getattr(aob, k) is not None}
    for packed in (False, True):
        batch = keep(dg.integrals(R, packed=packed))
        again = keep(dg.integrals(R, packed=packed))
        for k in batch:
            assert torch.equal(batch[k], again[k]), (k, "two runs")
        for g in range(3):
            one = keep(dg.integrals(R[g], packed=packed))
            for k in batch:
                assert torch.equal(batch[k][g], one[k][0]), (k, g, "batch against the call on the geometry alone")
        if not packed:
            full = {k: v.cpu().numpy() for k, v in batch.items()}
        else:
            for g in range(3):
                assert np.array_equal(sc.unpack_eri(batch["eri"][g].cpu().numpy(), n), full["eri"][g])
                assert np.array_equal(sc.unpack_ip1(batch["eri_ip1"][g].cpu().numpy(), n), full["eri_ip1"][g])
            for k in ("enuc", "S", "hcore", "ipovlp", "dhcore", "gnuc"):
                assert np.array_equal(batch[k].cpu().numpy(), full[k]), k
    assert np.array_equal(full["S"], full["S"].transpose(0, 2, 1))
    assert np.array_equal(full["hcore"], full["hcore"].transpose(0, 2, 1))
    assert np.array_equal(full["dhcore"], full["dhcore"].transpose(0, 1, 2, 4, 3))
    assert np.array_equal(full["eri"], full["eri"].transpose(0, 2, 1, 3, 4))
    assert np.array_equal(full["eri"], full["eri"].transpose(0, 1, 2, 4, 3))
    assert np.array_equal(full["eri_ip1"], full["eri_ip1"].transpose(0, 1, 2, 3, 5, 4))
    d1 = dg.dipole_integrals(R).clone()
    assert torch.equal(d1, dg.dipole_integrals(R)) and torch.equal(d1, d1.transpose(2, 3))
    assert torch.equal(d1[1], dg.dipole_integrals(R[1])[0])
    # energy-only: eri agrees with the gradient instantiation to rounding (other Boys orders), S and hcore bit for bit
    e_only = dg.integrals(R, need_grad=False)
    assert e_only.eri_ip1 is None and e_only.dhcore is None
    assert np.array_equal(e_only.S.cpu().numpy(), full["S"]) and np.array_equal(e_only.hcore.cpu().numpy(), full["hcore"])
    assert sc.scaled_diff(e_only.eri.cpu().numpy(), full["eri"]) < sc.TRUTH_GATE


def test_second_call_allocates_nothing_and_wrong_shapes_raise(molecules):
    from evcont_amd.gto_device import DeviceGaussians
    mol = molecules["water"]
    dg = DeviceGaussians.from_mol(mol, device=DEV)
    R = np.stack([mol.atom_coords(), mol.atom_coords() + 0.02])
    for packed in (True, False):
        first = dg.integrals(R, packed=packed)
        dg.dipole_integrals(R)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        second = dg.integrals(R + 0.01, packed=packed)
        dg.dipole_integrals(R + 0.01)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        assert second.eri.data_ptr() == first.eri.data_ptr() and second.eri_ip1.data_ptr() == first.eri_ip1.data_ptr()
    assert torch.equal(dg.staged_coords(2).cpu(), torch.from_numpy(R + 0.01))
    assert torch.equal(dg.charges.cpu(), torch.tensor([8.0, 1.0, 1.0], dtype=torch.float64))
    with pytest.raises(ValueError):
        dg.integrals(np.zeros((2, 4, 3)))
    with pytest.raises(ValueError):
        dg.integrals(torch.zeros((2, 3), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        dg.dipole_integrals(np.zeros((2, 3, 2)))
