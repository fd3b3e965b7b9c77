"""GPU tests of the device route from coordinates to forces for water in STO-3G (``gto_device.DeviceGaussians``,
``MD_utils.state_swarm(..., integrals="device")``) with three FCI training states: the batched evaluator on device-made
integrals against the same evaluator on uploaded host-statement integrals at the project's parity thresholds (1e-10 Ha,
1e-9 Ha / Bohr), the forces against a central difference of the device energy, the swarm against the host route and
its observables against ``evcont_amd.properties`` on host integrals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROH = 1.8088               # Bohr


@pytest.fixture(scope="module")
def training():
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    from evcont_amd.fci_small import SmallFCI
    from evcont_amd.gto_small import water
    cont = FCI_EVCont_obj(cisolver=SmallFCI(), cibasis="OAO")
    for r, ang in ((1.6, 100.0), (1.85, 106.0), (2.2, 112.0)):
        cont.append_to_rdms(water("sto-3g", r, ang, need_grad=False))
    return cont.overlap, cont.one_rdm, cont.two_rdm


def shaken(seed, amp=0.05):
    from evcont_amd.gto_small import water
    m = water("sto-3g", ROH, 104.5)
    return m.with_coords(m.atom_coords() + amp * np.random.default_rng(seed).standard_normal((3, 3)))


@pytest.mark.parametrize("packed", [True, False])
def test_energies_and_forces_match_uploaded_host_integrals(training, packed):
    from evcont_amd.evaluator import BatchedEvaluator, DeviceAOBatch, DeviceTRDMs
    from evcont_amd.gto_device import DeviceGaussians
    S, one, two = training
    mols = [shaken(s) for s in (1, 2, 3)]
    R = np.stack([m.atom_coords() for m in mols])
    trd = DeviceTRDMs(one, two, S, DEV, compress="sym8" if packed else None)
    ev = BatchedEvaluator(trd, 3, 3)
    pairs = [(0, 0), (1, 1)]
    host = DeviceAOBatch.from_arrays(mols, DEV, pack_ip1=packed, pack_eri=packed)
    E0, _, g0 = ev.multistate_energies_with_grads(host, 2, pairs)
    E0, g0 = np.array(E0), np.array(g0)
    dg = DeviceGaussians.from_mol(mols[0], device=DEV)
    aob = dg.integrals(R, packed=packed)
    assert aob.eri.shape == host.eri.shape and aob.eri_ip1.shape == host.eri_ip1.shape
    assert np.array_equal(aob.aoslices.cpu().numpy(), host.aoslices.cpu().numpy())
    E1, _, g1 = ev.multistate_energies_with_grads(aob, 2, pairs)
    print("max |dE| =", np.abs(E1 - E0).max(), " max |dgrad| =", np.abs(g1 - g0).max())
    assert np.abs(E1 - E0).max() < 1e-10
    assert np.abs(g1 - g0).max() < 1e-9
    # the forces of both roots against a central difference of the device energy (step and tolerance of the
    # continuation-gradient test of tests/test_hchain_physics.py)
    h = 2e-4
    disp = np.repeat(R[:1], 18, axis=0)
    for k in range(9):
        disp[2 * k].reshape(-1)[k] += h
        disp[2 * k + 1].reshape(-1)[k] -= h
    ev18 = BatchedEvaluator(trd, 3, 18)
    Ed = np.array(ev18.multistate_energies_with_grads(dg.integrals(disp, packed=packed), 2, pairs)[0])
    fd = ((Ed[0::2] - Ed[1::2]) / (2 * h)).T.reshape(2, 3, 3)
    print("max |grad - fd| =", np.abs(g1[0] - fd).max())
    assert np.abs(g1[0] - fd).max() < 2e-7


def test_swarm_and_observables_follow_the_host_route(training):
    from evcont_amd import properties as pr
    from evcont_amd.MD_utils import state_swarm
    from oracle import evcont_oracle as orc
    S, one, two = training
    mols = [shaken(5), shaken(6)]
    v0 = 1e-4 * np.random.default_rng(9).standard_normal((2, 3, 3))
    host = state_swarm(mols, one, two, S, root=1, dt=4.0, steps=3, init_veloc=v0)
    dev = state_swarm(mols, one, two, S, root=1, dt=4.0, steps=3, init_veloc=v0, integrals="device")
    assert len(dev) == len(host) == 3
    for fh, fd in zip(host, dev):
        assert set(fd) == set(fh) and fd["time"] == fh["time"]
        print("step", fh["time"], "max |dR| =", np.abs(fd["coord"] - fh["coord"]).max(),
              " max |dE| =", np.abs(fd["epot"] - fh["epot"]).max())
        assert np.abs(fd["coord"] - fh["coord"]).max() < 1e-10
        assert np.abs(fd["epot"] - fh["epot"]).max() < 1e-10
        np.testing.assert_allclose(fd["veloc"], fh["veloc"], rtol=0, atol=1e-12)
    frames = state_swarm(mols, one, two, S, root=1, dt=4.0, steps=3, init_veloc=v0, integrals="device",
                         observables=("dipole", "mulliken", "loewdin"))
    worst = 0.0
    for f, f0 in zip(frames, dev):
        assert set(f) == set(f0) | {"dipole", "mulliken_charges", "loewdin_charges"}
        assert np.abs(f["coord"] - f0["coord"]).max() < 1e-10 and np.abs(f["epot"] - f0["epot"]).max() < 1e-10
        for g, R in enumerate(f["coord"]):
            mol = mols[0].with_coords(R, need_grad=False)
            b = orc.AOBundle(mol.S, mol.hcore, mol.eri, mol.ipovlp, mol.dhcore, mol.eri_ip1, mol.aoslices, mol.enuc,
                             mol.gnuc)
            _, Cr = orc.approximate_multistate_OAO(b, one, two, S, 2)
            ref = pr.properties_host(one, orc.loewdin_trafo(mol.S), Cr, [(1, 1)], mol.S, mol.dipole_integrals(),
                                     mol.aoslices, mol.charges, R)
            worst = max(worst, np.abs(f["dipole"][g] - ref["dipole"][0]).max(),
                        np.abs(f["mulliken_charges"][g] - (mol.charges - ref["mulliken"][0])).max(),
                        np.abs(f["loewdin_charges"][g] - (mol.charges - ref["loewdin"][0])).max())
    print("swarm observables: max deviation from the host recomputation = %.2e" % worst)
    assert worst < 1e-10


def test_other_molecules_are_still_refused(training):
    from evcont_amd.MD_utils import state_swarm
    from evcont_amd.synthetic import make_ao_arrays
    S, one, two = training

    class Bare:
        def __init__(self, ao):
            self.__dict__.update(ao.__dict__)

        def atom_coords(self):
            return np.zeros((3, 3))

        def atom_mass_list(self):
            return np.ones(3)

    with pytest.raises(ValueError, match="s-Gaussian molecules"):
        state_swarm([Bare(make_ao_arrays(7, 3, 1))], one, two, S, root=0, steps=1, integrals="device")
