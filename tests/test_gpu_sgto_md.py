"""GPU tests of the device route from coordinates to forces (``hchain_device.DeviceSGaussians``,
``MD_utils.state_swarm(..., integrals="device")``) on an H6 chain with three FCI training states: the batched evaluator
on device-made integrals against the same evaluator on uploaded ``s_gaussian_mol`` arrays at the project's parity
thresholds (1e-10 Ha, 1e-9 Ha / Bohr), the swarm and its NVE drift against the host route, and no allocation in a
steady loop."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def training():
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    from evcont_amd.fci_small import SmallFCI
    from evcont_amd.hchain import hydrogen_chain
    cont = FCI_EVCont_obj(cisolver=SmallFCI(), cibasis="OAO")
    for d in (1.5, 2.0, 2.6):
        cont.append_to_rdms(hydrogen_chain(6, d, need_grad=False))
    return cont.overlap, cont.one_rdm, cont.two_rdm


def bent(seed, d=1.9, amp=0.05):
    R = np.zeros((6, 3))
    R[:, 0] = d * np.arange(6)
    return R + amp * np.random.default_rng(seed).standard_normal((6, 3))


@pytest.mark.parametrize("packed", [True, False])
def test_energies_forces_and_couplings_match_uploaded_host_integrals(training, packed):
    from evcont_amd.evaluator import BatchedEvaluator, DeviceAOBatch, DeviceTRDMs
    from evcont_amd.hchain import s_gaussian_mol
    from evcont_amd.hchain_device import DeviceSGaussians
    S, one, two = training
    R = np.stack([bent(s) for s in (1, 2, 3)])
    trd = DeviceTRDMs(one, two, S, DEV, compress="sym8" if packed else None)
    ev = BatchedEvaluator(trd, 6, 3)
    pairs = [(0, 0), (1, 1), (0, 1)]
    host = DeviceAOBatch.from_arrays([s_gaussian_mol(r) for r in R], DEV, pack_ip1=packed, pack_eri=packed)
    E0, _, g0 = ev.multistate_energies_with_grads(host, 2, pairs)
    sg = DeviceSGaussians(device=DEV)
    aob = sg.integrals(R, packed=packed)
    assert aob.eri_s4 == packed and aob.ip1_s2kl == packed and aob.eri.shape == host.eri.shape
    assert torch.equal(aob.aoslices, host.aoslices)
    E1, _, g1 = ev.multistate_energies_with_grads(aob, 2, pairs)
    print("max |dE| =", np.abs(E1 - E0).max(), " max |dgrad| =", np.abs(np.abs(g1) - np.abs(g0)).max())
    assert np.abs(E1 - E0).max() < 1e-10
    assert np.abs(g1[:, :2] - g0[:, :2]).max() < 1e-9
    assert np.abs(np.abs(g1[:, 2]) - np.abs(g0[:, 2])).max() < 1e-9       # (a coupling's sign follows the eigenvectors)
    # a device tensor of coordinates and the energy-only form
    e_only = sg.integrals(torch.from_numpy(R).to(DEV), need_grad=False, packed=packed)
    assert e_only.eri_ip1 is None and torch.equal(e_only.eri, aob.eri) and torch.equal(e_only.hcore, aob.hcore)


def test_swarm_on_device_integrals_follows_the_host_route(training):
    from evcont_amd.MD_utils import state_swarm
    from evcont_amd.hchain import s_gaussian_mol
    S, one, two = training
    mols = [s_gaussian_mol(bent(s)) for s in (5, 6)]
    v0 = 1e-4 * np.random.default_rng(9).standard_normal((2, 6, 3))
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
    with pytest.raises(ValueError):
        state_swarm(mols, one, two, S, root=0, steps=1, integrals="gpu")


def test_nve_drift_and_one_trajectory_form(training):
    from evcont_amd.MD_utils import get_trajectory, state_swarm
    from evcont_amd.hchain import s_gaussian_mol
    S, one, two = training
    mol = s_gaussian_mol(bent(7))
    drift = {}
    for route in ("host", "device"):
        frames = state_swarm([mol], one, two, S, root=0, dt=2.0, steps=20, integrals=route)
        etot = np.array([f["epot"][0] + f["ekin"][0] for f in frames])
        drift[route] = float(np.abs(etot - etot[0]).max())
        if route == "device":
            coords = np.array([f["coord"][0] for f in frames])
    print("NVE drift over 20 steps:", drift)
    assert drift["device"] <= drift["host"] + 1e-9
    traj = get_trajectory(mol, S, one, two, dt=2.0, steps=20, integrals="device")
    np.testing.assert_allclose(traj, coords, rtol=0, atol=1e-12)


def test_second_call_of_a_shape_allocates_nothing():
    from evcont_amd.hchain_device import DeviceSGaussians
    sg = DeviceSGaussians(device=DEV)
    R = np.stack([bent(s) for s in (1, 2)])
    for packed in (True, False):
        first = sg.integrals(R, packed=packed)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        second = sg.integrals(R + 0.01, packed=packed)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        assert second.eri.data_ptr() == first.eri.data_ptr() and second.eri_ip1.data_ptr() == first.eri_ip1.data_ptr()
