"""GPU tests of the device route from coordinates to forces for molecules with d shells
(``gto_spd_device.DeviceSpdGaussians``, ``MD_utils.state_swarm(..., integrals="device")``):

* the cc-pVDZ table of ``gto_spd`` through the RHF energy of water at a fixed geometry,
* water in STO-3G plus the cc-pVDZ d shell on O (N = 12) with three CAS training states: energies and forces on
  device-made integrals against the same evaluator on uploaded host-statement arrays (1e-10 Ha, 1e-9 Ha / Bohr), forces
  against a central difference of the device energy (h = 2e-4, 2e-7: tests/test_hchain_physics.py), and a 3-step swarm
  with observables against the host route,
* the same on water / cc-pVDZ (N = 24, the default kernels), training states through ``to_mol``.

The host statement takes about ten seconds per geometry with derivatives at N = 12, so it is computed for ONE geometry
(module fixture); the swarm's host route rebuilds its molecules through ``DeviceMadeMol.with_coords``, i.e. it evaluates
downloaded device-made arrays on the host path against the device path that never downloads them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda"
E_RHF_CCPVDZ = -76.0267656731     # RHF / cc-pVDZ, O (0,0,0), H (0, -/+0.757, 0.587) Angstrom


def small_d_water():
    """(charges, shells) of water in STO-3G plus the cc-pVDZ d shell on O: N = 12."""
    from evcont_amd import gto_spd as gd
    charges, shells = gd.water_shells("sto-3g")
    shells[0] = shells[0] + [gd.Shell(*gd.CCPVDZ["O"][-1])]
    assert shells[0][-1].l == 2
    return charges, shells


def geometry(r, ang, seed=None, amp=0.05):
    from evcont_amd.gto_spd import water_coords
    R = water_coords(r, ang)
    return R if seed is None else R + amp * np.random.default_rng(seed).standard_normal((3, 3))


def train(dg, geometries=((1.6, 100.0), (1.85, 106.0), (2.2, 112.0))):
    from evcont_amd.CASCI_EVCont import CAS_EVCont_obj
    from evcont_amd.fci_small import SmallFCI
    cont = CAS_EVCont_obj(4, 2, cisolver=SmallFCI())
    for r, ang in geometries:
        cont.append_to_rdms(dg.to_mol(geometry(r, ang), need_grad=False))
    return cont.overlap, cont.one_rdm, cont.two_rdm


@pytest.fixture(scope="module")
def small():
    from evcont_amd.gto_spd_device import DeviceSpdGaussians
    charges, shells = small_d_water()
    dg = DeviceSpdGaussians(charges, shells, device=DEV)
    assert dg.nao == 12
    return dg, train(dg)


@pytest.fixture(scope="module")
def host_mol(small):
    """The host statement at one shaken geometry, computed once."""
    from evcont_amd.gto_spd import spd_gaussian_mol
    dg = small[0]
    return spd_gaussian_mol(geometry(1.8088, 104.5, seed=1), dg._charges_host, dg.shells, nelec=(5, 5))


def test_ccpvdz_table_through_the_rhf_energy():
    """Check of the table: RHF of water / cc-pVDZ on integrals from ``to_mol`` against the known energy, 1e-6 Ha."""
    from evcont_amd import gto_spd as gd
    from evcont_amd.gto_spd_device import DeviceSpdGaussians
    from evcont_amd.scf_small import rhf
    dg = DeviceSpdGaussians(*gd.water_shells("cc-pvdz"), device=DEV)
    assert dg.nao == 24 and dg.exponents.shape[0] == 32 and dg.shell_l.shape[0] == 12
    R = np.array([[0.0, 0.0, 0.0], [0.0, -0.757, 0.587], [0.0, 0.757, 0.587]]) * gd.ANGSTROM
    m = dg.to_mol(R, need_grad=False)
    assert np.abs(np.diag(m.S) - 1.0).max() < 1e-12
    C, _, converged = rhf(m.S, m.hcore, m.eri, m.nelec)
    assert converged
    D = 2.0 * C[:, :5] @ C[:, :5].T
    V = np.einsum("pqrs,rs->pq", m.eri, D) - 0.5 * np.einsum("prqs,rs->pq", m.eri, D)
    E = float(np.sum(D * (m.hcore + 0.5 * V))) + m.enuc
    print("RHF / cc-pVDZ energy of water: %.10f (known %.10f, difference %.2e)" % (E, E_RHF_CCPVDZ, E - E_RHF_CCPVDZ))
    assert abs(E - E_RHF_CCPVDZ) < 1e-6


def central_difference(surfaces_for, R0, h=2e-4):
    """(E0 (nroots,), grads (nroots,3,3), fd (nroots,3,3)) from one call on R0 and its 18 displaced copies."""
    disp = np.repeat(R0[None], 19, axis=0)
    for k in range(9):
        disp[1 + 2 * k].reshape(-1)[k] += h
        disp[2 + 2 * k].reshape(-1)[k] -= h
    E, grads = surfaces_for(19)(disp)
    E, grads = np.array(E), np.array(grads)
    fd = ((E[1::2] - E[2::2]) / (2 * h)).T.reshape(E.shape[1], 3, 3)
    return E[0], grads[0], fd


@pytest.mark.parametrize("packed", [True, False])
def test_energies_and_forces_match_uploaded_host_integrals(small, host_mol, packed):
    from evcont_amd.evaluator import BatchedEvaluator, DeviceAOBatch, DeviceTRDMs
    dg, (S, one, two) = small
    mol, R = host_mol, host_mol.atom_coords()
    trd = DeviceTRDMs(one, two, S, DEV, compress="sym8" if packed else None)
    ev = BatchedEvaluator(trd, 3, 1)
    pairs = [(0, 0), (1, 1)]
    ref = DeviceAOBatch.from_arrays([mol], DEV, pack_ip1=packed, pack_eri=packed)
    E0, _, g0 = ev.multistate_energies_with_grads(ref, 2, pairs)
    E0, g0 = np.array(E0), np.array(g0)
    aob = dg.integrals(R, packed=packed)
    assert aob.eri.shape == ref.eri.shape and aob.eri_ip1.shape == ref.eri_ip1.shape
    E1, _, g1 = ev.multistate_energies_with_grads(aob, 2, pairs)
    print("max |dE| =", np.abs(E1 - E0).max(), " max |dgrad| =", np.abs(g1 - g0).max())
    assert np.abs(E1 - E0).max() < 1e-10
    assert np.abs(g1 - g0).max() < 1e-9
    ev19 = BatchedEvaluator(trd, 3, 19)

    def surfaces_for(G):
        return lambda Rs: ev19.multistate_energies_with_grads(dg.integrals(Rs, packed=packed), 2, pairs)[::2]

    _, g, fd = central_difference(surfaces_for, R)
    print("max |grad - fd| =", np.abs(g - fd).max())
    assert np.abs(g - fd).max() < 2e-7
    assert np.abs(g - g1[0]).max() < 1e-10


def test_swarm_and_observables_follow_the_host_route(small):
    from evcont_amd.MD_utils import state_swarm
    from evcont_amd.gto_spd_device import DeviceSpdGaussians
    dg, (S, one, two) = small
    mols = [dg.to_mol(geometry(1.8088, 104.5, seed=s)) for s in (5, 6)]
    assert DeviceSpdGaussians.from_mol(mols[0]).nao == 12
    v0 = 1e-4 * np.random.default_rng(9).standard_normal((2, 3, 3))
    obs = ("dipole", "mulliken", "loewdin")
    host = state_swarm(mols, one, two, S, root=1, dt=4.0, steps=3, init_veloc=v0, observables=obs)
    dev = state_swarm(mols, one, two, S, root=1, dt=4.0, steps=3, init_veloc=v0, integrals="device", observables=obs)
    assert len(dev) == len(host) == 3
    for fh, fd in zip(host, dev):
        assert set(fd) == set(fh) and fd["time"] == fh["time"]
        assert np.abs(fd["coord"] - fh["coord"]).max() < 1e-10
        assert np.abs(fd["epot"] - fh["epot"]).max() < 1e-10
        np.testing.assert_allclose(fd["veloc"], fh["veloc"], rtol=0, atol=1e-12)
        for k in ("dipole", "mulliken_charges", "loewdin_charges"):
            assert np.abs(fd[k] - fh[k]).max() < 1e-10, k


def test_swarm_on_water_ccpvdz():
    """N = 24: the swarm goes to ``DeviceSpdGaussians`` and through the default kernels; finite energies, and the forces
    of the surface the swarm uses agree with a central difference of its energy."""
    from evcont_amd import MD_utils
    from evcont_amd import gto_spd as gd
    from evcont_amd.gto_spd_device import DeviceSpdGaussians
    dg = DeviceSpdGaussians(*gd.water_shells("cc-pvdz"), nelec=(5, 5), device=DEV)
    # a narrow range: over a wide one the third and fourth virtual orbital of cc-pVDZ cross, and the CAS pair reduction
    # refuses states whose active spaces have swapped character
    S, one, two = train(dg, ((1.75, 103.0), (1.8088, 104.5), (1.87, 106.0)))
    assert one.shape[-1] == 24
    mol = dg.to_mol(geometry(1.8088, 104.5, seed=3))
    frames = MD_utils.state_swarm([mol], one, two, S, root=0, dt=4.0, steps=3, integrals="device")
    assert len(frames) == 3 and all(np.all(np.isfinite(f["epot"])) and np.all(np.isfinite(f["coord"])) for f in frames)

    def surfaces_for(G):
        return MD_utils._device_surfaces([mol] * G, one, two, S, 1)

    E, g, fd = central_difference(surfaces_for, mol.atom_coords())
    print("E =", E, " max |grad - fd| =", np.abs(g - fd).max())
    assert np.isfinite(E).all() and E[0] < -75.0
    assert np.abs(g - fd).max() < 2e-7
