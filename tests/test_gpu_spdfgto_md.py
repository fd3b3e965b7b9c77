"""GPU tests of the device route from coordinates to forces for molecules with f shells
(``gto_spdf_device.DeviceSpdfGaussians``, ``MD_utils.state_swarm(..., integrals="device")``):

* the producer's dipole integrals, their gradient and the fold of a uniform field against the host statement of the
  N = 11 molecule (three seconds on the host), and ``field=None`` enqueues nothing more,
* water in STO-3G plus one f shell on O (N = 14) with three CAS training states: energies and forces on device-made
  integrals against the same evaluator on the uploaded RECORDED host-statement arrays
  (tests/golden/spdfgto_water_refs.npz; 1e-10 Ha, 1e-9 Ha / Bohr), forces against a central difference of the device
  energy (h = 2e-4, 2e-7: tests/test_hchain_physics.py), and a two-step swarm against the host route,
* the N = 58 shape of water / cc-pVTZ (``spdfgto_cases.tz_shape_water``) through ``integrals(packed=True)`` and one
  batched evaluation; no host statement at this size."""
import numpy as np
import pytest

import spdfgto_cases as fc

pytestmark = pytest.mark.gpu

DEV = "cuda"
ORIGIN = (0.1, -0.2, 0.3)


@pytest.fixture(scope="module")
def small():
    from evcont_amd.gto_spdf import spdf_gaussian_mol
    from evcont_amd.gto_spdf_device import DeviceSpdfGaussians
    R, Z, shells = fc.small_f()
    return R, DeviceSpdfGaussians(Z, shells, device=DEV), spdf_gaussian_mol(R, Z, shells)


def test_producer_dipoles_and_field_against_the_host_statement(small):
    import torch
    from evcont_amd.gto_spd_device import DeviceSpdGaussians
    R, dg, mol = small
    assert dg.nao == 11
    with pytest.raises(ValueError, match="l=3"):
        DeviceSpdGaussians(dg._charges_host, dg.shells, device=DEV)
    dip = dg.dipole_integrals(R, ORIGIN)[0].cpu().numpy()
    ipdip = dg.dipole_grad_integrals(R, ORIGIN)[0].cpu().numpy()
    assert fc.scaled_diff(dip, mol.dipole_integrals(ORIGIN)) < fc.DEVICE_HOST_GATE
    assert fc.scaled_diff(ipdip, mol.dipole_grad_integrals(ORIGIN)) < fc.DEVICE_HOST_GATE
    F = np.array([0.01, -0.02, 0.015])
    ref = mol.with_field(F, ORIGIN)
    aob = dg.integrals(R, field=F, origin=ORIGIN)
    for k in ("hcore", "dhcore", "gnuc", "S", "eri", "ipovlp", "eri_ip1"):
        d = fc.scaled_diff(getattr(aob, k)[0].cpu().numpy(), getattr(ref, k))
        print("field", k, "%.1e" % d)
        assert d < fc.DEVICE_HOST_GATE, k
    assert abs(float(aob.enuc[0].cpu()) - ref.enuc) < fc.DEVICE_HOST_GATE
    assert fc.scaled_diff(ref.hcore, mol.hcore) > 1e-4             # the field did something
    # field=None: the arrays of a producer that has never seen a field, bit for bit, and nothing kept for one
    from evcont_amd.gto_spdf_device import DeviceSpdfGaussians
    fresh = DeviceSpdfGaussians(dg._charges_host, dg.shells, device=DEV)
    plain, other = dg.integrals(R), fresh.integrals(R)
    for k in ("S", "hcore", "eri", "ipovlp", "dhcore", "eri_ip1", "enuc", "gnuc"):
        assert torch.equal(getattr(plain, k), getattr(other, k)), k
    assert not fresh._ipdip and not fresh._dip and not fresh._field
    # to_mol: a device-made molecule of the f class whose with_coords goes back through the device
    m = dg.to_mol(R)
    assert type(m).__name__ == "DeviceMadeSpdfMol" and m.producer is dg
    assert fc.scaled_diff(m.eri, mol.eri) < fc.DEVICE_HOST_GATE
    m2 = m.with_coords(R + 0.01)
    assert type(m2) is type(m) and fc.scaled_diff(m2.eri, mol.eri) < 1e-13      # (a translation)
    assert fc.scaled_diff(m.dipole_grad_integrals(ORIGIN), ipdip) == 0.0


def geometry(r, ang, seed=None, amp=0.05):
    from evcont_amd.gto_small import water_coords
    R = water_coords(r, ang)
    return R if seed is None else R + amp * np.random.default_rng(seed).standard_normal((3, 3))


@pytest.fixture(scope="module")
def water():
    """(producer, (S, one, two) of three CAS training states) of water / STO-3G + f, N = 14."""
    from evcont_amd.CASCI_EVCont import CAS_EVCont_obj
    from evcont_amd.fci_small import SmallFCI
    from evcont_amd.gto_spdf_device import DeviceSpdfGaussians
    _, Z, shells = fc.water_sto3g_f()
    dg = DeviceSpdfGaussians(Z, shells, nelec=(5, 5), device=DEV)
    assert dg.nao == 14
    # two electrons in THREE orbitals (1b1, 4a1, 2b2): a fourth active orbital would be the lowest of the seven nearly
    # degenerate f virtuals of O, whose character changes from geometry to geometry, and the CAS pair reduction refuses
    # states whose active spaces differ in character
    cont = CAS_EVCont_obj(3, 2, cisolver=SmallFCI())
    for r, ang in ((1.6, 100.0), (1.85, 106.0), (2.2, 112.0)):
        cont.append_to_rdms(dg.to_mol(geometry(r, ang), need_grad=False))
    return dg, (cont.overlap, cont.one_rdm, cont.two_rdm)


@pytest.mark.parametrize("packed", [True, False])
def test_energies_and_forces_match_uploaded_host_integrals(water, packed):
    from evcont_amd.evaluator import BatchedEvaluator, DeviceAOBatch, DeviceTRDMs
    dg, (S, one, two) = water
    mol = fc.load_water_ref()
    R = mol.atom_coords()
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
    disp = np.repeat(R[None], 19, axis=0)
    h = 2e-4
    for k in range(9):
        disp[1 + 2 * k].reshape(-1)[k] += h
        disp[2 + 2 * k].reshape(-1)[k] -= h
    E, _, g = ev19.multistate_energies_with_grads(dg.integrals(disp, packed=packed), 2, pairs)
    E, g = np.array(E), np.array(g)
    fd = ((E[1::2] - E[2::2]) / (2 * h)).T.reshape(E.shape[1], 3, 3)
    print("max |grad - fd| =", np.abs(g[0] - fd).max())
    assert np.abs(g[0] - fd).max() < 2e-7
    assert np.abs(g[0] - g1[0]).max() < 1e-10


def test_swarm_follows_the_host_route(water):
    from evcont_amd.MD_utils import _device_producer, state_swarm
    from evcont_amd.gto_spdf_device import DeviceSpdfGaussians
    dg, (S, one, two) = water
    mols = [dg.to_mol(geometry(1.8088, 104.5, seed=s)) for s in (5, 6)]
    assert _device_producer(mols[0]) is DeviceSpdfGaussians
    v0 = 1e-4 * np.random.default_rng(9).standard_normal((2, 3, 3))
    host = state_swarm(mols, one, two, S, root=1, dt=4.0, steps=2, init_veloc=v0)
    dev = state_swarm(mols, one, two, S, root=1, dt=4.0, steps=2, init_veloc=v0, integrals="device")
    assert len(dev) == len(host) == 2
    for fh, fd in zip(host, dev):
        assert np.abs(fd["coord"] - fh["coord"]).max() < 1e-10
        assert np.abs(fd["epot"] - fh["epot"]).max() < 1e-10


def test_tz_shape_water():
    """N = 58, 42 primitives: the packed forms and one batched evaluation of two copies of one geometry."""
    import torch
    from evcont_amd.evaluator import BatchedEvaluator, DeviceTRDMs
    from evcont_amd.gto_spdf_device import DeviceSpdfGaussians
    _, R, Z, shells = fc.tz_shape_water()
    dg = DeviceSpdfGaussians(Z, shells, nelec=(5, 5), device=DEV)
    assert dg.nao == 58 and dg.exponents.shape[0] == 42
    aob = dg.integrals(np.stack([R, R]), packed=True)
    n, ms = 58, 58 * 59 // 2
    S = aob.S.cpu().numpy()
    assert np.isfinite(S).all() and np.abs(np.diagonal(S, axis1=1, axis2=2) - 1.0).max() < 1e-12
    assert np.array_equal(S, S.transpose(0, 2, 1)) and np.array_equal(S[0], S[1])
    assert np.linalg.eigvalsh(S[0]).min() > 1e-4
    assert aob.eri.shape == (2, ms, ms) and aob.eri_ip1.shape == (2, 3, n, n, ms)
    assert bool(torch.isfinite(aob.eri).all()) and bool(torch.isfinite(aob.eri_ip1).all())
    assert torch.equal(aob.eri[0], aob.eri[1]) and torch.equal(aob.eri_ip1[0], aob.eri_ip1[1])
    # the s4 form is the packed full form: sampled rows against a full-form call on one geometry
    full = dg.integrals(R, packed=False)
    iu, ju = np.tril_indices(n)
    for row in (0, 17, 700, ms - 1):
        got = aob.eri[0, row].cpu().numpy()
        assert np.array_equal(got, full.eri[0, iu[row], ju[row]].cpu().numpy()[iu, ju]), row
        # (bra and ket of an element run different code: the exchange symmetry holds to rounding)
        assert fc.scaled_diff(got, aob.eri[0, :, row].cpu().numpy()) < 1e-13
    assert np.array_equal(aob.eri_ip1[0, 1, 40, 3].cpu().numpy(), full.eri_ip1[0, 1, 40, 3].cpu().numpy()[iu, ju])
    # one batched evaluation on seeded training tensors: finite, and the same for the two copies
    from evcont_amd.synthetic import make_trdms
    ov, one, two = make_trdms(n, 2, 5801)
    trd = DeviceTRDMs(one, two, ov, DEV, compress="sym8")
    ev = BatchedEvaluator(trd, 3, 2)
    E, _, g = ev.multistate_energies_with_grads(aob, 1, [(0, 0)])
    E, g = np.array(E), np.array(g)
    assert np.isfinite(E).all() and np.isfinite(g).all()
    assert E[0, 0] == E[1, 0] and np.array_equal(g[0], g[1])
