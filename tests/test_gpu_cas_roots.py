"""GPU tests of several CASCI roots per geometry on the device route:
``DeviceFCI.cas_trans_rdm12_block`` row by row against the single-bra call (bit for bit, dense and packed) and against
the host statement, ``CAS_EVCont_obj(..., cisolver=DeviceFCI(), nroots=2)`` against the same container on the host
solver, through multistate energies and forces, and one swarm on an excited surface of water with a d shell whose
integrals are made on the device."""
import functools

import numpy as np
import pytest
import torch

from evcont_amd import cas_small
from evcont_amd.fci_small import SmallFCI
from cas_reference import near_rotation, random_orthogonal, random_state
from fci_pack_reference import pack_cols

pytestmark = pytest.mark.gpu
SPACINGS = (1.6, 1.8, 2.0)
# |E_tot(k) - E_tot(0)| over the 5 frames of test_swarm_on_an_excited_surface_of_water_with_a_d_shell, measured on the
# host-integrals route of the same run; the test allows a decade more
DRIFT_HOST_ROUTE = 2.65e-5


def chain(natm, d, need_grad=False):
    from evcont_amd.hchain import hydrogen_chain
    return hydrogen_chain(natm, d, need_grad=need_grad)


def worst(got, want):
    return max(float(np.abs(np.asarray(g) - np.asarray(w)).max()) for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def solver():
    from evcont_amd.fci_device import DeviceFCI
    return DeviceFCI()


@functools.lru_cache(maxsize=None)
def h6_states():
    """Three roots at each of three spacings, solved on the host: 9 states, three orbital sets."""
    return tuple(s for d in SPACINGS for s in cas_small.casci_roots(chain(6, d), 4, 4, SmallFCI(spin_penalty=0.2), 3))


def random_states(core):
    rng = np.random.default_rng(21)
    U0 = random_orthogonal(7, rng)
    U1 = near_rotation(U0, rng)
    return [random_state(7, 2 if core else 0, 3, (2, 1), rng, U=U) for U in (U0, U0, U1, U1)]


def packed_rows(n, layout, count):
    ld = (pack_cols(layout, n) + 15) // 16 * 16
    return torch.full((count, ld), float("nan"), dtype=torch.float64, device="cuda:0")


def check_block_against_rows(states, bras, n):
    s = solver()
    R, K = len(bras), len(states)
    ov, one, two = s.cas_trans_rdm12_block(bras, states)
    assert ov.shape == (R, K) and one.shape == (R, K, n, n) and two.shape == (R, K) + (n,) * 4
    for r, bra in enumerate(bras):
        rows = s.cas_trans_rdm12_rows(bra, states)
        assert np.array_equal(ov[r], rows[0]) and np.array_equal(one[r], rows[1]) and np.array_equal(two[r], rows[2]), r
    for layout in ("pack2", "sym8"):
        out = packed_rows(n, layout, R * K)
        pov, pone = s.cas_trans_rdm12_block(bras, states, layout=layout, out_rows=out)
        torch.cuda.synchronize()
        assert np.array_equal(pov, ov) and np.array_equal(pone, one), layout
        got = out.cpu().numpy()
        for r, bra in enumerate(bras):
            single = packed_rows(n, layout, K)
            s.cas_trans_rdm12_rows(bra, states, layout=layout, out_rows=single)
            torch.cuda.synchronize()
            assert np.array_equal(got[r * K:(r + 1) * K], single.cpu().numpy()), (layout, r)
    return ov, one, two


def test_block_rows_are_the_single_bra_rows_h6():
    states = list(h6_states())
    for g in range(3):
        bras = states[3 * g:3 * g + 3]
        got = check_block_against_rows(states, bras, 6)
        err = worst(got, cas_small.trans_rdm12_block(bras, states))
        print(f"cas device block H6 geometry {g} against the host statement: {err:.2e}")
        assert err <= 1e-13
    again = solver().cas_trans_rdm12_block(states[:3], states)
    assert worst(again, solver().cas_trans_rdm12_block(states[:3], states)) == 0.0


@pytest.mark.parametrize("core", [True, False])
def test_block_rows_on_a_shape_with_core_and_virtuals(core):
    states = random_states(core)
    for bras in (states[:2], states[2:]):
        got = check_block_against_rows(states, bras, 7)
        want = cas_small.trans_rdm12_block(bras, states)
        # 128 * 2^-53 times the formula on absolute values (tests/test_gpu_cas_expand.py) is at most 128 * 2^-53 times
        # the sum of |terms|; on these well-conditioned pairs the issue's 1e-13 is the bound used
        err = worst(got, want)
        print(f"cas device block random shape core={core}: {err:.2e}")
        assert err <= 1e-13
    with pytest.raises(ValueError, match="orbitals"):
        solver().cas_trans_rdm12_block([states[0], states[2]], states)
    with pytest.raises(Exception, match="out_rows"):
        solver().cas_trans_rdm12_block(states[:2], states, layout="sym8", out_rows=packed_rows(7, "sym8", 3))


def test_a_pair_beyond_the_guard_is_refused_before_any_launch():
    from cas_reference import sweep_pair
    bra, ket = sweep_pair(1.0e6, np.random.default_rng(46))
    twin = random_state(7, 2, 3, (2, 1), np.random.default_rng(1), U=bra.U)
    from evcont_amd import _lib
    solver()._dev()                                     # the library is loaded
    before = _lib.load().evc_profile_kernel(_lib.FCI_PROF_ROTATE)
    with pytest.raises(ValueError, match="s_eff"):
        solver().cas_trans_rdm12_block([bra, twin], [bra, ket])
    assert _lib.load().evc_profile_kernel(_lib.FCI_PROF_ROTATE) == before


# ---- the container -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def containers():
    from evcont_amd.CASCI_EVCont import CAS_EVCont_obj
    from evcont_amd.fci_device import DeviceFCI
    dev = CAS_EVCont_obj(4, 4, cisolver=DeviceFCI(spin_penalty=0.2), nroots=2)
    host = CAS_EVCont_obj(4, 4, cisolver=SmallFCI(spin_penalty=0.2), nroots=2)
    for d in SPACINGS:
        dev.append_to_rdms(chain(6, d))
        host.append_to_rdms(chain(6, d))
    return dev, host


def signs(cont):
    return np.array([np.sign(s.ci.reshape(-1)[np.argmax(np.abs(s.ci))]) for s in cont.cascis])


def test_device_container_against_the_host_container():
    dev, host = containers()
    assert dev.ntrain == host.ntrain == 6 and dev.mol_index == host.mol_index == [0, 0, 1, 1, 2, 2]
    sd, sh = signs(dev), signs(host)
    fix = lambda c, s: (c.overlap * np.outer(s, s), c.one_rdm * np.outer(s, s)[:, :, None, None],
                        c.two_rdm * np.outer(s, s)[:, :, None, None, None, None])
    err = worst(fix(dev, sd), fix(host, sh))
    print(f"cas device container (2 roots) against the host container: {err:.2e}")
    assert err <= 1e-12
    assert np.abs(np.asarray(dev.ens) - np.asarray(host.ens)).max() <= 1e-10


def test_multistate_energies_and_forces_on_both_containers():
    from evcont_amd.ab_initio_gradients_loewdin import get_multistate_energy_with_grad
    dev, host = containers()
    mol = chain(6, 1.7, need_grad=True)
    R0 = mol.atom_coords()
    R0 = R0 + 0.03 * np.random.default_rng(3).standard_normal(R0.shape)
    mol = mol.with_coords(R0)
    Ed, gd = get_multistate_energy_with_grad(mol, dev.one_rdm, dev.two_rdm, dev.overlap, nroots=2)
    Eh, gh = get_multistate_energy_with_grad(mol, host.one_rdm, host.two_rdm, host.overlap, nroots=2)
    Ed, gd, Eh, gh = (np.asarray(x) for x in (Ed, gd, Eh, gh))
    print(f"2-root CAS containers at a shaken H6: E = {Ed}, |dE| = {np.abs(Ed - Eh).max():.2e}, "
          f"|dF| = {np.abs(gd - gh).max():.2e}")
    assert np.abs(Ed - Eh).max() <= 1e-10 and np.abs(gd - gh).max() <= 1e-9
    # root 1: the force against a central difference of the continuation energy on the fixed training data
    h = 1e-3
    energy = lambda R: float(np.asarray(get_multistate_energy_with_grad(
        mol.with_coords(R), dev.one_rdm, dev.two_rdm, dev.overlap, nroots=2)[0])[1])
    worst_fd = 0.0
    for atom, axis in ((0, 2), (2, 0), (5, 2)):
        Rp, Rm = R0.copy(), R0.copy()
        Rp[atom, axis] += h
        Rm[atom, axis] -= h
        fd = (energy(Rp) - energy(Rm)) / (2 * h)
        worst_fd = max(worst_fd, abs(fd - gd[1, atom, axis]))
    print(f"root 1: max |grad - central difference| = {worst_fd:.2e}")
    assert worst_fd <= 1e-6


def test_invariance_against_the_fci_container():
    """H4, every orbital active: two CAS roots per geometry span what two FCI roots span."""
    from oracle.evcont_oracle import approximate_multistate, integrals_oao
    from evcont_amd.CASCI_EVCont import CAS_EVCont_obj
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    cas = CAS_EVCont_obj(4, 4, cisolver=SmallFCI(), nroots=2)
    fci = FCI_EVCont_obj(cisolver=SmallFCI(), cibasis="canonical", nroots=2)
    for d in SPACINGS:
        cas.append_to_rdms(chain(4, d))
        fci.append_to_rdms(chain(4, d))
    assert cas.ntrain == fci.ntrain == 6 and cas.cascis[0].ncore == 0
    for d in (1.7, 1.9):
        mol = chain(4, d)
        h1, h2 = integrals_oao(mol)
        a = approximate_multistate(h1, h2, cas.one_rdm, cas.two_rdm, cas.overlap, nroots=2)[0]
        b = approximate_multistate(h1, h2, fci.one_rdm, fci.two_rdm, fci.overlap, nroots=2)[0]
        print(f"H4 at {d}: CAS container {a + mol.enuc}, FCI container {b + mol.enuc}")
        assert np.abs(a - b).max() <= 1e-10


# ---- water with a d shell ------------------------------------------------------------------------------------------
def test_swarm_on_an_excited_surface_of_water_with_a_d_shell():
    """Water in STO-3G plus the cc-pVDZ d shell on O (N = 12): three CAS(4,4) geometries of two roots each, integrals
    from ``DeviceSpdGaussians``; five frames on root 1."""
    from evcont_amd import gto_spd as gd
    from evcont_amd.CASCI_EVCont import CAS_EVCont_obj
    from evcont_amd.MD_utils import state_swarm
    from evcont_amd.fci_device import DeviceFCI
    from evcont_amd.gto_spd_device import DeviceSpdGaussians
    charges, shells = gd.water_shells("sto-3g")
    shells[0] = shells[0] + [gd.Shell(*gd.CCPVDZ["O"][-1])]
    dg = DeviceSpdGaussians(charges, shells, device="cuda")
    assert dg.nao == 12
    cont = CAS_EVCont_obj(4, 4, cisolver=DeviceFCI(spin_penalty=0.2), nroots=2)
    for r in (0.90, 0.99, 1.08):
        cont.append_to_rdms(dg.to_mol(gd.water_coords(r * gd.ANGSTROM, 104.5), need_grad=False))
    assert cont.ntrain == 6 and cont.cascis[0].ncore == 3
    mol = dg.to_mol(gd.water_coords(0.96 * gd.ANGSTROM, 104.5))
    frames = state_swarm([mol], cont.one_rdm, cont.two_rdm, cont.overlap, root=1, dt=4.0, steps=5, integrals="device")
    assert len(frames) == 5
    etot = np.array([f["epot"][0] + f["ekin"][0] for f in frames])
    assert np.isfinite(etot).all() and all(np.isfinite(f["coord"]).all() for f in frames)
    drift = float(np.abs(etot - etot[0]).max())
    print(f"water + d, root 1, 5 frames: E_tot = {etot[0]:.10f}, drift {drift:.2e} (bound {10 * DRIFT_HOST_ROUTE:.1e})")
    assert drift <= 10.0 * DRIFT_HOST_ROUTE
