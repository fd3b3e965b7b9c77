"""GPU tests of the resident CAS training set: the triangular form of
``DeviceFCI.cas_trans_rdm12_block`` row by row against the rectangular call (bit for bit; dense, pack2 and sym8; host
and device-resident CI vectors), ``resident.ResidentCAS_EVCont_obj`` against the host container ``CAS_EVCont_obj`` on
the same ``DeviceFCI`` solver (the two-body rows bit for bit: both routes make the same sums in the same order), and
the routes that read it: multistate energies and forces, the water + d-shell swarm and the active-learning loop, to the
project's parity limits (1e-10 Ha, 1e-9 Ha/Bohr)."""
import functools

import numpy as np
import pytest
import torch

from evcont_amd import cas_small
from fci_pack_reference import pack_cols
from test_gpu_cas_roots import DRIFT_HOST_ROUTE, chain, h6_states, packed_rows, random_states, solver

pytestmark = pytest.mark.gpu
SPACINGS = (1.6, 1.8, 2.0)
PENALTY = 0.2


# ---- the triangular block call -------------------------------------------------------------------------------------
def on_device(states):
    """The same states with their CI vectors as device tensors; states that shared a ``U`` still share it."""
    return [cas_small.CASState(U=s.U, ncore=s.ncore, ncas=s.ncas, nelecas=s.nelecas,
                               ci=torch.from_numpy(np.ascontiguousarray(s.ci)).to("cuda:0"), e_tot=s.e_tot)
            for s in states]


def check_triangular(kets, R, n):
    """Every ragged row of the triangular call against row (r, k) of the rectangular one."""
    s = solver()
    K = len(kets)
    bras = kets[K - R:]
    counts = [K - R + r + 1 for r in range(R)]
    ov, one, two = s.cas_trans_rdm12_block(bras, kets)
    tov, tone, ttwo = s.cas_trans_rdm12_block(bras, kets, triangular=True)
    assert [len(x) for x in tov] == counts and len(tone) == len(ttwo) == R
    for r, c in enumerate(counts):
        assert tone[r].shape == (c, n, n) and ttwo[r].shape == (c,) + (n,) * 4
        assert np.array_equal(tov[r], ov[r, :c]) and np.array_equal(tone[r], one[r, :c]), r
        assert np.array_equal(ttwo[r], two[r, :c]), r
    for layout in ("pack2", "sym8"):
        rect = packed_rows(n, layout, R * K)
        s.cas_trans_rdm12_block(bras, kets, layout=layout, out_rows=rect)
        tri = packed_rows(n, layout, sum(counts))
        pov, pone = s.cas_trans_rdm12_block(bras, kets, layout=layout, out_rows=tri, triangular=True)
        torch.cuda.synchronize()
        rect, tri = rect.cpu().numpy(), tri.cpu().numpy()
        assert not np.isnan(tri).any()
        off = 0
        for r, c in enumerate(counts):
            assert np.array_equal(tri[off:off + c], rect[r * K:r * K + c]), (layout, r)
            assert np.array_equal(pov[r], ov[r, :c]) and np.array_equal(pone[r], one[r, :c]), (layout, r)
            off += c
    return tov, tone, ttwo


def test_triangular_rows_h6_host_and_device_vectors():
    states = list(h6_states())
    for T in (0, 3, 6):                                   # the three appends of a three-root container
        kets = states[:T + 3]
        got = check_triangular(kets, 3, 6)
        dgot = check_triangular(on_device(kets), 3, 6)    # (the bras are the last kets by identity in both lists)
        for a, b in zip(got, dgot):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), T
    check_triangular(states[:4], 1, 6)                    # one root: cas_trans_rdm12_rows' case
    rows = solver().cas_trans_rdm12_rows(states[3], states[:4])
    tri = solver().cas_trans_rdm12_block([states[3]], states[:4], triangular=True)
    assert all(np.array_equal(t[0], r) for t, r in zip(tri, rows))


@pytest.mark.parametrize("core", [True, False])
def test_triangular_rows_on_a_shape_with_core_and_virtuals(core):
    states = random_states(core)
    check_triangular(states, 2, 7)
    check_triangular(on_device(states), 2, 7)
    check_triangular(states[:2], 2, 7)


def test_triangular_refusals():
    states = list(h6_states())
    twin = cas_small.CASState(U=states[5].U, ncore=1, ncas=4, nelecas=states[5].nelecas, ci=states[5].ci.copy())
    for bras, kets in ((states[3:6], states[:5] + [twin]),       # equal, but not the bra itself
                       (states[3:6], states[:3] + [states[4], states[3], states[5]]),   # out of order
                       (states[3:6], states[4:6]),               # fewer kets than bras
                       (states[3:6], states[:6] + [states[0]])):
        with pytest.raises(ValueError, match="triangular"):
            solver().cas_trans_rdm12_block(bras, kets, triangular=True)
    with pytest.raises(Exception, match="out_rows"):
        solver().cas_trans_rdm12_block(states[3:6], states[:6], layout="sym8", out_rows=packed_rows(6, "sym8", 18),
                                       triangular=True)


def test_a_pair_beyond_the_guard_is_refused_before_any_launch():
    from cas_reference import random_state, sweep_pair
    from evcont_amd import _lib
    bra, ket = sweep_pair(1.0e6, np.random.default_rng(46))
    twin = random_state(7, 2, 3, (2, 1), np.random.default_rng(1), U=bra.U)
    solver()._dev()
    before = _lib.load().evc_profile_kernel(_lib.FCI_PROF_ROTATE)
    with pytest.raises(ValueError, match="s_eff"):
        solver().cas_trans_rdm12_block([bra, twin], [ket, bra, twin], triangular=True)
    assert _lib.load().evc_profile_kernel(_lib.FCI_PROF_ROTATE) == before


# ---- the container -------------------------------------------------------------------------------------------------
def device_fci():
    from evcont_amd.fci_device import DeviceFCI
    return DeviceFCI(spin_penalty=PENALTY)


def h6_mols():
    return [chain(6, d) for d in SPACINGS]


def grown(cls, mols, **kw):
    c = cls(4, 4, cisolver=device_fci(), **kw)
    for m in mols:
        c.append_to_rdms(m)
    return c


@functools.lru_cache(maxsize=None)
def host(nroots):
    from evcont_amd.CASCI_EVCont import CAS_EVCont_obj
    return grown(CAS_EVCont_obj, h6_mols(), nroots=nroots)


@functools.lru_cache(maxsize=None)
def resident(nroots, layout, capacity=16):
    from evcont_amd.resident import ResidentCAS_EVCont_obj
    return grown(ResidentCAS_EVCont_obj, h6_mols(), nroots=nroots, layout=layout, capacity=capacity)


def host_rows(c, layout):
    """The host codec applied to ``two_rdm[a, b]``, ``a >= b``: what the evaluator's upload of the host arrays holds."""
    from evcont_amd.evaluator import DeviceTRDMs
    if layout == "pack2":
        return c.device_trdms("pack2").two.cpu().numpy()
    return DeviceTRDMs(c.one_rdm, c.two_rdm, c.overlap, compress="sym8").two.cpu().numpy()


def same_bits(res, hst, layout):
    t = res.device_trdms()
    assert t.T == hst.ntrain == res.ntrain and t.layout == {"pack2": 2, "sym8": 8}[layout]
    want = host_rows(hst, layout)
    assert np.array_equal(t.two.cpu().numpy(), want)
    rows = res.rows_host()
    assert rows.shape == (t.T * (t.T + 1) // 2, pack_cols(layout, t.n)) and np.array_equal(rows, want[:, :rows.shape[1]])
    assert np.array_equal(res.overlap, hst.overlap) and np.array_equal(res.one_rdm, hst.one_rdm)
    assert res.mol_index == hst.mol_index and np.array_equal(res.ens, hst.ens)


@pytest.mark.parametrize("layout", ["pack2", "sym8"])
@pytest.mark.parametrize("nroots", [1, 2])
def test_h6_container_has_the_bits_of_the_host_container(nroots, layout):
    r, h = resident(nroots, layout), host(nroots)
    assert r.ntrain == 3 * nroots and r.mol_index == [g for g in range(3) for _ in range(nroots)]
    same_bits(r, h, layout)
    assert r.device_trdms() is r.device_trdms() and r.device_trdms(layout) is r.device_trdms()
    assert len(r.cascis) == len(r._dstates) == r.ntrain
    for hs, ds, ref in zip(r.cascis, r._dstates, h.cascis):
        assert isinstance(hs.ci, np.ndarray) and np.array_equal(hs.ci, ref.ci)          # the record on the host
        assert torch.is_tensor(ds.ci) and ds.ci.is_cuda and ds.U is hs.U                  # the kets of the next append
        assert np.array_equal(ds.ci.cpu().numpy(), hs.ci)


@pytest.mark.parametrize("layout", ["pack2", "sym8"])
def test_growth_inside_a_block_views_and_prune(layout):
    """capacity=2 with two roots per geometry: the second append (T = 2, R = 2) must grow before its block call, the
    third (T = 4, R = 2) again; the bits are those of capacity=16 and a view taken before keeps its rows."""
    from evcont_amd.resident import ResidentCAS_EVCont_obj
    mols = h6_mols()
    small = ResidentCAS_EVCont_obj(4, 4, cisolver=device_fci(), nroots=2, layout=layout, capacity=2)
    small.append_to_rdms(mols[0])
    early = small.device_trdms()
    early_bits = early.two.cpu().numpy().copy()
    assert early.T == 2 and small._res.capacity == 2
    small.append_to_rdms(mols[1])
    assert small._res.capacity == 4
    small.append_to_rdms(mols[2])
    assert small._res.capacity == 8 and small.ntrain == 6
    big = resident(2, layout)
    assert big._res.capacity == 16
    assert np.array_equal(small.device_trdms().two.cpu().numpy(), big.device_trdms().two.cpu().numpy())
    assert np.array_equal(small.overlap, big.overlap) and np.array_equal(small.one_rdm, big.one_rdm)
    assert early.T == 2 and np.array_equal(early.two.cpu().numpy(), early_bits)
    assert np.array_equal(early_bits, big.device_trdms().two[:3].cpu().numpy())
    # prune: strictly increasing ids only, gathered on the device, against the host container pruned alike
    from evcont_amd.CASCI_EVCont import CAS_EVCont_obj
    h = grown(CAS_EVCont_obj, mols, nroots=2)
    for bad in ([2, 0], [1, 1], [0, 6]):
        with pytest.raises(ValueError):
            small.prune_datapoints(bad)
    assert small.ntrain == 6
    late = small.device_trdms()
    for c in (small, h):
        c.prune_datapoints([0, 3, 4])
    same_bits(small, h, layout)
    assert len(small.cascis) == len(small._dstates) == len(small.ens) == 3 and small.device_trdms() is not late
    assert late.T == 6 and np.array_equal(late.two.cpu().numpy(), big.device_trdms().two.cpu().numpy())
    # and the pruned container keeps growing
    small.append_to_rdms(mols[1])
    h.append_to_rdms(mols[1])
    same_bits(small, h, layout)


def test_two_rdm_attribute_and_refusals():
    from evcont_amd._lib import EvcontHipError
    from evcont_amd.fci_small import SmallFCI
    from evcont_amd.resident import ResidentCAS_EVCont_obj
    empty = ResidentCAS_EVCont_obj(4, 4, cisolver=device_fci())
    assert empty.two_rdm is None and empty.ntrain == 0 and empty.layout == "sym8" and empty.roots_train == [0]
    with pytest.raises(ValueError):
        empty.device_trdms()
    with pytest.raises(ValueError):
        empty.rows_host()
    for layout in ("pack2", "sym8"):
        with pytest.raises(EvcontHipError, match=r"device_trdms\(\).*rows_host\(\)"):
            resident(1, layout).two_rdm
    with pytest.raises(EvcontHipError, match="sym8"):
        resident(1, "pack2").device_trdms("sym8")
    with pytest.raises(EvcontHipError, match="pack2"):
        resident(1, "sym8").device_trdms("pack2")
    with pytest.raises(EvcontHipError, match="cas_trans_rdm12_block"):
        ResidentCAS_EVCont_obj(4, 4, cisolver=SmallFCI())

    class Rectangular:                                     # a block call without the triangular form
        def cas_trans_rdm12_block(self, bras, kets, layout=None, out_rows=None):
            raise AssertionError

    with pytest.raises(EvcontHipError, match="triangular"):
        ResidentCAS_EVCont_obj(4, 4, cisolver=Rectangular())
    with pytest.raises(ValueError):
        ResidentCAS_EVCont_obj(4, 4, cisolver=device_fci(), layout="pair5")


def test_a_refused_append_leaves_the_container_as_it_was(monkeypatch):
    """The roots of the refused geometry are injected through cas_small.casci_roots: a pair beyond the conditioning
    guard raises before any launch; rows, lists and view stay, and the container keeps growing afterwards."""
    from evcont_amd import _lib
    from evcont_amd.resident import ResidentCAS_EVCont_obj
    mols = h6_mols()
    c = ResidentCAS_EVCont_obj(4, 4, cisolver=device_fci(), nroots=2, layout="pack2", capacity=2)
    c.append_to_rdms(mols[0])
    view = c.device_trdms()
    before = view.two.cpu().numpy().copy()
    lists = (list(c.cascis), list(c._dstates), list(c.ens), list(c.mol_index), c.overlap.copy(), c.one_rdm.copy())
    real = cas_small.casci_roots

    def swapped(mol, ncas, nelecas, cisolver, nroots):
        roots = real(mol, ncas, nelecas, cisolver, nroots)
        U = roots[0].U.copy()
        U[:, [0, 1]] = U[:, [1, 0]]                        # core and first active orbital change places: s_cc = 0
        return [cas_small.CASState(U=U, ncore=s.ncore, ncas=s.ncas, nelecas=s.nelecas, ci=s.ci, e_tot=s.e_tot)
                for s in roots]

    monkeypatch.setattr(cas_small, "casci_roots", swapped)
    rotate_before = _lib.load().evc_profile_kernel(_lib.FCI_PROF_ROTATE)
    with pytest.raises(ValueError, match="ill-conditioned"):
        c.append_to_rdms(mols[0])
    assert _lib.load().evc_profile_kernel(_lib.FCI_PROF_ROTATE) == rotate_before
    monkeypatch.setattr(cas_small, "casci_roots", real)
    assert c.ntrain == 2 and c._res.T == 2 and c.device_trdms() is view
    assert np.array_equal(view.two.cpu().numpy(), before) and np.array_equal(c.rows_host(), before[:, :c._res.cols])
    for now, was in zip((c.cascis, c._dstates, c.ens, c.mol_index), lists):
        assert len(now) == len(was) and all(a is b or a == b for a, b in zip(now, was))
    assert np.array_equal(c.overlap, lists[4]) and np.array_equal(c.one_rdm, lists[5])
    c.append_to_rdms(mols[1])
    c.append_to_rdms(mols[2])
    assert c.mol_index == [0, 0, 1, 1, 2, 2]
    assert np.array_equal(c.device_trdms().two.cpu().numpy(), resident(2, "pack2").device_trdms().two.cpu().numpy())


# ---- downstream ----------------------------------------------------------------------------------------------------
def shaken_h6():
    mol = chain(6, 1.7, need_grad=True)
    R0 = mol.atom_coords()
    return mol.with_coords(R0 + 0.03 * np.random.default_rng(3).standard_normal(R0.shape))


@pytest.mark.parametrize("layout", ["pack2", "sym8"])
def test_energies_forces_and_couplings_through_device_trdms(layout):
    from evcont_amd.ab_initio_gradients_loewdin import (get_multistate_energies_with_grads,
                                                        get_multistate_energy_with_grad)
    from evcont_amd.ab_initio_eigenvector_continuation import get_multistate_properties
    mol = shaken_h6()
    # one root per geometry, the ground state
    h, r = host(1), resident(1, layout)
    Eh, gh = get_multistate_energy_with_grad(mol, h.one_rdm, h.two_rdm, h.overlap, nroots=1)
    Er, gr = get_multistate_energy_with_grad(mol, None, None, None, nroots=1, device_trdms=r.device_trdms())
    print(f"resident CAS {layout}, one root: |dE|={np.abs(Er - Eh).max():.2e} |dg|={np.abs(gr - gh).max():.2e}")
    assert np.abs(Er - Eh).max() <= 1e-10 and np.abs(gr - gh).max() <= 1e-9
    # two roots per geometry, with the couplings
    h, r = host(2), resident(2, layout)
    Eh, gh, ch = get_multistate_energy_with_grad(mol, h.one_rdm, h.two_rdm, h.overlap, nroots=2, return_couplings=True)
    Er, gr, cr = get_multistate_energy_with_grad(mol, r.one_rdm, None, r.overlap, nroots=2, return_couplings=True,
                                                 device_trdms=r.device_trdms())
    dc = np.abs(cr - ch).max()          # (both routes hold the same training data to the bit: the same eigenvectors)
    print(f"resident CAS {layout}, two roots: |dE|={np.abs(Er - Eh).max():.2e} |dg|={np.abs(gr - gh).max():.2e} "
          f"|dh|={dc:.2e}")
    assert np.abs(Er - Eh).max() <= 1e-10 and np.abs(gr - gh).max() <= 1e-9
    assert dc <= 1e-9
    # the batched call and the observables read the same view
    mols = [mol, chain(6, 1.9, need_grad=True)]
    Eb, gb = get_multistate_energies_with_grads(mols, None, None, None, nroots=2, device_trdms=r.device_trdms())
    Ehb, ghb = get_multistate_energies_with_grads(mols, h.one_rdm, h.two_rdm, h.overlap, nroots=2)
    assert np.abs(Eb - Ehb).max() <= 1e-10 and np.abs(gb - ghb).max() <= 1e-9
    assert np.abs(Eb[0] - Er).max() <= 1e-10
    Ep, props = get_multistate_properties(mols, None, None, None, nroots=2, device_trdms=r.device_trdms())
    Ehp, hprops = get_multistate_properties(mols, h.one_rdm, h.two_rdm, h.overlap, nroots=2)
    assert np.abs(Ep - Ehp).max() <= 1e-10 and np.abs(props["dipole"] - hprops["dipole"]).max() <= 1e-9


def test_swarm_on_water_with_a_d_shell_from_the_resident_container():
    """The five-frame swarm of tests/test_gpu_cas_roots.py on root 1, its training set grown on the device and read
    through ``state_swarm(..., device_trdms=)``; the same drift bound."""
    from evcont_amd import gto_spd as gd
    from evcont_amd.MD_utils import state_swarm
    from evcont_amd.gto_spd_device import DeviceSpdGaussians
    from evcont_amd.resident import ResidentCAS_EVCont_obj
    charges, shells = gd.water_shells("sto-3g")
    shells[0] = shells[0] + [gd.Shell(*gd.CCPVDZ["O"][-1])]
    dg = DeviceSpdGaussians(charges, shells, device="cuda")
    cont = ResidentCAS_EVCont_obj(4, 4, cisolver=device_fci(), nroots=2, layout="sym8")
    for r in (0.90, 0.99, 1.08):
        cont.append_to_rdms(dg.to_mol(gd.water_coords(r * gd.ANGSTROM, 104.5), need_grad=False))
    assert cont.ntrain == 6 and cont.cascis[0].ncore == 3
    mol = dg.to_mol(gd.water_coords(0.96 * gd.ANGSTROM, 104.5))
    frames = state_swarm([mol], cont.one_rdm, None, cont.overlap, root=1, dt=4.0, steps=5, integrals="device",
                         device_trdms=cont.device_trdms())
    assert len(frames) == 5
    etot = np.array([f["epot"][0] + f["ekin"][0] for f in frames])
    assert np.isfinite(etot).all() and all(np.isfinite(f["coord"]).all() for f in frames)
    drift = float(np.abs(etot - etot[0]).max())
    print(f"water + d, root 1, resident container: E_tot = {etot[0]:.10f}, drift {drift:.2e} "
          f"(bound {10 * DRIFT_HOST_ROUTE:.1e})")
    assert drift <= 10.0 * DRIFT_HOST_ROUTE


def test_active_learning_h4_resident_cas_against_host(tmp_path):
    """converge_EVCont_MD with a resident CAS container and with the host CAS container, both on DeviceFCI: the same
    training times, overlaps within 1e-12; several roots per geometry are refused by the loop."""
    from evcont_amd.CASCI_EVCont import CAS_EVCont_obj
    from evcont_amd.MD_utils import converge_EVCont_MD
    from evcont_amd.hchain import s_gaussian_mol
    from evcont_amd.resident import ResidentCAS_EVCont_obj
    from test_hchain_physics import bent_chain
    m0 = s_gaussian_mol(bent_chain(4, d=1.7, seed=2, amp=0.03))
    conts = {"host": CAS_EVCont_obj(2, 2, cisolver=device_fci()),
             "resident": ResidentCAS_EVCont_obj(2, 2, cisolver=device_fci(), layout="sym8", capacity=1)}
    traj = {}
    for name, c in conts.items():
        d = tmp_path / name
        d.mkdir()
        traj[name] = converge_EVCont_MD(c, m0, steps=12, dt=5.0, convergence_thresh=1e-4, workdir=str(d),
                                        max_iterations=2)
    assert traj["host"].shape == (12, 4, 3)
    assert conts["host"].ntrain == conts["resident"].ntrain >= 2
    np.testing.assert_allclose(conts["resident"].overlap, conts["host"].overlap, rtol=0, atol=1e-12)
    assert np.array_equal(np.loadtxt(tmp_path / "host" / "trn_times.txt"),
                          np.loadtxt(tmp_path / "resident" / "trn_times.txt"))
    assert np.abs(traj["host"] - traj["resident"]).max() < 1e-8
    assert (tmp_path / "resident" / "two_rdm_sym8.npy").exists() and not (tmp_path / "resident" / "two_rdm.npy").exists()
    two = ResidentCAS_EVCont_obj(2, 2, cisolver=device_fci(), nroots=2)
    with pytest.raises(NotImplementedError, match="roots_train"):
        converge_EVCont_MD(two, m0, steps=2, workdir=str(tmp_path))
    assert two.ntrain == 0
    torch.cuda.synchronize()
