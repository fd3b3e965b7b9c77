"""GPU tests of the training set that grows on the device (evcont_amd/resident.py): ``ResidentFCI_EVCont_obj`` against
the host container ``FCI_EVCont_obj`` with the same ``DeviceFCI`` solver on hydrogen chains.  The two-body rows are the
same sums in the same order on both routes (csrc/fci_pack.hip states the order), so they are compared bit for bit;
energies and forces to the project's parity limits (1e-10 Ha, 1e-9 Ha/Bohr)."""
import numpy as np
import pytest
import torch

from evcont_amd.hchain import hydrogen_chain, s_gaussian_mol
from test_hchain_physics import bent_chain

pytestmark = pytest.mark.gpu

SPACINGS = (1.5, 2.0, 2.8)


def device_fci():
    from evcont_amd.fci_device import DeviceFCI
    return DeviceFCI()


def grown(cls, mols, **kw):
    c = cls(cisolver=device_fci(), cibasis="OAO", **kw)
    for m in mols:
        c.append_to_rdms(m)
    return c


def h6_mols():
    return [hydrogen_chain(6, d, need_grad=False) for d in SPACINGS]


@pytest.fixture(scope="module")
def host():
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    return grown(FCI_EVCont_obj, h6_mols())


@pytest.fixture(scope="module")
def resident():
    from evcont_amd.resident import ResidentFCI_EVCont_obj
    return {lay: grown(ResidentFCI_EVCont_obj, h6_mols(), layout=lay) for lay in ("pack2", "sym8")}


def host_rows(c, layout):
    """The device rows the host container's arrays give, in ``layout``."""
    from evcont_amd.evaluator import DeviceTRDMs
    if layout == "pack2":
        return c.device_trdms("pack2").two.cpu().numpy()
    return DeviceTRDMs(c.one_rdm, c.two_rdm, c.overlap, compress="sym8").two.cpu().numpy()


def same_bits(res, hst, layout):
    t = res.device_trdms()
    assert t.T == hst.ntrain == res.ntrain and t.layout == {"pack2": 2, "sym8": 8}[layout]
    assert np.array_equal(t.two.cpu().numpy(), host_rows(hst, layout))
    assert np.array_equal(res.overlap, hst.overlap) and np.array_equal(res.one_rdm, hst.one_rdm)
    assert np.array_equal(t.S.cpu().numpy(), hst.overlap)
    n2 = t.n * t.n
    assert np.array_equal(t.one[:, :n2].cpu().numpy().reshape(hst.one_rdm.shape), hst.one_rdm)


@pytest.mark.parametrize("layout", ["pack2", "sym8"])
def test_h6_rows_overlap_and_one_body_have_the_bits_of_the_host_container(host, resident, layout):
    r = resident[layout]
    same_bits(r, host, layout)
    assert r.mol_index == host.mol_index == [0, 1, 2] and np.array_equal(r.ens, host.ens)
    assert all(np.array_equal(a, b) for a, b in zip(r.fcivecs, host.fcivecs))
    assert r.device_trdms() is r.device_trdms() and r.device_trdms(layout) is r.device_trdms()
    rows = r.rows_host()
    assert rows.shape == (6, r.device_trdms().cols) and np.array_equal(rows, host_rows(host, layout)[:, :rows.shape[1]])


@pytest.mark.parametrize("layout", ["pack2", "sym8"])
def test_capacity_growth_views_and_prune(host, layout):
    """capacity=1 over four appends (two growths) gives the bits of capacity=8; a view taken at T=2 keeps T=2 and its
    bits through two more appends and a prune; pruning gives the bits of pruning the host container."""
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    from evcont_amd.resident import ResidentFCI_EVCont_obj
    mols = h6_mols() + [hydrogen_chain(6, 2.4, need_grad=False)]
    small = ResidentFCI_EVCont_obj(cisolver=device_fci(), cibasis="OAO", layout=layout, capacity=1)
    for m in mols[:2]:
        small.append_to_rdms(m)
    early = small.device_trdms()
    early_bits = early.two.cpu().numpy().copy()
    assert early.T == 2 and small._res.capacity == 2
    for m in mols[2:]:
        small.append_to_rdms(m)
    assert small._res.capacity == 4 and small.ntrain == 4
    big = grown(ResidentFCI_EVCont_obj, mols, layout=layout, capacity=8)
    assert big._res.capacity == 8
    assert np.array_equal(small.device_trdms().two.cpu().numpy(), big.device_trdms().two.cpu().numpy())
    assert np.array_equal(small.overlap, big.overlap) and np.array_equal(small.one_rdm, big.one_rdm)
    h4 = grown(FCI_EVCont_obj, mols)
    same_bits(small, h4, layout)
    with pytest.raises(ValueError):
        small.prune_datapoints([2, 0])
    assert small.ntrain == 4
    late = small.device_trdms()
    for c in (small, h4):
        c.prune_datapoints([0, 2])
    same_bits(small, h4, layout)
    assert len(small.fcivecs) == len(small.ens) == len(small._dvecs) == 2 and small.device_trdms() is not late
    assert np.array_equal(small.fcivecs[1], h4.fcivecs[1])
    assert early.T == 2 and early.two.shape[0] == 3 and np.array_equal(early.two.cpu().numpy(), early_bits)
    assert late.T == 4 and np.array_equal(late.two.cpu().numpy(), big.device_trdms().two.cpu().numpy())
    # the first two states of the pruned-from set are the early view: the prefix rule
    assert np.array_equal(early_bits, big.device_trdms().two[:3].cpu().numpy())
    # and the pruned container keeps growing
    small.append_to_rdms(mols[1])
    h4.append_to_rdms(mols[1])
    same_bits(small, h4, layout)


def test_two_rdm_attribute_and_refused_layouts(resident):
    from evcont_amd._lib import EvcontHipError
    from evcont_amd.fci_small import SmallFCI
    from evcont_amd.resident import ResidentFCI_EVCont_obj
    empty = ResidentFCI_EVCont_obj(cisolver=device_fci(), cibasis="OAO")
    assert empty.two_rdm is None and empty.ntrain == 0 and empty.layout == "sym8"
    with pytest.raises(ValueError):
        empty.device_trdms()
    for r in resident.values():
        with pytest.raises(EvcontHipError, match=r"device_trdms\(\).*rows_host\(\)"):
            r.two_rdm
    with pytest.raises(EvcontHipError, match="sym8"):
        resident["pack2"].device_trdms("sym8")
    with pytest.raises(EvcontHipError, match="trans_rdm12_rows_packed"):
        ResidentFCI_EVCont_obj(cisolver=SmallFCI(), cibasis="OAO")
    with pytest.raises(ValueError):
        ResidentFCI_EVCont_obj(cisolver=device_fci(), layout="pair5")


def test_forces_and_energies_on_the_bent_h6(host, resident):
    from evcont_amd.MD_utils import get_scanner
    from evcont_amd.ab_initio_gradients_loewdin import get_energy_with_grad
    m = s_gaussian_mol(bent_chain(6, d=1.9, seed=11, amp=0.15))
    Eh, gh = get_energy_with_grad(m, host.one_rdm, host.two_rdm, host.overlap)
    for layout, c in resident.items():
        E, g = get_scanner(m, c.one_rdm, None, c.overlap, device_trdms=c.device_trdms())(m)
        print(f"H6 resident {layout}: |dE|={abs(E - Eh):.2e} |dg|={np.abs(g - gh).max():.2e}")
        assert abs(E - Eh) < 1e-10 and np.abs(g - gh).max() < 1e-9
        mt = hydrogen_chain(6, 2.0)
        Et, _ = get_scanner(mt, c.one_rdm, None, c.overlap, device_trdms=c.device_trdms())(mt)
        assert abs(Et - c.ens[1]) < 1e-8
    # the pack2 rows on the host are the reference's two-index two_RDM
    c = resident["pack2"]
    Es, gs = get_scanner(m, c.one_rdm, None, c.overlap, device_trdms=c.device_trdms())(m)
    E2, g2 = get_energy_with_grad(m, c.one_rdm, c.rows_host(), c.overlap)
    assert abs(E2 - Es) < 1e-10 and np.abs(g2 - gs).max() < 1e-9


@pytest.mark.parametrize("layout", ["pack2", "sym8"])
def test_two_roots(layout):
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    from evcont_amd.resident import ResidentFCI_EVCont_obj
    mols = h6_mols()[:2]
    h = grown(FCI_EVCont_obj, mols, nroots=2, roots_train=[0, 1])
    r = grown(ResidentFCI_EVCont_obj, mols, nroots=2, roots_train=[0, 1], layout=layout, capacity=2)
    assert r.mol_index == h.mol_index == [0, 0, 1, 1] and r.ntrain == 4
    same_bits(r, h, layout)


def test_active_learning_h4_resident_against_host(tmp_path):
    """converge_EVCont_MD with a resident sym8 container and with a host container, both on DeviceFCI: the same
    training times, the last trajectory within 1e-8, and every sym8 checkpoint loads to the bits of the view the
    container had when it was written."""
    from evcont_amd import trdm_io
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    from evcont_amd.MD_utils import converge_EVCont_MD
    from evcont_amd.resident import ResidentFCI_EVCont_obj
    m0 = s_gaussian_mol(bent_chain(4, d=1.7, seed=2, amp=0.03))
    conts = {"host": FCI_EVCont_obj(cisolver=device_fci(), cibasis="OAO"),
             "resident": ResidentFCI_EVCont_obj(cisolver=device_fci(), cibasis="OAO", layout="sym8", capacity=1)}
    snapshots = []
    append = conts["resident"].append_to_rdms

    def append_and_snapshot(mol):
        append(mol)
        t = conts["resident"].device_trdms()
        snapshots.append((t.T, t.two.cpu().numpy().copy()))
    conts["resident"].append_to_rdms = append_and_snapshot
    traj = {}
    for name, c in conts.items():
        d = tmp_path / name
        d.mkdir()
        traj[name] = converge_EVCont_MD(c, m0, steps=12, dt=5.0, convergence_thresh=1e-4, workdir=str(d),
                                        max_iterations=3, prune_irrelevant_data=True)
    assert traj["host"].shape == (12, 4, 3)
    assert np.abs(traj["host"] - traj["resident"]).max() < 1e-8
    assert conts["host"].ntrain == conts["resident"].ntrain
    np.testing.assert_allclose(conts["resident"].overlap, conts["host"].overlap, rtol=0, atol=1e-12)
    n_saved = len(list((tmp_path / "resident").glob("overlap_*.npy")))
    assert n_saved == len(snapshots) >= 2 and n_saved == len(list((tmp_path / "host").glob("overlap_*.npy")))
    for i in range(1, n_saved):
        assert np.array_equal(np.loadtxt(tmp_path / "host" / f"trn_times_{i}.txt"),
                              np.loadtxt(tmp_path / "resident" / f"trn_times_{i}.txt")), i
    for i, (T, bits) in enumerate(snapshots):
        assert not (tmp_path / "resident" / f"two_rdm_{i}.npy").exists()
        t = trdm_io.load_checkpoint(str(tmp_path / "resident"), suffix=f"_{i}")
        assert t.layout == 8 and t.T == T and np.array_equal(t.two.cpu().numpy(), bits), i
    torch.cuda.synchronize()


def test_a_failed_row_call_leaves_the_container_as_it_was(resident):
    from evcont_amd._lib import EvcontHipError
    from evcont_amd.fci_device import DeviceFCI
    from evcont_amd.resident import ResidentFCI_EVCont_obj

    class Failing(DeviceFCI):
        fail = False

        def trans_rdm12_rows_packed(self, *a, **k):
            if self.fail:
                raise EvcontHipError("row call refused")
            return super().trans_rdm12_rows_packed(*a, **k)

    c = ResidentFCI_EVCont_obj(cisolver=Failing(), cibasis="OAO", layout="pack2", capacity=1)
    mols = h6_mols()
    c.append_to_rdms(mols[0])
    before = c.device_trdms().two.cpu().numpy().copy()
    c.cisolver.fail = True
    with pytest.raises(EvcontHipError, match="refused"):
        c.append_to_rdms(mols[1])
    assert c.ntrain == 1 and len(c.fcivecs) == len(c.ens) == len(c.mol_index) == len(c._dvecs) == 1
    assert np.array_equal(c.device_trdms().two.cpu().numpy(), before)
    c.cisolver.fail = False
    c.append_to_rdms(mols[1])
    c.append_to_rdms(mols[2])
    assert np.array_equal(c.device_trdms().two.cpu().numpy(), resident["pack2"].device_trdms().two.cpu().numpy())
    assert c.mol_index == [0, 1, 2]


def test_from_padded_rows_refuses_what_it_cannot_adopt(resident):
    from evcont_amd._lib import EvcontHipError
    from evcont_amd.evaluator import DeviceTRDMs
    r = resident["sym8"]
    t = r.device_trdms()
    wide = torch.zeros((t.two.shape[0], t.ld + 16), dtype=torch.float64, device=t.device)
    for bad in (t.two[:5], wide[:, :t.ld], t.two[:, :t.cols], t.two.float(), t.two.cpu()):
        with pytest.raises(EvcontHipError, match="from_padded_rows"):
            DeviceTRDMs.from_padded_rows(r.one_rdm, bad, r.overlap, 8)
    ok = DeviceTRDMs.from_padded_rows(r.one_rdm, t.two, r.overlap, 8)
    assert ok.two.data_ptr() == t.two.data_ptr() and ok.ld == t.ld


def test_the_loop_refuses_a_workdir_with_a_checkpoint_of_the_other_form(tmp_path):
    from evcont_amd._lib import EvcontHipError
    from evcont_amd.MD_utils import converge_EVCont_MD
    from evcont_amd.resident import ResidentFCI_EVCont_obj
    np.save(tmp_path / "two_rdm.npy", np.zeros((1, 1)))
    c = ResidentFCI_EVCont_obj(cisolver=device_fci(), cibasis="OAO", layout="sym8")
    with pytest.raises(EvcontHipError, match="two_rdm.npy exists"):
        converge_EVCont_MD(c, s_gaussian_mol(bent_chain(4, d=1.7, seed=2, amp=0.03)), steps=2, dt=5.0,
                           workdir=str(tmp_path), max_iterations=1)
    assert np.array_equal(np.load(tmp_path / "two_rdm.npy"), np.zeros((1, 1)))
