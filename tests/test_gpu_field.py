"""GPU tests of a molecule in a uniform electric field on the device (csrc/field.hip: evc_sgto_dipole_grad_batch,
evc_gto_dipole_grad_batch, evc_field_fold_batch; ``integrals(..., field=)`` of the three device producers;
``get_multistate_field_response``; ``state_swarm(..., field=)``) against the host statements of evcont_amd/field.py and
the numpy oracle.

Tolerances.
* The gradient calls against the host statements: what the dipole tests of the same routes use, 1e-10 absolute for the
  s route (tests/test_gpu_properties.py) and ``scaled_diff`` < DEVICE_HOST_GATE = 1e-10 for the shell routes
  (tests/spgto_cases.py).  The identity ipdip + ipdip^T = -delta_xc S: 1e-12 of the array's scale, as on the host.
* The fold against numpy ON THE DEVICE'S OWN dip / ipdip: every element is its old value plus at most six products
  |F| |integral| <= 0.05 x 10, summed in another order than numpy's einsum: a few ulp of 10, bound 1e-13.
* ``integrals(R, field=F)`` through the batched evaluator against the oracle on ``with_field`` molecules: the project's
  parity, 1e-10 Ha and 1e-9 Ha/Bohr.
* ``get_multistate_field_response``, device against host route at the same step h: both routes differ by the parity
  at each field point, and a central difference divides the difference of two points by 2h: dipoles to 1e-10 give
  alpha to 2 x 1e-10 / 2h = 1e-10 / h, forces to 1e-9 give the atomic polar tensor to 1e-9 / h (1e-7 and 1e-6 at
  h = 1e-3).  The sum rule is the difference of two net forces over 2h; a net force is A force components, each held to
  the parity: A x 1e-9 / h.
* One column of the atomic polar tensor against Richardson-combined central differences of the device dipoles over
  that coordinate (steps k and k/2): 10 x (|FD(k) - FD(k/2)| + |apt(h) - apt(h/2)|), both gaps measured on the CPU with
  the numpy oracle in place of the device (``python tests/test_gpu_field.py``; the truncation errors are properties of
  the functions, not of the route): k = 4e-3: 4.0e-7; h = 1e-3: 1.7e-9 -> 4.0e-6 (there the Richardson value and the
  finite-field value differ by 5.8e-10).
* The swarm in a static field: frames of both routes as the field-free swarm tests hold them (1e-10); the drift of
  epot + ekin over the four steps at most 10 x the drift of the field-free run of the same length.  Measured on MI355X:
  SWARM_MEASURED below.

Measured on MI355X (worst of each kind): ipdip against the host statements 3.6e-15 (the 24-atom chain; 6.4e-16 with d
shells); the fold against numpy 1.4e-17; energies and forces in a field against the oracle 2.7e-12 Ha and 3.4e-13
Ha/Bohr; the response, device against host route: alpha 5.7e-9 (bound 1e-7), atomic polar tensor 2.4e-9 (bound 1e-6); the
sum rule 3.3e-12 (bound 4e-6); the tensor column against displaced-geometry dipoles 2.0e-9 (bound 4.0e-6).
"""
import ctypes as C

import numpy as np
import pytest

import spgto_cases as sc
from oracle import evcont_oracle as orc
from test_field_host import (H4_COORDS, H4_ORIGIN, ORIGIN, bent_h3, h4_training, host_dipoles,   # noqa: F401 (fixture)
                             oracle_energies, oracle_response, spd_molecule)
from test_hchain_physics import bundle

DEV = "cuda"
BAR = 1e-10
H4_CHARGES = (1.0, 2.0, 0.5, 1.0)
# epot + ekin of the four-step swarm of test_swarm_in_a_static_field, measured on MI355X: max drift with the field and
# without it (Hartree)
SWARM_MEASURED = "field 2.19e-05, field-free 2.20e-05"
APT_COLUMN_TOL = 10.0 * (4.0e-7 + 1.7e-9)


def producer_for(mol):
    from evcont_amd.MD_utils import _device_producer
    return _device_producer(mol).from_mol(mol, device=DEV)


def shaken(mol, G, amp=0.05, seed=7):
    rng = np.random.default_rng(seed)
    return np.stack([mol.coords + (amp * rng.standard_normal(mol.coords.shape) if k else 0.0) for k in range(G)])


def molecules():
    from evcont_amd import gto_small, hchain
    return {"h3": bent_h3(), "water_sto3g": gto_small.water("sto-3g", need_grad=False),
            "water_631g": gto_small.water("6-31g", need_grad=False), "spd": spd_molecule(),
            "h24": hchain.hydrogen_chain(24, 1.8, need_grad=False)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["h3", "water_sto3g", "water_631g", "spd", "h24"])
def test_gradient_calls_against_the_host_statements(name):
    import torch
    mol = molecules()[name]
    sg = producer_for(mol)
    R = shaken(mol, 3)
    got = sg.dipole_grad_integrals(R, ORIGIN).clone()
    singles = [sg.dipole_grad_integrals(R[g], ORIGIN).clone() for g in range(3)]
    again = sg.dipole_grad_integrals(torch.from_numpy(R).to(DEV), ORIGIN)
    torch.cuda.synchronize()
    n = mol.nao
    assert got.shape == (3, 3, 3, n, n)
    # geometry g of a batch = the call on it alone, bit for bit; twice the same bits
    assert torch.equal(got, again)
    for g in range(3):
        assert torch.equal(got[g], singles[g][0]), g
    a = got.cpu().numpy()
    worst = 0.0
    for g in range(3):
        want = mol.with_coords(R[g], need_grad=False).dipole_grad_integrals(ORIGIN)
        d = np.abs(a[g] - want).max() if name in ("h3", "h24") else sc.scaled_diff(a[g], want)
        worst = max(worst, d)
    print(f"{name}: device ipdip against the host statement {worst:.2e}")
    assert worst < (BAR if name in ("h3", "h24") else sc.DEVICE_HOST_GATE)
    # the identity against S of the integrals call
    S = sg.integrals(R, need_grad=False).S.cpu().numpy()
    scale = np.abs(a).max()
    for x in range(3):
        for c in range(3):
            want = -S if x == c else 0.0 * S
            assert np.abs(a[:, x, c] + a[:, x, c].transpose(0, 2, 1) - want).max() < 1e-12 * scale, (x, c)


def fold_call(lib, n, A, G, dip, ipdip, slices, charges, R, F, origin, flags, out):
    import torch
    from evcont_amd import _lib
    o = (C.c_double * 3)(*origin)
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(lib.evc_field_fold_batch(n, A, G, ptr(dip), ptr(ipdip), ptr(slices), ptr(charges), ptr(R), ptr(F),
                                        C.cast(o, C.c_void_p), flags, ptr(out["hcore"]), ptr(out.get("dhcore")),
                                        ptr(out["enuc"]), ptr(out.get("gnuc")), torch.cuda.current_stream().cuda_stream),
               "evc_field_fold_batch")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["h4", "water_sto3g", "spd"])
def test_fold_against_numpy(name):
    """Three different fields in one batch (the second is zero), straight through the C call."""
    import torch
    from evcont_amd import _lib, hchain
    from evcont_amd.field import field_terms
    mol = hchain.s_gaussian_mol(H4_COORDS, H4_CHARGES, need_grad=False) if name == "h4" else molecules()[name]
    sg = producer_for(mol)
    G, A, n = 3, mol.natm, mol.nao
    R = shaken(mol, G)
    aob = sg.integrals(R)
    Rd = sg.staged_coords(G)
    keys = ("hcore", "dhcore", "enuc", "gnuc")
    before = {k: getattr(aob, k).clone() for k in keys}
    dip, ipdip = sg.dipole_integrals(Rd, ORIGIN), sg.dipole_grad_integrals(Rd, ORIGIN)
    F = np.array([[0.01, -0.02, 0.015], [0.0, 0.0, 0.0], [-0.03, 0.004, 0.02]])
    Fd = torch.from_numpy(F).to(DEV)
    out = {k: before[k].clone() for k in keys}
    fold_call(sg.lib, n, A, G, dip, ipdip, aob.aoslices, sg.charges, Rd, Fd, ORIGIN, 0, out)
    worst = 0.0
    for g in range(G):
        dh, ddh, de, dg = field_terms(F[g], ORIGIN, dip[g].cpu().numpy(), ipdip[g].cpu().numpy(), mol.aoslices,
                                      mol.charges, R[g])
        for k, add in (("hcore", dh), ("dhcore", ddh), ("enuc", de), ("gnuc", dg)):
            worst = max(worst, float(np.abs(out[k][g].cpu().numpy() - (before[k][g].cpu().numpy() + add)).max()))
    print(f"{name}: fold against numpy {worst:.2e}")
    assert worst < 1e-13
    # it did something, the zero field nothing, and the mirror symmetry is exact
    for k in keys:
        assert not torch.equal(out[k][0], before[k][0]), k
        assert torch.equal(out[k][1], before[k][1]), k
    assert torch.equal(out["hcore"], out["hcore"].transpose(1, 2))
    assert torch.equal(out["dhcore"], out["dhcore"].transpose(3, 4))
    # a zero field for every geometry: every array as it was
    zero = {k: before[k].clone() for k in keys}
    fold_call(sg.lib, n, A, G, dip, ipdip, aob.aoslices, sg.charges, Rd, torch.zeros_like(Fd), ORIGIN, 0, zero)
    for k in keys:
        assert torch.equal(zero[k], before[k]), k
    # energy only: hcore and enuc as above, sentinel-filled dhcore and gnuc untouched -- and they may be absent
    sent = {"hcore": before["hcore"].clone(), "enuc": before["enuc"].clone(),
            "dhcore": torch.full_like(before["dhcore"], -7.25), "gnuc": torch.full_like(before["gnuc"], -7.25)}
    fold_call(sg.lib, n, A, G, dip, ipdip, aob.aoslices, sg.charges, Rd, Fd, ORIGIN, _lib.FLAG_ENERGY_ONLY, sent)
    assert torch.equal(sent["hcore"], out["hcore"]) and torch.equal(sent["enuc"], out["enuc"])
    assert bool((sent["dhcore"] == -7.25).all()) and bool((sent["gnuc"] == -7.25).all())
    bare = {"hcore": before["hcore"].clone(), "enuc": before["enuc"].clone()}
    fold_call(sg.lib, n, A, G, dip, None, None, sg.charges, Rd, Fd, ORIGIN, _lib.FLAG_ENERGY_ONLY, bare)
    assert torch.equal(bare["hcore"], out["hcore"]) and torch.equal(bare["enuc"], out["enuc"])


@pytest.mark.gpu
def test_integrals_without_a_field_enqueue_what_they_did():
    """``field=None``: the arrays of the call are those of a producer that has never seen a field, bit for bit, and a
    field given as (3,) is the same field for every geometry."""
    import torch
    from evcont_amd import hchain
    mol = hchain.s_gaussian_mol(H4_COORDS, H4_CHARGES, need_grad=False)
    R = shaken(mol, 2)
    a, b = producer_for(mol), producer_for(mol)
    F = np.array([0.01, -0.02, 0.015])
    one = {k: getattr(a.integrals(R, field=F, origin=H4_ORIGIN), k).clone() for k in ("hcore", "dhcore", "enuc", "gnuc")}
    two = a.integrals(R, field=np.stack([F, F]), origin=H4_ORIGIN)
    for k, v in one.items():
        assert torch.equal(v, getattr(two, k)), k
    plain, fresh = a.integrals(R), b.integrals(R)
    for k in ("S", "hcore", "eri", "ipovlp", "dhcore", "eri_ip1", "enuc", "gnuc"):
        assert torch.equal(getattr(plain, k), getattr(fresh, k)), k
    assert not b._ipdip and not b._dip and not b._field


@pytest.fixture(scope="module")
def water_training():
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    from evcont_amd.fci_small import SmallFCI
    from evcont_amd.gto_small import water
    cont = FCI_EVCont_obj(cisolver=SmallFCI(), cibasis="OAO")
    for r, ang in ((1.6, 100.0), (1.85, 106.0), (2.2, 112.0)):
        cont.append_to_rdms(water("sto-3g", r, ang, need_grad=False))
    return cont.overlap, cont.one_rdm, cont.two_rdm


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["h4", "water_sto3g"])
@pytest.mark.parametrize("packed", [False, True])
def test_integrals_in_a_field_through_the_batched_evaluator(h4_training, water_training, name, packed):
    from evcont_amd import gto_small, hchain
    from evcont_amd.evaluator import BatchedEvaluator, DeviceTRDMs
    if name == "h4":
        mol, tr = hchain.s_gaussian_mol(H4_COORDS), h4_training
    else:
        mol, tr = gto_small.water("sto-3g", 1.8088, 104.5), water_training
    S, one, two = tr
    G, A = 3, mol.natm
    R = shaken(mol, G)
    F = np.array([[0.01, -0.02, 0.015], [0.0, 0.0, 0.0], [-0.03, 0.004, 0.02]])
    sg = producer_for(mol)
    ev = BatchedEvaluator(DeviceTRDMs(one, two, S, DEV, compress="sym8" if packed else None), A, G)
    E, _, grads = ev.multistate_energies_with_grads(sg.integrals(R, packed=packed, field=F, origin=H4_ORIGIN), 2)
    E, grads = np.array(E), np.array(grads)
    de = dg = 0.0
    for g in range(G):
        m = mol.with_coords(R[g]).with_field(F[g], H4_ORIGIN)
        Eo = oracle_energies(m, tr)[0]
        E0, g0 = orc.energy_with_grad(bundle(m), one, two, S)
        assert abs(Eo[0] - E0) < 1e-12                    # (the oracle's several-roots energies include enuc)
        de, dg = max(de, np.abs(E[g] - Eo).max()), max(dg, np.abs(grads[g, 0] - g0).max())
    print(f"{name} packed={packed}: max |dE| = {de:.2e}, max |dgrad| = {dg:.2e}")
    assert de < 1e-10 and dg < 1e-9
    # the field is felt: the zero-field geometry aside, the energies moved by far more than the parity
    E_free = np.array(ev.multistate_energies_with_grads(sg.integrals(R, packed=packed), 2)[0])
    assert np.abs(E[1] - E_free[1]).max() < 1e-12 and np.abs(E[0] - E_free[0]).min() > 1e-5


@pytest.mark.gpu
def test_field_response_device_against_host_and_finite_differences(h4_training):
    from evcont_amd import hchain
    from evcont_amd.ab_initio_eigenvector_continuation import (get_multistate_field_response,
                                                               get_multistate_properties)
    S, one, two = h4_training
    h, R = 1e-3, 2
    for charges, Q in (((1.0, 1.0, 1.0, 1.0), 0.0), ((1.0, 2.0, 1.0, 1.0), 1.0)):
        mol = hchain.s_gaussian_mol(H4_COORDS, charges=charges, nelec=(2, 2))
        host = get_multistate_field_response(mol, one, two, S, R, h, origin=H4_ORIGIN)
        dev = get_multistate_field_response(mol, one, two, S, R, h, origin=H4_ORIGIN, integrals="device")
        assert set(host) == set(dev) == {"energies", "dipole", "polarizability", "apt"}
        assert dev["energies"].shape == (R,) and dev["dipole"].shape == (R, 3)
        assert dev["polarizability"].shape == (R, 3, 3) and dev["apt"].shape == (R, 4, 3, 3)
        gaps = {k: float(np.abs(dev[k] - host[k]).max()) for k in host}
        rule = {k: float(np.abs(r["apt"].sum(axis=1) - Q * np.eye(3)).max()) for k, r in (("host", host), ("device", dev))}
        print(f"Q = {Q}: device - host {gaps}; sum rule {rule}")
        assert gaps["energies"] < 1e-10 and gaps["dipole"] < 1e-10
        assert gaps["polarizability"] < 1e-10 / h and gaps["apt"] < 1e-9 / h
        assert max(rule.values()) < 4 * 1e-9 / h
        # the zero-field point is the field-free molecule
        E0, p0 = get_multistate_properties([mol], one, two, S, R, origin=H4_ORIGIN)
        assert np.abs(dev["energies"] - E0[0]).max() < 1e-10 and np.abs(dev["dipole"] - p0["dipole"][0]).max() < 1e-10
    # one column of the atomic polar tensor of the ground state, d mu / dR_Ax for A = 1, x = 1, against central differences
    # of the dipoles of displaced geometries (the cation above)
    at, x, k = 1, 1, 4e-3
    disp = []
    for s in (k, -k, k / 2, -k / 2):
        Rs = H4_COORDS.copy()
        Rs[at, x] += s
        disp.append(mol.with_coords(Rs, need_grad=False))
    mu = get_multistate_properties(disp, one, two, S, 1, origin=H4_ORIGIN)[1]["dipole"][:, 0]
    a, b = (mu[0] - mu[1]) / (2 * k), (mu[2] - mu[3]) / k
    err = float(np.abs((4.0 * b - a) / 3.0 - dev["apt"][0, at, x]).max())
    print(f"apt column: |FD(k) - FD(k/2)| = {np.abs(a - b).max():.2e}, |Richardson - finite field| = {err:.2e}")
    assert err < APT_COLUMN_TOL


@pytest.mark.gpu
def test_swarm_in_a_static_field(h4_training):
    from evcont_amd import hchain
    from evcont_amd.MD_utils import state_swarm
    S, one, two = h4_training
    base = hchain.s_gaussian_mol(H4_COORDS)
    mols = [base, base.with_coords(shaken(base, 2)[1])]
    F = np.array([[0.01, -0.02, 0.015], [-0.03, 0.004, 0.02]])
    kw = dict(root=1, dt=4.0, steps=4, init_veloc=1e-4 * np.random.default_rng(9).standard_normal((2, 4, 3)))
    host = state_swarm(mols, one, two, S, field=F, field_origin=H4_ORIGIN, **kw)
    dev = state_swarm(mols, one, two, S, field=F, field_origin=H4_ORIGIN, integrals="device", **kw)
    free = state_swarm(mols, one, two, S, integrals="device", **kw)
    assert len(host) == len(dev) == len(free) == 4
    for fh, fd in zip(host, dev):
        assert set(fd) == set(fh) and fd["time"] == fh["time"]
        assert np.abs(fd["coord"] - fh["coord"]).max() < 1e-10 and np.abs(fd["epot"] - fh["epot"]).max() < 1e-10
        np.testing.assert_allclose(fd["veloc"], fh["veloc"], rtol=0, atol=1e-12)
    # epot of a frame includes the field terms
    m0 = mols[0].with_field(F[0], H4_ORIGIN)
    assert abs(dev[0]["epot"][0] - oracle_energies(m0, h4_training)[0][1]) < 1e-10
    assert abs(dev[0]["epot"][0] - free[0]["epot"][0]) > 1e-4
    # a callable field that is constant in time is that field
    pulse = state_swarm(mols, one, two, S, field=lambda t: F, field_origin=H4_ORIGIN, integrals="device", **kw)
    assert all(np.array_equal(p["coord"], d["coord"]) and np.array_equal(p["epot"], d["epot"]) for p, d in zip(pulse, dev))
    total = lambda frames: np.array([f["epot"] + f["ekin"] for f in frames])
    drift = {k: float(np.abs(total(f) - total(f)[0]).max()) for k, f in (("field", dev), ("field-free", free))}
    print(f"swarm: drift of epot + ekin over four steps {drift}")
    assert np.abs(dev[-1]["coord"] - dev[0]["coord"]).max() > 1e-3          # the atoms did move
    assert drift["field"] <= 10.0 * drift["field-free"]


if __name__ == "__main__":
    # the two truncation gaps behind APT_COLUMN_TOL, with the numpy oracle in place of the device
    from evcont_amd import hchain
    from test_hchain_physics import chain, train
    tr = train([chain(4, d) for d in (1.5, 2.0, 2.8)])[:3]
    Z = (1.0, 2.0, 1.0, 1.0)
    a, b = oracle_response(Z, tr, 1e-3), oracle_response(Z, tr, 5e-4)
    print("|apt(h) - apt(h/2)| column (1,1): %.2e" % np.abs(a["apt"][0, 1, 1] - b["apt"][0, 1, 1]).max())
    mol = hchain.s_gaussian_mol(H4_COORDS, charges=Z, nelec=(2, 2))

    def mu(s):
        Rs = H4_COORDS.copy()
        Rs[1, 1] += s
        m = mol.with_coords(Rs, need_grad=False)
        return host_dipoles(m, tr, oracle_energies(m, tr, 1)[1], H4_ORIGIN)[0]

    k = 4e-3
    fa, fb = (mu(k) - mu(-k)) / (2 * k), (mu(k / 2) - mu(-k / 2)) / k
    print("|FD(k) - FD(k/2)| = %.2e, |Richardson - apt(h/2)| = %.2e" % (
        np.abs(fa - fb).max(), np.abs((4 * fb - fa) / 3 - b["apt"][0, 1, 1]).max()))
