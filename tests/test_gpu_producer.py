"""GPU tests of what the three device integral producers inherit from ``evcont_amd.producer.DeviceProducer``: the
buffers kept per ``(G, need_grad, packed)``, the workspace, the staging of host coordinates, ``out=``, and the field path,
on one small molecule per route (two geometries each):

* ``h4``: ``hydrogen_chain(4, 1.8)`` (``DeviceSGaussians``, N = 4);
* ``water``: ``gto_small.water("sto-3g")`` (``DeviceGaussians``, N = 7);
* ``spd``: one s + p + d centre of one-primitive shells and one s centre (``DeviceSpdGaussians``, N = 10).

Tolerances: the values against the host statements ``scaled_diff`` < ``DEVICE_HOST_GATE`` = 1e-10 (tests/spgto_cases.py);
``integrals(R, field=F)`` against the field-free call plus the host ``field.field_terms`` on the host statement's dipole
integrals 1e-10 absolute (the fold adds at most six products |F| |integral| per element, and the dipole integrals of the
routes are held to 1e-10 themselves); everything about buffers is an identity of pointers or of bits.

Left to the tests that already hold them for the s route: ``out=`` (test_gpu_sgto_limits.py,
``test_wrapper_writes_into_out_and_leaves_its_own_buffers``), the refusal of another molecule size (the same file) and
``field=None`` against a producer that never saw a field (test_gpu_field.py,
``test_integrals_without_a_field_enqueue_what_they_did``); here ``out=`` runs on the two shell routes, and ``field=None``
on all three against the same producer AFTER a call with a field."""
import numpy as np
import pytest

import spdgto_cases as dc
import spgto_cases as sc

DEV = "cuda"
NAMES = ("h4", "water", "spd")
ORIGIN = (0.1, -0.2, 0.3)
FIELD = np.array([[0.01, -0.02, 0.015], [-0.03, 0.004, 0.02]])
GRAD = ("ipovlp", "dhcore", "eri_ip1", "gnuc")


def _molecule(name):
    from evcont_amd import gto_small, gto_spd, hchain
    if name == "h4":
        return hchain.hydrogen_chain(4, 1.8)
    if name == "water":
        return gto_small.water("sto-3g")
    return gto_spd.spd_gaussian_mol([[0.0, 0.0, 0.0], [0.9, -0.6, 1.3]], [3.0, 1.0],
                                    [dc.spd_centre(1.1, 0.9, 0.8), [gto_spd.Shell(0, [0.7], [1.0])]])


@pytest.fixture(scope="module")
def host():
    """name -> (molecule, R (2,A,3), the host statement at R[0] and R[1])."""
    out = {}
    for name in NAMES:
        mol = _molecule(name)
        R = np.stack([mol.coords, mol.coords + 0.05 * np.random.default_rng(7).standard_normal(mol.coords.shape)])
        out[name] = (mol, R, [mol] + [mol.with_coords(R[1])])
    return out


def producer_for(mol):
    from evcont_amd.MD_utils import _device_producer
    return _device_producer(mol).from_mol(mol, device=DEV)


def check_values(aob, refs, need_grad, packed, order=(0, 1)):
    n = refs[0].nao
    for g, k in enumerate(order):
        ref = refs[k]
        eri = aob.eri[g].cpu().numpy()
        got = {"enuc": float(aob.enuc[g].cpu()), "S": aob.S[g].cpu().numpy(), "hcore": aob.hcore[g].cpu().numpy(),
               "eri": sc.unpack_eri(eri, n) if packed else eri}
        if need_grad:
            ip1 = aob.eri_ip1[g].cpu().numpy()
            got.update(ipovlp=aob.ipovlp[g].cpu().numpy(), dhcore=aob.dhcore[g].cpu().numpy(),
                       gnuc=aob.gnuc[g].cpu().numpy(), eri_ip1=sc.unpack_ip1(ip1, n) if packed else ip1)
        else:
            assert all(getattr(aob, f) is None for f in GRAD)
        for f, x in got.items():
            assert sc.scaled_diff(x, getattr(ref, f)) < sc.DEVICE_HOST_GATE, (f, g)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_a_steady_loop_of_one_shape_keeps_its_tensors(host, name):
    import torch
    mol, R, refs = host[name]
    p = producer_for(mol)
    for need_grad, packed in ((True, False), (False, True)):
        first = p.integrals(R, need_grad=need_grad, packed=packed)
        ws = p._ws.data_ptr()
        fields = [f for f in sc.NAMES if getattr(first, f) is not None]
        ptrs = {f: getattr(first, f).data_ptr() for f in fields}
        again = p.integrals(R[::-1].copy(), need_grad=need_grad, packed=packed)
        assert {f: getattr(again, f).data_ptr() for f in fields} == ptrs and p._ws.data_ptr() == ws
        # host coordinates went through the staging tensor of this G
        assert torch.equal(p.staged_coords(2).cpu(), torch.from_numpy(R[::-1].copy()))
        assert (p.natm, p.nao, again.natm) == (mol.natm, mol.nao, mol.natm) and (again.eri_s4, again.ip1_s2kl) == (packed, False)
        torch.cuda.synchronize()
        check_values(again, refs, need_grad, packed, order=(1, 0))
    assert sorted(p._buffers) == [(2, False, True), (2, True, False)] and list(p._coords) == [2]
    assert not p._dip and not p._ipdip and not p._field


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["water", "spd"])
def test_out_is_written_and_the_kept_buffers_are_not(host, name):
    import torch
    mol, R, refs = host[name]
    p = producer_for(mol)
    kept = p.integrals(R)
    before = {f: getattr(kept, f).clone() for f in sc.NAMES}
    out = p.allocate(2)
    for v in out.values():
        v.fill_(float("nan"))
    aob = p.integrals(R[::-1].copy(), out=out)
    torch.cuda.synchronize()
    assert all(getattr(aob, f).data_ptr() == out[f].data_ptr() for f in sc.NAMES)
    check_values(aob, refs, True, False, order=(1, 0))
    for f in sc.NAMES:
        assert torch.equal(getattr(kept, f), before[f]), f
    assert sorted(p.allocate(1, need_grad=False, packed=True)) == ["S", "enuc", "eri", "hcore"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_the_field_path_against_the_host_terms(host, name):
    import torch
    from evcont_amd.field import field_terms
    mol, R, refs = host[name]
    p = producer_for(mol)
    keys = ("hcore", "dhcore", "enuc", "gnuc")
    plain = {f: getattr(p.integrals(R), f).clone() for f in sc.NAMES}
    got = p.integrals(R, field=FIELD, origin=ORIGIN)
    torch.cuda.synchronize()
    worst = 0.0
    for g in range(2):
        adds = field_terms(FIELD[g], ORIGIN, refs[g].dipole_integrals(ORIGIN), refs[g].dipole_grad_integrals(ORIGIN),
                           mol.aoslices, mol.charges, R[g])
        for f, add in zip(keys, adds):
            want = plain[f][g].cpu().numpy() + add
            worst = max(worst, float(np.abs(getattr(got, f)[g].cpu().numpy() - want).max()))
    print(f"{name}: integrals(field=) against the field-free call plus the host terms {worst:.2e}")
    assert worst < 1e-10
    assert float((got.hcore - plain["hcore"]).abs().max()) > 1e-4                  # the field is felt
    for f in ("S", "eri", "ipovlp", "eri_ip1"):
        assert torch.equal(getattr(got, f), plain[f]), f
    # energy only, one field (3,) for both geometries: no dipole gradient is enqueued into a producer that has none yet
    q = producer_for(mol)
    e = q.integrals(R, need_grad=False, field=FIELD[0], origin=ORIGIN)
    assert list(q._dip) == [2] and not q._ipdip and list(q._field) == [2]
    for g in range(2):
        dh, _, de, _ = field_terms(FIELD[0], ORIGIN, refs[g].dipole_integrals(ORIGIN), None, mol.aoslices, mol.charges,
                                   R[g])
        assert np.abs(e.hcore[g].cpu().numpy() - (plain["hcore"][g].cpu().numpy() + dh)).max() < 1e-10
        assert abs(float(e.enuc[g].cpu()) - (float(plain["enuc"][g].cpu()) + de)) < 1e-10
    # no field again: the bits of the first call
    back = p.integrals(R, field=None)
    for f in sc.NAMES:
        assert torch.equal(getattr(back, f), plain[f]), f
