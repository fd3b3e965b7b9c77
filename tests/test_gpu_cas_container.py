"""GPU tests of the device route of the CAS container: ``CAS_EVCont_obj(..., cisolver=DeviceFCI())`` and
``DeviceFCI.cas_trans_rdm12_rows`` (rotate, active-space row call, ``evc_cas_expand_rows``) against the full-space
embedding oracle (tests/cas_reference.py), the host container, and -- beyond the ceiling of the built-in full CI, where the
oracle cannot go -- the host statement ``cas_small.trans_rdm12_rows`` that tests/test_cas_host.py pins at small N."""
import functools

import numpy as np
import pytest
import torch

from evcont_amd import cas_small
from evcont_amd.fci_small import SmallFCI
from cas_reference import oracle_rows
from fci_pack_reference import pack_cols, pack_row

pytestmark = pytest.mark.gpu
SPACINGS = (1.6, 1.8, 2.1)


def chain(natm, d, need_grad=False):
    from evcont_amd.hchain import hydrogen_chain
    return hydrogen_chain(natm, d, need_grad=need_grad)


def worst(got, want):
    return max(float(np.abs(np.asarray(g) - np.asarray(w)).max()) for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def containers():
    from evcont_amd.CASCI_EVCont import CAS_EVCont_obj
    from evcont_amd.fci_device import DeviceFCI
    dev, host = CAS_EVCont_obj(4, 4, cisolver=DeviceFCI()), CAS_EVCont_obj(4, 4, cisolver=SmallFCI())
    for d in SPACINGS:
        dev.append_to_rdms(chain(6, d))
        host.append_to_rdms(chain(6, d))
    return dev, host


def test_device_container_against_the_oracle_and_the_host_container():
    dev, host = containers()
    assert dev.ntrain == 3 and dev.two_rdm.shape == (3, 3, 6, 6, 6, 6)
    assert all(s.ncore == 1 and s.nelecas == (2, 2) for s in dev.cascis)
    for i in range(3):
        want = oracle_rows(dev.cascis[i], dev.cascis[:i + 1])
        got = (dev.overlap[i, :i + 1], dev.one_rdm[i, :i + 1], dev.two_rdm[i, :i + 1])
        err = worst(got, want)
        print(f"cas device container row {i}: worst |d| against the oracle = {err:.2e}")
        assert err <= 1e-10
    err = worst((dev.overlap, dev.one_rdm, dev.two_rdm, dev.ens), (host.overlap, host.one_rdm, host.two_rdm, host.ens))
    print(f"cas device container against the host container: {err:.2e}")
    assert err <= 1e-10
    assert np.abs(np.diag(dev.overlap) - 1.0).max() <= 1e-10


def test_evaluator_at_a_training_geometry():
    from evcont_amd.ab_initio_gradients_loewdin import get_energy_with_grad
    dev, _ = containers()
    for i, d in enumerate(SPACINGS):
        e, g = get_energy_with_grad(chain(6, d, need_grad=True), dev.one_rdm, dev.two_rdm, dev.overlap)
        print(f"cas evaluator at geometry {i}: E = {float(e):.12f}  CASCI = {dev.ens[i]:.12f}")
        assert float(e) <= dev.ens[i] + 1e-9
        assert np.isfinite(np.asarray(g)).all()


@functools.lru_cache(maxsize=None)
def h18_pair():
    """Two CAS(4,4) states of H18 (ncore = 7, N = 18: beyond the 16 orbitals of the built-in full CI)."""
    from evcont_amd.fci_device import DeviceFCI
    solver = DeviceFCI()
    states = [cas_small.casci(chain(18, d), 4, 4, solver) for d in (1.8, 1.9)]
    assert all(s.ncore == 7 and s.U.shape == (18, 18) for s in states)
    dense = solver.cas_trans_rdm12_rows(states[1], states)
    return solver, states, dense


def test_beyond_the_fci_ceiling_against_the_host_statement():
    _, states, dense = h18_pair()
    want = cas_small.trans_rdm12_rows(states[1], states)
    err = worst(dense, want)
    print(f"cas H18 CAS(4,4) device row against the host statement: {err:.2e}  overlap = {dense[0]}")
    assert err <= 1e-10
    assert abs(dense[0][1] - 1.0) <= 1e-10 and abs(np.trace(dense[1][1]) - 18.0) <= 1e-9


def test_packed_row_has_the_bits_of_compress_sym8():
    from evcont_amd.evaluator import DeviceTRDMs
    solver, states, (ov, one, two) = h18_pair()
    n, cols = 18, pack_cols("sym8", 18)
    ld = (cols + 15) // 16 * 16
    rows = torch.full((2, ld), float("nan"), dtype=torch.float64, device="cuda:0")
    pov, pone = solver.cas_trans_rdm12_rows(states[1], states, layout="sym8", out_rows=rows)
    torch.cuda.synchronize()
    got = rows.cpu().numpy()
    assert np.array_equal(pov, ov) and np.array_equal(pone, one)
    for i in range(2):
        assert np.array_equal(got[i, :cols], pack_row("sym8", two[i])) and not got[i, cols:].any(), i
        t = DeviceTRDMs(one[i][None, None], two[i][None, None], np.ones((1, 1)), "cuda:0", compress="sym8")
        assert t.layout == 8 and np.array_equal(got[i], t.two[0].cpu().numpy()), i
    with pytest.raises(Exception, match="out_rows"):
        solver.cas_trans_rdm12_rows(states[1], states, layout="sym8", out_rows=rows[:1])
