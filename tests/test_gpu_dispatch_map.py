"""Every row of tests/dispatch_table.py that needs no knob: the call runs once, each of the eight stages reports the
kernel the table names for it (``evc_profile_kernel``; a stage the call did not run reports ""), and the results of the
first, a middle and the last slot match ``oracle.energy_with_grad`` on the original pack2 rows and full integral arrays:
|dE| <= 1e-10 Ha, |dgrad| <= 1e-9 Ha/Bohr, and the predicted 1- and 2-RDMs to 1e-10 where the case asks for them.
The rows of the roots APIs hold every root pair of the first, a middle and the last geometry to the per-slot oracle
of tests/test_gpu_excited_forces.py (root k's total gradient on (k, k), the coupling vector on (k, l))."""
import numpy as np
import pytest
import torch

from evcont_amd import _lib
from evcont_amd.synthetic import make_device_ao, make_trdms, pack_rows
from oracle import evcont_oracle as orc

from dispatch_table import CASES, STAGES

pytestmark = pytest.mark.gpu

E_TOL, G_TOL, RDM_TOL = 1e-10, 1e-9, 1e-10
LAYOUT_PACK = {"full6": (False, False), "pair5": (True, False), "elec3": (False, True), "pack2": (True, True),
               "sym8": (True, True)}


def _records():
    lib = _lib.load()
    return {k: lib.evc_profile_kernel(_lib.PROF_STAGES[k]).decode() for k in STAGES}


def _assert_records(got, want, what):
    # (an expected IP1 record without "slots=" names the one-slot form: the multi-slot record does not match it)
    bad = {k: (got[k], want[k]) for k in STAGES
           if (got[k] != "" if want[k] == "" else not got[k].startswith(want[k]))
           or ("slots=" in got[k]) != ("slots=" in want[k])}
    assert not bad, (what, bad, got)


def _sym8(G):
    """Mean over the index permutations of real two-electron integrals: the 2-RDM the compressed layout predicts."""
    a = G + np.swapaxes(G, -4, -3)
    a = a + np.swapaxes(a, -2, -1)
    a = a + np.moveaxis(a, (-2, -1), (-4, -3))
    return a / 8.0


def _bundle(ao):
    c = lambda t: t.cpu().numpy()
    return orc.AOBundle(S=c(ao.S), hcore=c(ao.hcore), eri=c(ao.eri), ipovlp=c(ao.ipovlp), dhcore=c(ao.dhcore),
                        eri_ip1=c(ao.eri_ip1), aoslices=c(ao.aoslices), enuc=ao.enuc, gnuc=c(ao.gnuc))


ROOTS_APIS = ("roots", "roots_batch")


@pytest.mark.parametrize("c", [c for c in CASES if not c["env"] and c["api"] not in ROOTS_APIS], ids=lambda c: c["id"])
def test_dispatch_case(c):
    from evcont_amd import cache
    from evcont_amd.evaluator import BatchedEvaluator, ContinuationEvaluator, DeviceAOBatch, DeviceTRDMs
    cache.clear()
    dev = torch.device("cuda:0")
    n, T, A, G = c["n"], c["T"], c["A"], c["G"]
    seed = 31000 + 97 * n + 7 * T + G
    S, one, two = make_trdms(n, T, seed)
    two_p = pack_rows(two, True, True)
    two_l = pack_rows(two, *LAYOUT_PACK[c["layout"]]) if c["layout"] != "full6" else two
    del two
    trd = DeviceTRDMs(one, two_l, S, dev, compress="sym8" if c["layout"] == "sym8" else None)
    if not c["keep"] or c["layout"] in ("pack2", "sym8"):
        del two_l
    aos = [make_device_ao(n, A, seed * 100 + k, dev, ip1_rs_symmetric=True) for k in range(G)]
    run = [a.packed_ip1(eri=True) for a in aos] if c["packed"] else aos
    slots = sorted({0, G // 2, G - 1})
    if c["api"] == "single":
        assert G == 1
        ev = ContinuationEvaluator(trd, A, warm_start=c["warm"], want_two_rdm=c["keep"])
        geo = run[0]
    else:
        ev = BatchedEvaluator(trd, A, G, keep_density_matrices=c["keep"], warm_start=c["warm"])
        geo = DeviceAOBatch.stack(run)
    if c["warm"]:
        ev.enqueue(geo, c["nroots"])      # the cold call; the warm one below starts from its eigenvectors
        ev.synchronize()
    ev.enqueue(geo, c["nroots"], energy_only=c["energy_only"])
    ev.synchronize()
    _assert_records(_records(), c["expect"], "call")
    energy = ev.energy.reshape(G, T).cpu().numpy()
    if c["energy_only"]:
        ev.phase_gradient(geo, partial_rank=False)
        ev.synchronize()
        _assert_records(_records(), c["expect_grad"], "gradient phase after the energy-only call")
    grad = ev.grad.reshape(G, -1, 3)[:, :A].cpu().numpy()
    d_pred = ev.d_pred.reshape(G, n, n).cpu().numpy() if c["keep"] else None
    g_pred = ev.g_pred.reshape(G, n, n, n, n).cpu().numpy() if c["keep"] else None
    S_h = np.asarray(S)
    for k in slots:
        b = _bundle(aos[k])
        Eo, go, Do, Go = orc.energy_with_grad(b, one, two_p, S_h, return_density_matrices=True)
        assert abs(energy[k, 0] - Eo) <= E_TOL, (k, energy[k, 0] - Eo)
        dg = float(np.abs(grad[k] - go).max())
        assert dg <= G_TOL, (k, dg)
        if c["nroots"] > 1:
            eo, _ = orc.approximate_multistate_OAO(b, one, two_p, S_h, nroots=c["nroots"])
            de = float(np.abs(energy[k, : c["nroots"]] - eo).max())
            assert de <= E_TOL, (k, de)
        if c["keep"]:
            # (the synthetic t-RDMs are symmetric under bra <-> ket only together with p <-> q, r <-> s: a layout that
            #  keeps the pairs a >= b alone predicts the same energy but a different 2-RDM, so the 2-RDM is held to
            #  the oracle on the layout's own t-RDMs -- for the compressed layout, to the 8-fold symmetrised pack2 one)
            if c["layout"] not in ("pack2", "sym8"):
                _, _, Do, Go = orc.energy_with_grad(b, one, two_l, S_h, return_density_matrices=True)
            Go = np.asarray(Go).reshape(n, n, n, n)
            if c["layout"] == "sym8":
                Go = _sym8(Go)
            assert float(np.abs(d_pred[k] - Do).max()) <= RDM_TOL, (k, float(np.abs(d_pred[k] - Do).max()))
            assert float(np.abs(g_pred[k] - Go).max()) <= RDM_TOL, (k, float(np.abs(g_pred[k] - Go).max()))


@pytest.mark.parametrize("c", [c for c in CASES if not c["env"] and c["api"] in ROOTS_APIS], ids=lambda c: c["id"])
def test_dispatch_roots_case(c):
    from evcont_amd import cache
    from evcont_amd.evaluator import BatchedEvaluator, ContinuationEvaluator, DeviceAO, DeviceAOBatch, DeviceTRDMs
    from evcont_amd.synthetic import make_ao_arrays
    from test_gpu_excited_forces import Oracle
    cache.clear()
    dev = torch.device("cuda:0")
    n, T, A, G, nroots, pairs = c["n"], c["T"], c["A"], c["G"], c["nroots"], c["pairs"]
    seed = 31000 + 97 * n + 7 * T + G
    S, one, two = make_trdms(n, T, seed)
    two_p = pack_rows(two, True, True)
    two_l = pack_rows(two, *LAYOUT_PACK[c["layout"]]) if c["layout"] != "full6" else two
    del two
    trd = DeviceTRDMs(one, two_l, S, dev, compress="sym8" if c["layout"] == "sym8" else None)
    del two_l
    # (host-generated geometries: their root gaps are known, so the per-root oracle is well defined)
    aos = [make_ao_arrays(n, A, seed * 100 + k, ip1_rs_symmetric=True) for k in range(G)]
    daos = [DeviceAO.from_arrays(a, dev, pack_ip1=c["packed"], pack_eri=c["packed"]) for a in aos]
    if c["api"] == "roots":
        assert G == 1
        E, Cd, grads = ContinuationEvaluator(trd, A).energies_with_grads(daos[0], nroots, pairs)
        E, Cd, grads = E[None], Cd[None], grads[None]
    else:
        E, Cd, grads = BatchedEvaluator(trd, A, G).multistate_energies_with_grads(DeviceAOBatch.stack(daos), nroots,
                                                                                  pairs)
    _assert_records(_records(), c["expect"], "roots call")
    for k in sorted({0, G // 2, G - 1}):
        o = Oracle(aos[k], one, two_p, S, nroots)
        de = float(np.abs(E[k] - o.E).max())
        assert de <= E_TOL, (k, de)
        o.align(Cd[k])
        for p, (r, s) in enumerate(pairs):
            dg = float(np.abs(grads[k][p] - o.slot(r, s)).max())
            assert dg <= G_TOL, (k, (r, s), dg)
