"""GPU sweep of the LDS-DMA pair-step kernels (csrc/pair_dma.hip: ptd_kernel<1>, ptd_kernel<0>, ptd_kernel<0, 1> "+ip1",
y2d_kernel<1> "pairstep") over EVERY orbital count they take, 17 <= N <= 30, on the fused (default) and
the unfused (EVC_Y2_PAIRSTEP=0 EVC_IP1_PAIRSTEP=0) route.

Every N is a shape class of its own (tests/pair_dma_shapes.py, held to the table on the CPU by
tests/test_pair_dma_shapes.py): passes of the write-out per wave, the counted waits cntA / cntB per wave, live pairs in
the last tile, the parity of npairs (the 16-byte DMA window shifts by one double on odd row starts) and, through the
batch size, 2 / 4 / 8 tiles per workgroup with a ragged last workgroup.

Inputs as tests/test_gpu_ip1_pairstep.py: make_trdms(n, 2, 300 + n) packed, compress="sym8", four atoms with AO blocks
(n - 7, 2, 2, 3), packed s4 / s2kl integrals.  Per N three distinct geometries and their oracle values, made once; slot
s of a batch of G holds geometry s % 3, so every geometry lands on even and on odd slots (odd npairs: both alignments
of the caller's s4 matrix).  EVERY slot is held to the oracle of its geometry, |dE| < 1e-9 and |dgrad| <= 1e-8 (the
neighbouring batched tests' bounds); fused against unfused forces within 1e-10; a second call on the same evaluator and
batch must be bit-identical (the pipeline sums in a fixed order: a mis-counted wait shows first as run-to-run noise).
Lines that start with "pair_dma_sweep:" carry the measured figures (profiles/pair_dma_sweep.txt).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, REPO)
import torch

from evcont_amd.synthetic import make_ao_arrays, make_trdms, pack_rows
from oracle import evcont_oracle as orc
from pair_dma_shapes import BOUNDARY, KEEP_SIZES, KNOBS_OFF, ROOTS_SIZES, SIZES, SWEEP
from test_gpu_ip1_pairstep import A, TOL_E, TOL_G, TOL_KNOB, ao_sizes, assert_fused, bundle, record

pytestmark = pytest.mark.gpu
T = 2
K = 3   # distinct geometries per orbital count
FUSED_Y2 = "y2d_kernel<1> pairstep"

_inputs = {}


def inputs(n):
    """t-RDMs and K AO problems of a size, made once."""
    if n not in _inputs:
        S, one, two = make_trdms(n, T, 300 + n)
        _inputs[n] = (S, one, pack_rows(two, True, True),
                      [make_ao_arrays(n, A, 900 + 10 * n + k, ao_sizes=ao_sizes(n), ip1_rs_symmetric=True) for k in range(K)])
    return _inputs[n]


_oracle = {}
_oracle_dir = None   # the child process of test_knobs_off_every_size reads the parent's values from here


def oracle(n):
    """E (K,), grad (K, A, 3) of the K geometries from the oracle on the original packed t-RDMs, computed once."""
    if n not in _oracle:
        if _oracle_dir:
            with np.load(os.path.join(_oracle_dir, f"oracle_{n}.npz")) as z:
                _oracle[n] = (z["E"], z["g"])
        else:
            S, one, two_l, aos = inputs(n)
            res = [orc.energy_with_grad(bundle(a), one, two_l, S, return_density_matrices=n in KEEP_SIZES) for a in aos]
            _oracle[n] = (np.array([r[0] for r in res]), np.array([r[1] for r in res]))
            if n in KEEP_SIZES:
                _gamma8[n] = [sym8(np.asarray(r[3]), n) for r in res]
    return _oracle[n]


_gamma8 = {}


def sym8(G, n):
    """The 8-fold symmetrised 2-RDM, as tests/test_gpu_y2_pairstep.py::test_unpacked_two_rdm_requested."""
    s8 = G.reshape(n, n, n, n)
    s8 = s8 + np.swapaxes(s8, 0, 1)
    s8 = s8 + np.swapaxes(s8, 2, 3)
    return (s8 + np.moveaxis(s8, (2, 3), (0, 1))) / 8.0


_device = {}


def device(n):
    """The uploaded t-RDMs and the K uploaded geometries of a size (the last size asked for is kept)."""
    if n not in _device:
        from evcont_amd.evaluator import DeviceAO, DeviceTRDMs
        _device.clear()
        dev = torch.device("cuda:0")
        S, one, two_l, aos = inputs(n)
        _device[n] = (DeviceTRDMs(one, two_l, S, dev, compress="sym8"),
                      [DeviceAO.from_arrays(a, dev, pack_ip1=True, pack_eri=True) for a in aos])
    return _device[n]


def run(n, G, keep=False):
    """One batched call on G slots, geometry s % K in slot s."""
    from evcont_amd.evaluator import BatchedEvaluator, DeviceAOBatch
    trd, daos = device(n)
    be = BatchedEvaluator(trd, A, G, keep_density_matrices=keep)
    aob = DeviceAOBatch.stack([daos[s % K] for s in range(G)])
    E, g = be.energies_with_grads(aob)
    assert E.shape == (G,) and g.shape == (G, A, 3)
    return be, aob, E, g


def check_oracle(route, n, G, E, g):
    """Every slot against the oracle of its geometry."""
    Eo, go = oracle(n)
    idx = np.arange(G) % K
    de = np.abs(E - Eo[idx])
    dg = np.abs(g - go[idx]).reshape(G, -1).max(axis=1)
    print(f"pair_dma_sweep: route={route} n={n} G={G}: max|dE|={de.max():.2e} (slot {int(de.argmax())}) "
          f"max|dgrad|={dg.max():.2e} (slot {int(dg.argmax())}) max|grad|={np.abs(go).max():.2f}")
    assert de.max() < TOL_E, (route, n, G, int(de.argmax()), float(de.max()))
    assert dg.max() <= TOL_G, (route, n, G, int(dg.argmax()), float(dg.max()))


_fused_g4 = {}


def fused_case(n, G):
    be, aob, E, g = run(n, G)
    assert_fused()
    assert record("y2") == FUSED_Y2, record("y2")
    check_oracle("fused", n, G, E, g)
    E2, g2 = be.energies_with_grads(aob)
    same = [bool(np.array_equal(E[s], E2[s]) and np.array_equal(g[s], g2[s])) for s in range(G)]
    assert all(same), (n, G, "slots that differ between two calls:", [s for s in range(G) if not same[s]],
                       float(np.abs(g - g2).max()))
    if G == 4:
        _fused_g4[n] = g
    return g


def fused_forces_g4(n):
    if n not in _fused_g4:
        fused_case(n, 4)
    return _fused_g4[n]


@pytest.mark.parametrize("n,G", SWEEP)
def test_fused_route_every_size(n, G):
    fused_case(n, G)


@pytest.mark.parametrize("n,G", BOUNDARY)
def test_batch_size_boundaries(n, G):
    fused_case(n, G)


def test_knobs_off_every_size(tmp_path):
    """Both knobs off (read once per process: a fresh interpreter): the storing ptd_kernel<0> twice with its counted
    waits, the separate y2d_kernel, the pair blocks of ip1_dh_kernel.  The child holds every slot to the oracle and
    asserts the unfused records; its forces agree with the default route's within 1e-10."""
    out = str(tmp_path)
    for n, _ in KNOBS_OFF:
        Eo, go = oracle(n)
        np.savez(os.path.join(out, f"oracle_{n}.npz"), E=Eo, g=go)
    e = {**os.environ, "EVC_Y2_PAIRSTEP": "0", "EVC_IP1_PAIRSTEP": "0"}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], cwd=REPO, env=e, capture_output=True, text=True,
                       timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    diff = {}
    for n, G in KNOBS_OFF:
        diff[n] = float(np.abs(fused_forces_g4(n) - np.load(os.path.join(out, f"g_{n}_{G}.npy"))).max())
        print(f"pair_dma_sweep: n={n} G={G}: max|grad(fused) - grad(knobs off)|={diff[n]:.2e}")
    print(f"pair_dma_sweep: worst fused against knobs off: {max(diff.values()):.2e}")
    assert all(d <= TOL_KNOB for d in diff.values()), {n: d for n, d in diff.items() if not d <= TOL_KNOB}


@pytest.mark.parametrize("n", KEEP_SIZES)
def test_unpacked_two_rdm_requested_sizes(n):
    """With the unpacked 2-RDM requested y2d_kernel<1> runs over the second unpack and the storing ptd_kernel<0> is the
    second step; forces and the 2-RDM of every slot against the oracle."""
    G = 4
    be, aob, E, g = run(n, G, keep=True)
    assert record("y2") == FUSED_Y2, record("y2")
    assert_fused(False)
    assert record("pair_transform") == "ptd_kernel<0>", record("pair_transform")
    check_oracle("keep", n, G, E, g)
    d = [float(np.abs(be.g_pred[s].cpu().numpy() - _gamma8[n][s % K]).max()) for s in range(G)]
    print(f"pair_dma_sweep: route=keep n={n} G={G}: max|d2RDM|={max(d):.2e} (slot {int(np.argmax(d))})")
    assert max(d) <= 1e-10, (n, d)


@pytest.mark.parametrize("n", ROOTS_SIZES)
def test_multi_slot_roots_sizes(n):
    """evc_phase_gradient_roots_batch, 2 roots of 2 geometries, all pairs: 6 slots with geo_period set -- Y2 inside the
    first step, the second one storing, ip1_dh_kernel's multi-slot form behind it."""
    from test_gpu_excited_forces import Oracle, all_pairs
    from test_gpu_excited_forces_batch import check_batch, device_inputs, host_case, _evs
    Tr, Ar, nroots, G = 3, 3, 2, 2
    S, one, two_l, aos = host_case(n, Tr, Ar, 300 + n, (7000 + 10 * n, 7001 + 10 * n), "sym8_packed")
    oracles = [Oracle(a, one, two_l, S, nroots) for a in aos]
    trd, daos, aob = device_inputs("sym8_packed", S, one, two_l, aos, Ar)
    check_batch(_evs(trd, Ar, G), aob, oracles, nroots, all_pairs(nroots))
    pt, ip1 = record("pair_transform"), record("ip1")
    assert record("y2").startswith("y2d_kernel<1>"), record("y2")
    assert pt.startswith("ptd_kernel<0>") and "+ip1" not in pt, pt
    assert "slots=2" in ip1, ip1


if __name__ == "__main__":   # the knobs-off leg of test_knobs_off_every_size: oracle values from, forces into argv[1]
    assert os.environ.get("EVC_Y2_PAIRSTEP") == "0" and os.environ.get("EVC_IP1_PAIRSTEP") == "0"
    _oracle_dir = sys.argv[1]
    failed_ = []   # (every size runs: the parent sees all that are outside the bounds, not the first)
    for n_, G_ in KNOBS_OFF:
        _, _, E_, g_ = run(n_, G_)
        pt_, y2_, ip1_ = record("pair_transform"), record("y2"), record("ip1")
        assert pt_ == "ptd_kernel<0>", pt_
        assert y2_.startswith("y2d_kernel") and not y2_.startswith("y2d_kernel<1>"), y2_
        assert ip1_.startswith("ip1_dh_kernel<8> pairs") and "dot in ptd" not in ip1_, ip1_
        np.save(os.path.join(sys.argv[1], f"g_{n_}_{G_}.npy"), g_)
        try:
            check_oracle("knobs-off", n_, G_, E_, g_)
        except AssertionError as err_:
            failed_.append(err_.args[0])
    assert not failed_, failed_
