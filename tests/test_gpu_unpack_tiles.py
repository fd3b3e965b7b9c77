"""GPU tests of the mirrored-tile unpack of the predicted 2-RDM (csrc/unpack_tiles.hpp: the unpack blocks of
unpack8_prep_kernel, one 64 x 32 tile of the lower triangle of the (pair, pair) matrix per workgroup), through the public
path only: BatchedEvaluator.energies_with_grads on compress="sym8" training data with packed s4 / s2kl integrals, A = 2.

Shapes (N, G), chosen for where the tiling can go wrong, not for the workload: npairs = 3 (far below a tile), 28 (just
below 32 columns), 36 (a full column block and a sliver; G = 9: eight interleaved geometries and the remainder path),
55 / 66, 120 / 136 and 190 (N = 10, 11, 15, 16, 19: the pair counts next to the multiples 64, 128 and 192 of a tile's rows;
N = 16 is also the size at which the pt_pipe / y2_fused route reads SB), 153 (first size of the fused y2d_kernel<1>
route), 253 (8 x 32 - 3), 276, 465 (the workload's N: 71 tiles per geometry).  T = 3 below N = 22, T = 2 from there on.

Check 1: every slot's energy and forces against oracle/evcont_oracle.py on the original packed t-RDMs, |dE| < 1e-9 and
|dgrad| <= 1e-8 (the bounds of tests/test_gpu_pair_dma_sweep.py for the same quantities).  Check 2: a second call on the
same inputs is bit-identical (a wrong edge or a race in the LDS transpose shows as noise first).  Slot s holds geometry
s % 3; the oracle values of a size are computed once.

K8 with few rows: T = 2, G = 17 with EVC_ROWS_LDS_MINCOLS=1 in a fresh interpreter (the knob is read once per process)
reaches gemv_cols_lds_kernel with three matrix rows: two pieces per tile against eleven ring slots to fill, so the
prologue's re-read branch runs, and most waves of the one-body blocks have no tile at all; the same two checks.
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
from test_gpu_ip1_pairstep import TOL_E, TOL_G, bundle, record

pytestmark = pytest.mark.gpu
A = 2
K = 3   # distinct geometries per size
CASES = [(2, 1), (7, 3), (8, 9), (10, 2), (11, 2), (15, 2), (16, 4), (17, 4), (19, 2), (22, 8), (23, 5), (30, 9)]
K8_CASE = (8, 17)


_host = {}


def host(n, T):
    """t-RDMs, K AO problems and their oracle (E (K,), grad (K, A, 3)) of a size, made once."""
    if n not in _host:
        S, one, two = make_trdms(n, T, 300 + n)
        two_l = pack_rows(two, True, True)
        aos = [make_ao_arrays(n, A, 4100 + 10 * n + k, ip1_rs_symmetric=True) for k in range(K)]
        res = [orc.energy_with_grad(bundle(a), one, two_l, S) for a in aos]
        _host[n] = (S, one, two_l, aos, np.array([r[0] for r in res]), np.array([r[1] for r in res]))
    return _host[n]


def run_case(n, G, T):
    """Both checks on one batch of G slots; returns the record of the K8 stage."""
    from evcont_amd.evaluator import BatchedEvaluator, DeviceAO, DeviceAOBatch, DeviceTRDMs
    dev = torch.device("cuda:0")
    S, one, two_l, aos, Eo, go = host(n, T)
    trd = DeviceTRDMs(one, two_l, S, dev, compress="sym8")
    daos = [DeviceAO.from_arrays(a, dev, pack_ip1=True, pack_eri=True) for a in aos]
    be = BatchedEvaluator(trd, A, G)
    aob = DeviceAOBatch.stack([daos[s % K] for s in range(G)])
    E, g = be.energies_with_grads(aob)
    assert E.shape == (G,) and g.shape == (G, A, 3)
    assert record("unpack") == "unpack8_prep_kernel", record("unpack")
    k8 = record("k8_cols")
    idx = np.arange(G) % K
    de = np.abs(E - Eo[idx])
    dg = np.abs(g - go[idx]).reshape(G, -1).max(axis=1)
    print(f"unpack_tiles: n={n} G={G} k8={k8}: max|dE|={de.max():.2e} (slot {int(de.argmax())}) "
          f"max|dgrad|={dg.max():.2e} (slot {int(dg.argmax())})")
    assert de.max() < TOL_E, (n, G, int(de.argmax()), float(de.max()))
    assert dg.max() <= TOL_G, (n, G, int(dg.argmax()), float(dg.max()))
    E2, g2 = be.energies_with_grads(aob)
    assert np.array_equal(E, E2) and np.array_equal(g, g2), (n, G, float(np.abs(g - g2).max()))
    return k8


@pytest.mark.parametrize("n,G", CASES)
def test_every_slot_against_oracle_and_repeatable(n, G):
    run_case(n, G, 3 if n < 22 else 2)


def test_k8_few_rows_fewer_pieces_than_ring_slots():
    e = {**os.environ, "EVC_ROWS_LDS_MINCOLS": "1"}
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=REPO, env=e, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


if __name__ == "__main__":   # the child of test_k8_few_rows_fewer_pieces_than_ring_slots
    assert os.environ.get("EVC_ROWS_LDS_MINCOLS") == "1"
    k8_ = run_case(*K8_CASE, 2)
    assert k8_.startswith("gemv_cols_lds_kernel"), k8_
