"""GPU tests of the Y2 contraction inside the first gradient-side pair step (csrc/pair_dma.hip y2d_kernel<1>,
knob EVC_Y2_PAIRSTEP): 17 <= N <= 30, the compressed layout with packed s4 / s2kl integrals, at least 4
slots per launch.

Shapes: N = 17 (153 pairs: the smallest shape, one live row in the second 16-row tile, a ragged last tile), N = 23 (276
pairs, odd row starts), N = 30 (465 pairs: the benchmark's shape, the largest row, a ragged last tile); G = 4 and 5
geometries (the smallest batches of this route, an even and an odd count).  The first and the last geometry of every
batch are held to the oracle on the original t-RDMs, |dE| < 1e-9 and |dgrad| <= 1e-8 as the neighbouring batched tests
(tests/test_gpu_sym8.py); the two settings of the knob are held to each other within the same bound on every geometry.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dispatch_table import knob_row
from evcont_amd.synthetic import make_ao_arrays, make_trdms, pack_rows
from oracle import evcont_oracle as orc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(17, 3), (23, 2), (30, 2)]
COUNTS = [4, 5]
A = 3
TOL_E, TOL_G = 1e-9, 1e-8


def bundle(a):
    return orc.AOBundle(a.S, a.hcore, a.eri, a.ipovlp, a.dhcore, a.eri_ip1, a.aoslices, a.enuc, a.gnuc)


def y2_record():
    from evcont_amd import _lib
    return _lib.load().evc_profile_kernel(_lib.PROF_STAGES["y2"]).decode()


def pt_record():
    from evcont_amd import _lib
    return _lib.load().evc_profile_kernel(_lib.PROF_STAGES["pair_transform"]).decode()


_inputs = {}


def inputs(n, T):
    """t-RDMs and five AO problems of a shape, made once."""
    if (n, T) not in _inputs:
        S, one, two = make_trdms(n, T, 300 + n)
        _inputs[n, T] = (S, one, pack_rows(two, True, True),
                         [make_ao_arrays(n, A, 700 + 10 * n + k, ip1_rs_symmetric=True) for k in range(max(COUNTS))])
    return _inputs[n, T]


_oracle = {}


def oracle(n, T, k):
    """(E, grad) of geometry k from the oracle on the original packed t-RDMs, computed once."""
    if (n, T, k) not in _oracle:
        S, one, two_l, aos = inputs(n, T)
        _oracle[n, T, k] = orc.energy_with_grad(bundle(aos[k]), one, two_l, S)
    return _oracle[n, T, k]


def run_batch(n, T, G, keep=False):
    from evcont_amd.evaluator import DeviceTRDMs, DeviceAOBatch, BatchedEvaluator
    dev = torch.device("cuda:0")
    S, one, two_l, aos = inputs(n, T)
    trd = DeviceTRDMs(one, two_l, S, dev, compress="sym8")
    be = BatchedEvaluator(trd, A, G, keep_density_matrices=keep)
    E, g = be.energies_with_grads(DeviceAOBatch.from_arrays(aos[:G], dev, pack_ip1=True, pack_eri=True))
    return E, g, be


def check_oracle(n, T, G, E, g):
    for k in (0, G - 1):
        Eo, go = oracle(n, T, k)
        de, dg = abs(E[k] - Eo), float(np.abs(g[k] - go).max())
        print(f"n={n} G={G} geometry {k}: |dE|={de:.2e} max|dgrad|={dg:.2e}")
        assert de < TOL_E, (n, G, k, de)
        assert dg <= TOL_G, (n, G, k, dg)


def expected_y2_record():
    return "y2d_kernel" if os.environ.get("EVC_Y2_PAIRSTEP") == "0" else "y2d_kernel<1>"


@pytest.mark.parametrize("G", COUNTS)
@pytest.mark.parametrize("n,T", SHAPES)
def test_batch_against_oracle(n, T, G):
    E, g, _ = run_batch(n, T, G)
    rec = y2_record()
    assert rec.startswith(expected_y2_record()), rec
    if os.environ.get("EVC_Y2_PAIRSTEP") == "0":
        assert not rec.startswith("y2d_kernel<1>"), rec
        # the whole records of the knob's dispatch-table row: Y2 alone, the int2e_ip1 dot still in the second step
        want = knob_row("knob_y2_pairstep_off")["expect"]
        assert (rec, pt_record()) == (want["y2"], want["pair_transform"]), (rec, pt_record())
    assert pt_record().startswith("ptd_kernel<0>"), pt_record()
    check_oracle(n, T, G, E, g)
    out = os.environ.get("EVC_Y2_PAIRSTEP_DUMP")
    if out:   # (the child of test_knob_off_agrees hands its forces to the parent)
        np.save(os.path.join(out, f"g_{n}_{G}.npy"), g)


def test_knob_off_agrees(tmp_path):
    """EVC_Y2_PAIRSTEP=0 (read once per process: a fresh interpreter) runs Y2 and the pair step as two kernels; the
    same cases pass there, the Y2 stage reports the separate y2d_kernel, and its forces agree with the default's."""
    e = dict(os.environ)
    e.update({"EVC_Y2_PAIRSTEP": "0", "EVC_Y2_PAIRSTEP_DUMP": str(tmp_path)})
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_y2_pairstep.py::test_batch_against_oracle"],
                       cwd=REPO, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    for n, T in SHAPES:
        for G in COUNTS:
            _, g, _ = run_batch(n, T, G)
            assert y2_record().startswith("y2d_kernel<1>"), y2_record()
            d = float(np.abs(g - np.load(os.path.join(str(tmp_path), f"g_{n}_{G}.npy"))).max())
            print(f"n={n} G={G}: max|grad(on) - grad(off)|={d:.2e}")
            assert d <= TOL_G, (n, G, d)


def test_multi_root_slots():
    """evc_phase_gradient_roots_batch, 2 roots of 2 geometries: 4 slots with geo_period set (SB per slot; X and the
    first step's intermediate per geometry), against the host reference of tests/test_gpu_excited_forces_batch.py."""
    from test_gpu_excited_forces import Oracle
    from test_gpu_excited_forces_batch import check_batch, device_inputs, host_case, _evs
    n, T, nroots, G = 17, 3, 2, 2
    S, one, two_l, aos = host_case(n, T, A, 317, (7170, 7171), "sym8_packed")
    oracles = [Oracle(a, one, two_l, S, nroots) for a in aos]
    trd, daos, aob = device_inputs("sym8_packed", S, one, two_l, aos, A)
    check_batch(_evs(trd, A, G), aob, oracles, nroots, None)
    assert y2_record().startswith("y2d_kernel<1>"), y2_record()


def test_unpacked_two_rdm_requested():
    """With the unpacked 2-RDM requested the dense (pair, pair) SB is unpacked a second time, over the N^4-addressed
    one; energies, forces and the 2-RDM itself against the oracle."""
    n, T, G = 17, 3, 4
    E, g, be = run_batch(n, T, G, keep=True)
    assert y2_record().startswith("y2d_kernel<1>"), y2_record()
    check_oracle(n, T, G, E, g)
    S, one, two_l, aos = inputs(n, T)
    Go = np.asarray(orc.energy_with_grad(bundle(aos[G - 1]), one, two_l, S, return_density_matrices=True)[3])
    s8 = Go.reshape(n, n, n, n)
    s8 = s8 + np.swapaxes(s8, 0, 1)
    s8 = s8 + np.swapaxes(s8, 2, 3)
    s8 = (s8 + np.moveaxis(s8, (2, 3), (0, 1))) / 8.0
    np.testing.assert_allclose(be.g_pred[G - 1].cpu().numpy(), s8, rtol=0, atol=1e-10)
