"""GPU tests of the int2e_ip1 contraction inside the second gradient-side pair step (csrc/pair_dma.hip ptd_kernel<0, 1>,
knob EVC_IP1_PAIRSTEP): 17 <= N <= 30, the compressed layout with packed s4 / s2kl integrals, at least 4
slots per launch, one slot per geometry, the unpacked 2-RDM not requested.

Shapes: N = 17 (153 pairs: the smallest shape, three write-out passes, the last one ragged), N = 23 (276 pairs: operand
rows on odd 8-byte offsets, a ragged last tile of pairs, a partly empty last pass), N = 30 (465 pairs: the benchmark's
shape, all eight passes, one live pair in the last tile); T = 3; G = 4 (the fewest slots of the route), 5 and 9 (the Y2
pair step in front cuts its grid differently from 8 slots on).  Four atoms with AO blocks of unequal size (N - 7, 2, 2,
3): the per-orbital sums of the contraction land in different atoms.  The first and the last geometry of every batch
are held to the oracle, |dE| < 1e-9 and |dgrad| <= 1e-8 as the neighbouring small-shape tests; every geometry's forces
to those of a fresh process with EVC_IP1_PAIRSTEP=0 within 1e-10 (the sums run in another order).
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

from dispatch_table import knob_row
from evcont_amd.synthetic import make_ao_arrays, make_trdms, pack_rows
from oracle import evcont_oracle as orc

pytestmark = pytest.mark.gpu
T = 3
SIZES = [17, 23, 30]
COUNTS = [4, 5, 9]
A = 4
TOL_E, TOL_G, TOL_KNOB = 1e-9, 1e-8, 1e-10
FUSED_PT, FUSED_IP1 = "ptd_kernel<0> +ip1", "ip1_dh_kernel<8> pairs (dot in ptd)"


def ao_sizes(n):
    return (n - 7, 2, 2, 3)


def bundle(a):
    return orc.AOBundle(a.S, a.hcore, a.eri, a.ipovlp, a.dhcore, a.eri_ip1, a.aoslices, a.enuc, a.gnuc)


def record(stage):
    from evcont_amd import _lib
    return _lib.load().evc_profile_kernel(_lib.PROF_STAGES[stage]).decode()


def assert_fused(fused=True):
    pt, ip1 = record("pair_transform"), record("ip1")
    if fused:
        assert pt.startswith(FUSED_PT), pt
        assert ip1.startswith(FUSED_IP1), ip1
    else:
        assert "+ip1" not in pt, pt
        assert "dot in ptd" not in ip1, ip1


_inputs = {}


def inputs(n):
    """t-RDMs and nine AO problems of a size, made once."""
    if n not in _inputs:
        S, one, two = make_trdms(n, T, 300 + n)
        _inputs[n] = (S, one, pack_rows(two, True, True),
                      [make_ao_arrays(n, A, 900 + 10 * n + k, ao_sizes=ao_sizes(n), ip1_rs_symmetric=True)
                       for k in range(max(COUNTS))])
    return _inputs[n]


_oracle = {}


def oracle(n, k):
    """(E, grad) of geometry k from the oracle on the original packed t-RDMs, computed once."""
    if (n, k) not in _oracle:
        S, one, two_l, aos = inputs(n)
        _oracle[n, k] = orc.energy_with_grad(bundle(aos[k]), one, two_l, S)
    return _oracle[n, k]


def evaluator(n, G, keep=False):
    from evcont_amd.evaluator import DeviceTRDMs, DeviceAOBatch, BatchedEvaluator
    dev = torch.device("cuda:0")
    S, one, two_l, aos = inputs(n)
    trd = DeviceTRDMs(one, two_l, S, dev, compress="sym8")
    be = BatchedEvaluator(trd, A, G, keep_density_matrices=keep)
    return be, DeviceAOBatch.from_arrays(aos[:G], dev, pack_ip1=True, pack_eri=True)


def run_batch(n, G, keep=False):
    be, aob = evaluator(n, G, keep)
    E, g = be.energies_with_grads(aob)
    return E, g


def check_oracle(n, G, E, g):
    for k in (0, G - 1):
        Eo, go = oracle(n, k)
        de, dg = abs(E[k] - Eo), float(np.abs(g[k] - go).max())
        print(f"n={n} G={G} geometry {k}: |dE|={de:.2e} max|dgrad|={dg:.2e}")
        assert de < TOL_E, (n, G, k, de)
        assert dg <= TOL_G, (n, G, k, dg)


_knob_off = {}


def knob_off_forces(tmp_path_factory):
    """Forces of every (N, G) from a fresh interpreter with EVC_IP1_PAIRSTEP=0 (the knob is read once per process),
    which also asserts that its records do not name the fused route; run once."""
    if not _knob_off:
        out = str(tmp_path_factory.mktemp("ip1_pairstep_off"))
        e = {**os.environ, "EVC_IP1_PAIRSTEP": "0"}
        r = subprocess.run([sys.executable, os.path.abspath(__file__), out], cwd=REPO, env=e, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        for n in SIZES:
            for G in COUNTS:
                _knob_off[n, G] = np.load(os.path.join(out, f"g_{n}_{G}.npy"))
    return _knob_off


@pytest.mark.parametrize("G", COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_batch_against_oracle_and_knob_off(n, G, tmp_path_factory):
    E, g = run_batch(n, G)
    assert_fused()
    check_oracle(n, G, E, g)
    d = float(np.abs(g - knob_off_forces(tmp_path_factory)[n, G]).max())
    print(f"n={n} G={G}: max|grad(on) - grad(off)|={d:.2e}")
    assert d <= TOL_KNOB, (n, G, d)


def test_gradient_phase_after_energy_only():
    """evc_phase_gradient on the workspace of an energy-only call takes the fused route and matches the oracle."""
    n, G = 23, 5
    be, aob = evaluator(n, G)
    be.enqueue(aob, 1, energy_only=True)
    be.synchronize()
    assert_fused(False)
    be.phase_gradient(aob, partial_rank=False)
    be.synchronize()
    assert_fused()
    check_oracle(n, G, be.energy[:, 0].cpu().numpy(), be.grad[:, :A].cpu().numpy())


def test_unpacked_two_rdm_requested_keeps_the_separate_dot():
    n, G = 17, 4
    be, aob = evaluator(n, G, keep=True)
    E, g = be.energies_with_grads(aob)
    assert_fused(False)
    assert record("pair_transform").startswith("ptd_kernel<0>"), record("pair_transform")
    check_oracle(n, G, E, g)


def test_sixteen_orbitals_keep_the_separate_dot():
    n, G = 16, 4
    S, one, two = make_trdms(n, T, 300 + n)
    two_l = pack_rows(two, True, True)
    aos = [make_ao_arrays(n, A, 900 + 10 * n + k, ao_sizes=ao_sizes(n), ip1_rs_symmetric=True) for k in range(G)]
    _inputs[n] = (S, one, two_l, aos)
    E, g = run_batch(n, G)
    assert_fused(False)
    check_oracle(n, G, E, g)


def test_multi_slot_roots_call_keeps_the_separate_dot():
    """evc_phase_gradient_roots_batch, 2 roots of 2 geometries: 4 slots, two per geometry -- ip1_dh_kernel's multi-slot
    form reads the int2e_ip1 rows once for both."""
    from test_gpu_excited_forces import Oracle
    from test_gpu_excited_forces_batch import check_batch, device_inputs, host_case, _evs
    n, nroots, G = 17, 2, 2
    S, one, two_l, aos = host_case(n, T, 3, 317, (7170, 7171), "sym8_packed")
    oracles = [Oracle(a, one, two_l, S, nroots) for a in aos]
    trd, daos, aob = device_inputs("sym8_packed", S, one, two_l, aos, 3)
    check_batch(_evs(trd, 3, G), aob, oracles, nroots, None)
    assert_fused(False)
    assert record("pair_transform").startswith("ptd_kernel<0>"), record("pair_transform")
    assert "slots=" in record("ip1"), record("ip1")


if __name__ == "__main__":   # the EVC_IP1_PAIRSTEP=0 leg of test_batch_against_oracle_and_knob_off: forces into argv[1]
    assert os.environ.get("EVC_IP1_PAIRSTEP") == "0"
    for n_ in SIZES:
        for G_ in COUNTS:
            E_, g_ = run_batch(n_, G_)
            assert_fused(False)
            assert record("pair_transform").startswith("ptd_kernel<0>"), record("pair_transform")
            assert record("ip1").startswith("ip1_dh_kernel<8> pairs"), record("ip1")
            # the whole records of the knob's dispatch-table row: the storing second step, Y2 still in the first
            want_ = knob_row("knob_ip1_pairstep_off")["expect"]
            for stage_ in ("pair_transform", "ip1", "y2"):
                assert record(stage_) == want_[stage_], (stage_, record(stage_))
            np.save(os.path.join(sys.argv[1], f"g_{n_}_{G_}.npy"), g_)
