"""Several evaluators on several torch streams at once, sharing one ``DeviceTRDMs``, as ``bench.py: measure`` runs them
(``--streams 3``): 2 S calls enqueued round-robin with no synchronisation in between, each call's outputs cloned on its
evaluator's stream before that evaluator is enqueued again, then compared slot by slot with the same calls run one at a
time on one stream.

The comparison is bitwise: both runs launch the same kernels on the same inputs, and every sum in them has a fixed
order (no atomics, no split depending on timing), so a difference can only come from one call reading or overwriting
another's buffers -- a missing stream or event dependency.  Kernel names are not asserted here: the record of
``evc_profile_kernel`` is process-wide and means nothing while calls run concurrently."""
import pytest
import torch

from evcont_amd.synthetic import make_device_ao, make_device_trdm_rows

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _trdms(n, T, seed):
    from evcont_amd.evaluator import DeviceTRDMs
    S, one, rows = make_device_trdm_rows(n, T, 2, seed, DEV)
    trd = DeviceTRDMs.from_device_rows(one, rows, S, 2)
    del rows
    return trd.compress_sym8_()


def _batches(n, A, G, nb, seed):
    """nb batches of G packed geometries (s4 / s2kl), built from 2 G distinct ones in bench.py's cyclic order."""
    from evcont_amd.evaluator import DeviceAOBatch
    aos = [make_device_ao(n, A, seed + k, DEV, ip1_rs_symmetric=True).packed_ip1(eri=True) for k in range(2 * G)]
    if G == 1:
        return [aos[i % len(aos)] for i in range(nb)]
    return [DeviceAOBatch.stack([aos[(i * G + j) % len(aos)] for j in range(G)]) for i in range(nb)]


def _outputs(ev, energy_only):
    return (ev.energy.clone(), None if energy_only else ev.grad.clone())


def _concurrent(evs, calls):
    """calls: (evaluator index, input, energy_only), enqueued in order without synchronisation; the outputs of each are
    cloned on its evaluator's stream right behind it."""
    out = []
    for i, x, eo in calls:
        ev = evs[i]
        ev.enqueue(x, 1, eo)
        with torch.cuda.stream(ev.stream):
            out.append(_outputs(ev, eo))
    torch.cuda.synchronize(DEV)
    return out


def _serial(ev, calls):
    out = []
    for _, x, eo in calls:
        ev.enqueue(x, 1, eo)
        ev.synchronize()
        out.append(_outputs(ev, eo))
    return out


def _assert_bitwise(got, want):
    assert len(got) == len(want)
    for k, ((e, g), (e0, g0)) in enumerate(zip(got, want)):
        assert torch.equal(e, e0), (k, float((e - e0).abs().max()))
        if g0 is not None:
            assert torch.equal(g, g0), (k, float((g - g0).abs().max()))


def _batched_case(n, A, T, G, S, seed):
    from evcont_amd.evaluator import BatchedEvaluator
    trd = _trdms(n, T, seed)
    xs = _batches(n, A, G, 2 * S, seed * 1000)
    calls = [(i % S, xs[i], False) for i in range(2 * S)]
    evs = [BatchedEvaluator(trd, A, G, stream=torch.cuda.Stream(DEV)) for _ in range(S)]
    got = _concurrent(evs, calls)
    want = _serial(BatchedEvaluator(trd, A, G), calls)
    _assert_bitwise(got, want)


def test_h30_three_streams_bitwise():
    """The figure of record: H30 (N=30, A=30, T=20), sym8 with packed inputs, 32 geometries per call, three streams."""
    _batched_case(30, 30, 20, 32, 3, 1234)


def test_n58_side_stream_three_workspaces_bitwise():
    """N=58, 4 geometries per call: every call forks its eigensolver onto the device's ONE side stream, three
    workspaces at once."""
    _batched_case(58, 3, 8, 4, 3, 1240)


def test_n40_md_regime_three_streams_bitwise():
    """One geometry per call through ContinuationEvaluator (the MD regime), N=40 (side-stream Loewdin step), three
    streams."""
    from evcont_amd.evaluator import ContinuationEvaluator
    n, A, T, S = 40, 2, 6, 3
    trd = _trdms(n, T, 4040)
    xs = _batches(n, A, 1, 2 * S, 4040000)
    calls = [(i % S, xs[i], False) for i in range(2 * S)]
    evs = [ContinuationEvaluator(trd, A, stream=torch.cuda.Stream(DEV), want_two_rdm=False) for _ in range(S)]
    got = _concurrent(evs, calls)
    want = _serial(ContinuationEvaluator(trd, A, want_two_rdm=False), calls)
    _assert_bitwise(got, want)


def test_n40_energy_only_beside_full_calls_bitwise():
    """Energy-only calls on one stream while full calls run on two others, N=40, 2 geometries per call: the energy-only
    calls also fork their eigensolver onto the side stream (and are joined by nothing of their own)."""
    from evcont_amd.evaluator import BatchedEvaluator
    n, A, T, G = 40, 2, 6, 2
    trd = _trdms(n, T, 4141)
    xs = _batches(n, A, G, 6, 4141000)
    calls = [(0, xs[0], True), (1, xs[1], False), (2, xs[2], False), (0, xs[3], True), (1, xs[4], False),
             (0, xs[5], True), (2, xs[0], False)]
    evs = [BatchedEvaluator(trd, A, G, stream=torch.cuda.Stream(DEV)) for _ in range(3)]
    got = _concurrent(evs, calls)
    want = _serial(BatchedEvaluator(trd, A, G), calls)
    _assert_bitwise(got, want)
