"""Pair sharding emulated on one device, for tests: one evaluator per row range of the two-body t-RDM, the three phase
calls on each, and the two collectives of ``distributed.PairShardedContinuation`` replaced by what they compute -- the
(G, chunk) send buffers of the ranks stacked as ``all_gather_into_tensor`` stacks them and permuted to (G, world * chunk),
the partial gradients (and predicted 2-RDMs) summed.  The loop of
``tests/test_gpu_batch.py::test_batched_phase_api_emulated_pair_sharding`` for arbitrary cut points, empty ranges
included, with the outputs of phase C filled with NaN beforehand and the K5 / K8 / subspace kernel records of every rank
read back.  A plain module (as ``dispatch_table.py`` is); ``tests/test_gpu_shard_routes.py`` holds the cases."""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from evcont_amd import _lib


@dataclass
class ShardedRun:
    ranges: list                      # [(r0, r1)] per rank
    energy: List[np.ndarray]          # per rank (G, T): the roots the solve was asked for lead every row
    grad_rank: List[np.ndarray]       # per rank (G, A, 3), the partial gradients
    grad: np.ndarray                  # their sum
    d_pred: List[Optional[np.ndarray]] = field(default_factory=list)   # per rank (G, n, n), None where not kept
    g_pred_rank: List[Optional[np.ndarray]] = field(default_factory=list)   # per rank (G, n, n, n, n)
    g_pred: Optional[np.ndarray] = None                                # their sum
    records: List[dict] = field(default_factory=list)    # per rank {"k5_rows", "k8_cols", "subspace"}
    plans: List[str] = field(default_factory=list)       # per rank evc_trdm_plan_describe on this device


def _record(stage):
    return _lib.load().evc_profile_kernel(_lib.PROF_STAGES[stage]).decode()


def describe(trdm_set, count, cus=0):
    """``evc_trdm_plan_describe``: the K5 / K8 passes of ``count`` geometries on this set (cus = 0: the current device)."""
    import ctypes as C
    lib = _lib.load()
    buf = C.create_string_buffer(1 << 16)
    n = lib.evc_trdm_plan_describe(C.byref(trdm_set), count, cus, buf, len(buf))
    assert 0 <= n < len(buf), lib.evc_last_error()
    return buf.value.decode()


def check_ranges(ranges, rows_total):
    """The ranges tile [0, rows_total) in order (empty ones anywhere)."""
    at = 0
    for r0, r1 in ranges:
        assert r0 == at and r0 <= r1 <= rows_total, (ranges, rows_total)
        at = r1
    assert at == rows_total, (ranges, rows_total)


def run_sharded(one, two, S, ranges, aos, natm, device, compress=None, rows_layout=None, keep=False, nroots=1):
    """``two``: the two-body t-RDMs in a layout of the reference (host array: every rank uploads its ``row_range``), or,
    with ``rows_layout``, the (rows, cols) matrix of that layout on the device (every rank adopts its slice through
    ``from_device_rows(row_offset=...)``).  ``compress``: None or "sym8".  ``aos``: the geometries as ``DeviceAO``; one of
    them runs on a ``ContinuationEvaluator``, several on a ``BatchedEvaluator``.  ``keep``: the predicted RDMs are
    outputs."""
    from evcont_amd.evaluator import (BatchedEvaluator, ContinuationEvaluator, DeviceAOBatch, DeviceTRDMs)
    G = len(aos)
    single = G == 1
    geo = aos[0] if single else DeviceAOBatch.stack(aos)
    world = len(ranges)
    evs = []
    for r0, r1 in ranges:
        if rows_layout is not None:
            trd = DeviceTRDMs.from_device_rows(one, two[r0:r1], S, rows_layout, row_offset=r0)
            if compress is not None:
                assert compress == "sym8"
                trd.compress_sym8_()
        else:
            trd = DeviceTRDMs(one, two, S, device, row_range=(r0, r1), compress=compress)
        assert (trd.row_offset, trd.rows_local) == (r0, r1 - r0)
        evs.append(ContinuationEvaluator(trd, natm, want_two_rdm=keep) if single
                   else BatchedEvaluator(trd, natm, G, keep_density_matrices=keep))
    rows_total = evs[0].t.rows_total
    check_ranges(ranges, rows_total)
    # phase A into (G, chunk) send buffers; chunk holds the longest range (PairShardedContinuation: ceil(rows / world))
    chunk = max(1, max(r1 - r0 for r0, r1 in ranges))
    send, records = [], []
    for ev, (r0, r1) in zip(evs, ranges):
        buf = torch.zeros((G, chunk), dtype=torch.float64, device=device)
        if single:
            rows_local = ev.phase_hamiltonian(geo)
            if r1 > r0:
                buf[0, : r1 - r0].copy_(rows_local[: r1 - r0])
        else:
            ev.phase_hamiltonian(geo, buf)
        send.append(buf)
        records.append({"k5_rows": _record("k5_rows")})
    recv = torch.stack(send)                                       # (world, G, chunk) = all_gather_into_tensor
    rows_all = recv.permute(1, 0, 2).reshape(G, world * chunk).contiguous()
    # (rank, g, r) -> (g, rank * chunk + r).  Equal chunks (shard_rows) leave the rows of a geometry contiguous in pair
    # order, padding behind them; other cut points leave padding between the chunks, which is taken out
    at = torch.cat([k * chunk + torch.arange(r1 - r0) for k, (r0, r1) in enumerate(ranges)])
    if not torch.equal(at, torch.arange(rows_total)):
        rows_all = rows_all[:, at.to(device)].contiguous()
    nan = float("nan")
    for k, ev in enumerate(evs):
        if single:
            ev.phase_solve(geo, rows_all[0, :rows_total].contiguous(), nroots)
        else:
            ev.phase_solve(geo, rows_all, nroots)
        records[k]["subspace"] = _record("subspace")
        ev.grad.fill_(nan)                 # a kernel of phase C that skips its stores must not pass on what was there
        if keep:
            ev.d_pred.fill_(nan)
            ev.g_pred.fill_(nan)
        ev.phase_gradient(geo, partial_rank=(k != 0))
        records[k]["k8_cols"] = _record("k8_cols")
    torch.cuda.synchronize(device)
    n, T = evs[0].t.n, evs[0].t.T
    host = lambda t, shape: t.reshape(shape).cpu().numpy().copy()
    run = ShardedRun(ranges=list(ranges), energy=[host(ev.energy, (G, T)) for ev in evs],
                     grad_rank=[host(ev.grad, (G, -1, 3))[:, :natm] for ev in evs], grad=None, records=records,
                     plans=[describe(ev.t.cstruct, G) for ev in evs])
    run.grad = np.sum(run.grad_rank, axis=0)
    run.d_pred = [host(ev.d_pred, (G, n, n)) if keep else None for ev in evs]
    run.g_pred_rank = [host(ev.g_pred, (G, n, n, n, n)) if keep else None for ev in evs]
    run.g_pred = np.sum(run.g_pred_rank, axis=0) if keep else None
    return run
