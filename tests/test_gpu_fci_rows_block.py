"""GPU tests of the block row call (include/evcont_hip.h: evc_fci_trdm_rows_block), called directly: several bras
against shared kets, ragged consecutive output rows.

One shape per distinct t-RDM tiling of tests/fci_dispatch_table.py (every (RT, NBW, quadrants)), with the fewest
electrons that still give two determinant blocks where the orbital count allows more than 256 determinants.  Per shape:
K = 6 random vectors, the bras are the last kets by pointer; nbras in 1, 2, 3, 5; counts triangular, rectangular and
[1, ..., 1, K]; the least workspace, the resident one and the one between (every bra resident, kets in chunks of one
block).  Every call is held to

  (a) the bits of evc_fci_trdm_rows of each bra against all kets (one reference per shape, shared and left unchanged);
  (b) SmallFCI.trans_rdm12 within 2 * trdm_bound of tests/test_gpu_fci_device.py (the single call's bound);
  (c) a second call: the same bits;
  (d) NaN-filled outputs with two guard rows behind them: exactly the ragged rows are written, the fences stay;
  (e) the single call's stage record followed by " bras=<nbras>", the single call's own record unchanged.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from evcont_amd.fci_small import SmallFCI
from fci_dispatch_table import TILINGS, rows_per_block, trdm_record
from test_gpu_fci_abi import Fenced, Problem
from test_gpu_fci_device import random_vectors, trdm_bound

pytestmark = pytest.mark.gpu

_HOST = SmallFCI()
K = 6
NBRAS = (1, 2, 3, 5)
GUARD = 2
# (norb, nelec): one per (RT, NBW, quadrants); 5 orbitals and fewer have at most 100 determinants (one block)
BLOCK_SHAPES = [(2, (1, 1)), (5, (2, 2)), (6, (3, 3)), (7, (2, 2)), (9, (2, 1)), (10, (2, 1)), (12, (2, 1)), (12, (1, 1)),
                (13, (2, 1)), (14, (2, 1)), (16, (1, 1))]
IDS = [f"{n}-{e}".replace(" ", "") for n, e in BLOCK_SHAPES]


def test_shapes_cover_every_tiling():
    key = lambda n: (TILINGS[n]["trdm"], TILINGS[n]["quadrants"])
    assert {key(n) for n, _ in BLOCK_SHAPES} == {key(n) for n in TILINGS}
    for norb, nelec in BLOCK_SHAPES:
        p = Problem(norb, nelec)
        if norb > 5 and (norb, nelec) not in ((12, (1, 1)), (16, (1, 1))):
            assert p.dim > rows_per_block(p.dim), (norb, nelec)      # at least two determinant blocks


def counts_of(kind, R):
    return {"triangular": list(range(K - R + 1, K + 1)), "rectangular": [K] * R, "one_one_K": [1] * (R - 1) + [K]}[kind]


def workspaces(p, R):
    """(name, bytes, regime) of the three workspaces: the layout of include/evcont_hip.h written out."""
    rows = rows_per_block(p.dim)
    nblk = -(-p.dim // rows)
    fixed = -(-(R * (nblk * (p.npad * p.npad + p.npad + 1) + p.npad) * 8) // 256) * 256
    block = rows * p.npad * 8
    least = fixed + (R + 1) * block
    full = fixed + (R + 1) * nblk * block
    between = fixed + (R * nblk + 1) * block
    assert p.lib.evc_fci_rows_block_workspace_bytes(p.norb, p.na, p.nb, R, 1) >= least
    assert p.lib.evc_fci_rows_block_workspace_bytes(p.norb, p.na, p.nb, R, 0) >= full
    out = [("least", least, f"bra_resident={int(nblk == 1)} ket_blocks=1"),
           ("between", between, "bra_resident=1 ket_blocks=1"),
           ("resident", full, f"bra_resident=1 ket_blocks={nblk}")]
    return out


@functools.lru_cache(maxsize=None)
def reference(norb, nelec):
    """Per shape, once: the vectors on the device, the single call of every bra against all K kets (resident
    workspace) and the numpy statement of every pair with its bound."""
    p = Problem(norb, nelec)
    vecs = random_vectors(norb, nelec, K, seed=4000 + 31 * norb + nelec[0])
    dvecs = [p.up(v) for v in vecs]
    single = {}
    for j in range(K - max(NBRAS), K):
        ov, d1, d2, rec = p.trdm_rows(vecs[j], vecs, p.full)
        for a in (ov, d1, d2):
            a.setflags(write=False)
        single[j] = (ov, d1, d2)
        assert " bras=" not in rec and rec.startswith(trdm_record(norb, p.dim)), rec
        for i in range(K):
            r1, r2 = _HOST.trans_rdm12(vecs[j], vecs[i], norb, nelec)
            tol = 2.0 * trdm_bound(vecs[j], vecs[i], norb, nelec)
            assert abs(ov[i] - np.dot(vecs[j].ravel(), vecs[i].ravel())) <= tol
            assert np.abs(d1[i] - r1).max() <= tol and np.abs(d2[i] - r2).max() <= tol, (j, i)
    return p, vecs, dvecs, single, rec


def block_call(p, dvecs, R, counts, ws_bytes):
    n2 = p.norb ** 2
    total = sum(counts)
    nk = counts[-1]
    bras = (C.c_void_p * R)(*[dvecs[K - R + r].data_ptr() for r in range(R)])
    kets = (C.c_void_p * nk)(*[dvecs[i].data_ptr() for i in range(nk)])
    cnt = (C.c_int * R)(*counts)
    ws = Fenced(ws_bytes, p.dev, front=False)
    ov, d1, d2 = (Fenced(8 * (total + GUARD) * w, p.dev) for w in (1, n2, n2 * n2))
    p.check(p.lib.evc_fci_trdm_rows_block(p.norb, p.na, p.nb, p.ta.data_ptr(), p.tb.data_ptr(), bras, R, kets, cnt, ov.ptr,
                                          d1.ptr, d2.ptr, ws.ptr, ws_bytes, None), "evc_fci_trdm_rows_block")
    torch.cuda.synchronize()
    for f in (ws, ov, d1, d2):
        assert f.fences_intact(), (R, counts, ws_bytes)
    return (ov.doubles(), d1.doubles().reshape(total + GUARD, n2), d2.doubles().reshape(total + GUARD, n2 * n2),
            p.record("fci_trdm"))


@pytest.mark.parametrize("norb,nelec", BLOCK_SHAPES, ids=IDS)
def test_block_call_against_single_calls(norb, nelec):
    p, vecs, dvecs, single, single_rec = reference(norb, nelec)
    n2 = norb * norb
    head = trdm_record(norb, p.dim)
    regimes = set()
    for R in NBRAS:
        for kind in ("triangular", "rectangular", "one_one_K"):
            counts = counts_of(kind, R)
            total = sum(counts)
            for name, ws_bytes, regime in workspaces(p, R):
                ov, d1, d2, rec = block_call(p, dvecs, R, counts, ws_bytes)
                what = (norb, nelec, R, kind, name)
                assert rec == f"{head}{regime} bras={R}", (what, rec)                                  # (e)
                regimes.add(regime)
                row = 0
                for r in range(R):
                    sov, sd1, sd2 = single[K - R + r]
                    n = counts[r]
                    assert np.array_equal(ov[row:row + n], sov[:n]), what                                # (a), (b), (d)
                    assert np.array_equal(d1[row:row + n], sd1[:n].reshape(n, n2)), what
                    assert np.array_equal(d2[row:row + n], sd2[:n].reshape(n, n2 * n2)), what
                    row += n
                assert row == total
                assert np.isnan(ov[total:]).all() and np.isnan(d1[total:]).all() and np.isnan(d2[total:]).all(), what
                ov2, d12, d22, rec2 = block_call(p, dvecs, R, counts, ws_bytes)                          # (c)
                assert rec2 == rec and np.array_equal(ov2, ov, equal_nan=True), what
                assert np.array_equal(d12, d1, equal_nan=True) and np.array_equal(d22, d2, equal_nan=True), what
    nblk = -(-p.dim // rows_per_block(p.dim))
    assert len(regimes) == (3 if nblk > 1 else 1), regimes
    # the single call after the block calls: its record and its bits as before
    ov, d1, d2, rec = p.trdm_rows(vecs[K - 1], vecs, p.full)
    assert rec == single_rec and " bras=" not in rec
    sov, sd1, sd2 = single[K - 1]
    assert np.array_equal(ov, sov) and np.array_equal(d1, sd1) and np.array_equal(d2, sd2)


def test_short_workspace_is_refused():
    p, _, dvecs, _, _ = reference(6, (3, 3))
    _, least, _ = workspaces(p, 3)[0]
    with pytest.raises(Exception, match="evc_fci_trdm_rows_block: workspace of"):
        block_call(p, dvecs, 3, [4, 5, 6], least - 16)
