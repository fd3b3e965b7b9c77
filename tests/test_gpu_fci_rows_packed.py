"""GPU tests of the packed row call (``DeviceFCI.trans_rdm12_rows_packed`` / ``evc_fci_trdm_rows_packed``,
csrc/fci_pack.hip): the two-body t-RDM rows of a bra against K kets written on the device in the layouts the evaluator
streams, against the numpy statement of the two packings (tests/fci_pack_reference.py, held to the project's own
definitions by tests/test_fci_pack_host.py).

* Integer CI vectors (tests/test_gpu_fci_shapes.py): every sum is an integer and the factor 0.125 is exact, so the rows
  must be the packing of the host's ``SmallFCI.trans_rdm12`` bit for bit.
* Random unit vectors: the packing only moves (pack2) or adds in a fixed order (sym8) the elements ``trans_rdm12_rows``
  returns, so the rows must have the bits of the packing of that dense result, and for sym8 the bits of
  ``DeviceTRDMs(..., compress="sym8")`` on it; against the host they are held to twice the bound derived in
  tests/test_gpu_fci_device.py (a pack2 column is one element, a sym8 column the mean of eight, so the element bound
  holds for both; the host side of that comparison is packed in extended precision so that only the device rounds).
* The target is a NaN-poisoned matrix with rows and columns to spare, the workspace sits between fences.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from evcont_amd.fci_small import SmallFCI
from fci_pack_reference import pack_cols, pack_row
from test_gpu_fci_abi import FENCE, Fenced, Problem
from test_gpu_fci_device import random_vectors, solver, trdm_bound
from test_gpu_fci_shapes import integer_vectors, integral

pytestmark = pytest.mark.gpu

_HOST = SmallFCI()
SHAPES = [(1, (1, 1)), (2, (1, 1)), (3, (2, 1)), (4, (2, 2)), (5, (3, 2)),     # na != nb and odd N^2 among them
          (6, (3, 3)),                                                         # two determinant blocks
          (9, (2, 2)),                                                         # npad = 96 != 81, <3,2> tiling
          (13, (1, 1)),                                                        # 2 x 2 quadrants
          (16, (1, 1))]                                                        # the largest cols
IDS = [f"{n}-{e[0]}{e[1]}" for n, e in SHAPES]
LAYOUTS = ["pack2", "sym8"]
K = 3                                    # two other kets and the bra itself


def ld_of(layout, norb):
    return (pack_cols(layout, norb) + 15) // 16 * 16


def pack_record():
    from evcont_amd import _lib
    return _lib.load().evc_profile_kernel(_lib.FCI_PROF_PACK).decode()


@functools.lru_cache(maxsize=None)
def integer_case(norb, nelec):
    """(bra, kets, host dm2 per ket, dense device (ovlp, dm1)): computed once, read by both layouts."""
    vecs = integer_vectors(norb, nelec, K, seed=4000 + 31 * norb + nelec[0] + 5 * nelec[1])
    bra, kets = vecs[0], vecs[1:] + [vecs[0]]
    host2 = [_HOST.trans_rdm12(bra, k, norb, nelec)[1] for k in kets]
    assert all(integral(d) for d in host2)
    ov, one, _ = solver().trans_rdm12_rows(bra, kets, norb, nelec)
    return bra, kets, host2, ov, one


@functools.lru_cache(maxsize=None)
def random_case(norb, nelec):
    """(bra, kets, dense device results, host dm2 and bound per ket)."""
    vecs = random_vectors(norb, nelec, K, seed=6000 + norb * 10 + nelec[1])
    bra, kets = vecs[0], vecs[1:] + [vecs[0]]
    dense = solver().trans_rdm12_rows(bra, kets, norb, nelec)
    host2 = [_HOST.trans_rdm12(bra, k, norb, nelec)[1] for k in kets]
    tol = [2.0 * trdm_bound(bra, k, norb, nelec) for k in kets]
    return bra, kets, dense, host2, tol


def packed_call(dev_solver, bra, kets, norb, nelec, layout):
    out = torch.full((len(kets), ld_of(layout, norb)), float("nan"), dtype=torch.float64, device="cuda:0")
    ov, one = dev_solver.trans_rdm12_rows_packed(bra, kets, norb, nelec, layout, out)
    torch.cuda.synchronize()
    return ov, one, out.cpu().numpy()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("norb,nelec", SHAPES, ids=IDS)
def test_integer_inputs_give_the_packing_of_the_host_bit_for_bit(norb, nelec, layout):
    bra, kets, host2, ov_d, one_d = integer_case(norb, nelec)
    ov, one, rows = packed_call(solver(), bra, kets, norb, nelec, layout)
    cols, ld = pack_cols(layout, norb), ld_of(layout, norb)
    assert pack_record() == f"fci_row_pack_kernel<{8 if layout == 'sym8' else 1}> rows={K} cols={cols} ld={ld}"
    assert np.array_equal(ov, ov_d) and np.array_equal(one, one_d)
    for i, d2 in enumerate(host2):
        want = pack_row(layout, d2)
        assert want.shape == (cols,)
        assert np.array_equal(rows[i, :cols], want), (i, int((rows[i, :cols] != want).sum()))
        assert not rows[i, cols:].any()                                   # zeros, not NaN
    print(f"packed integers norb={norb} nelec={nelec} {layout}: cols={cols} ld={ld} max|row|={np.abs(rows).max():.3f}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("norb,nelec", SHAPES, ids=IDS)
def test_random_vectors_give_the_bits_of_the_dense_call_packed(norb, nelec, layout):
    from evcont_amd.evaluator import DeviceTRDMs
    bra, kets, (ov_d, one_d, two_d), host2, tol = random_case(norb, nelec)
    ov, one, rows = packed_call(solver(), bra, kets, norb, nelec, layout)
    cols = pack_cols(layout, norb)
    assert np.array_equal(ov, ov_d) and np.array_equal(one, one_d)
    worst = 0.0
    for i in range(K):
        assert np.array_equal(rows[i, :cols], pack_row(layout, two_d[i])), i
        if layout == "sym8":
            t = DeviceTRDMs(one_d[i][None, None], two_d[i][None, None], np.ones((1, 1)), "cuda:0", compress="sym8")
            assert t.layout == 8 and np.array_equal(rows[i], t.two[0].cpu().numpy()), i
        err = np.abs(rows[i, :cols] - pack_row(layout, host2[i], np.longdouble)).max()
        worst = max(worst, float(err / tol[i]))
        print(f"packed random norb={norb} nelec={nelec} {layout} ket {i}: |d row|={float(err):.3e} bound={tol[i]:.3e}")
        assert err <= tol[i]
    print(f"packed random norb={norb} nelec={nelec} {layout}: worst error / allowed = {worst:.3e}")


def fenced_solver(norb, nelec):
    """A DeviceFCI whose workspace sits between two fences: (solver, the fenced buffer)."""
    from evcont_amd import _lib
    from evcont_amd.fci_device import DeviceFCI
    lib = _lib.load()
    s = DeviceFCI()
    _, _, na, nb, _ = s._setup(norb, nelec)[1:]
    f = Fenced(lib.evc_fci_rows_packed_workspace_bytes(norb, na, nb, 0), torch.device("cuda:0"))
    s._ws = f.buf[f.off:f.off + f.nbytes]
    return s, f


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("norb,nelec", SHAPES, ids=IDS)
def test_only_the_rows_of_the_view_are_written(norb, nelec, layout):
    """A (K + 4, ld + 32) matrix of NaN, the (K, ld) view at row 2: rows 2 ... K + 1 and columns < ld change, columns
    cols ... ld - 1 are zero, everything else is still NaN; the workspace fences are intact."""
    bra, kets, _, _, _ = random_case(norb, nelec)
    _, _, want = packed_call(solver(), bra, kets, norb, nelec, layout)
    cols, ld = pack_cols(layout, norb), ld_of(layout, norb)
    s, fence = fenced_solver(norb, nelec)
    M = torch.full((K + 4, ld + 32), float("nan"), dtype=torch.float64, device="cuda:0")
    s.trans_rdm12_rows_packed(bra, kets, norb, nelec, layout, M[2:K + 2, :ld])
    torch.cuda.synchronize()
    assert fence.fences_intact() and s._ws.data_ptr() == fence.ptr
    got = M.cpu().numpy()
    assert np.array_equal(got[2:K + 2, :ld], want)
    assert not got[2:K + 2, cols:ld].any()
    assert np.isnan(got[:2]).all() and np.isnan(got[K + 2:]).all() and np.isnan(got[:, ld:]).all()
    # rows that follow each other at the pitch ld are written in place, through the same fenced workspace
    M2 = torch.full((K + 4, ld), float("nan"), dtype=torch.float64, device="cuda:0")
    s.trans_rdm12_rows_packed(bra, kets, norb, nelec, layout, M2[2:K + 2])
    torch.cuda.synchronize()
    assert fence.fences_intact()
    got = M2.cpu().numpy()
    assert np.array_equal(got[2:K + 2], want) and np.isnan(got[:2]).all() and np.isnan(got[K + 2:]).all()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("norb,nelec", [(6, (3, 3)), (9, (2, 2))], ids=["6-33", "9-22"])
def test_the_entry_point_with_fenced_buffers_and_the_least_workspace(norb, nelec, layout):
    """evc_fci_trdm_rows_packed called directly: outputs and workspace between fences, a pitch wider than the columns
    (zero up to the pitch), and the least workspace gives the bits of the resident one."""
    from evcont_amd import _lib
    p = Problem(norb, nelec)
    lib = p.lib
    bra, kets, _, _, _ = random_case(norb, nelec)
    _, _, want = packed_call(solver(), bra, kets, norb, nelec, layout)
    cols, ld = pack_cols(layout, norb), ld_of(layout, norb) + 32
    least = lib.evc_fci_rows_packed_workspace_bytes(norb, p.na, p.nb, 1)
    full = lib.evc_fci_rows_packed_workspace_bytes(norb, p.na, p.nb, 0)
    assert 0 < least < full
    dbra, dkets = p.up(bra), [p.up(k) for k in kets]
    ptrs = (C.c_void_p * K)(*[t.data_ptr() for t in dkets])
    lay = {"pack2": _lib.LAYOUT_PACK2, "sym8": _lib.LAYOUT_SYM8}[layout]
    for ws_bytes in (full, least):
        ws = Fenced(ws_bytes, p.dev, front=False)
        ov, d1, rows = Fenced(8 * K, p.dev), Fenced(8 * K * norb * norb, p.dev), Fenced(8 * K * ld, p.dev)
        p.check(lib.evc_fci_trdm_rows_packed(norb, p.na, p.nb, p.ta.data_ptr(), p.tb.data_ptr(), dbra.data_ptr(), ptrs, K,
                                             ov.ptr, d1.ptr, lay, rows.ptr, ld, ws.ptr, ws_bytes, None),
                "evc_fci_trdm_rows_packed")
        torch.cuda.synchronize()
        for f in (ws, ov, d1, rows):
            assert f.fences_intact(), ws_bytes
        got = rows.doubles().reshape(K, ld)
        assert np.array_equal(got[:, :cols], want[:, :cols]), ws_bytes
        assert not got[:, cols:].any()
        rec = p.record("fci_trdm")
        assert ("bra_resident=1" in rec) == (ws_bytes == full), rec


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("norb,nelec", [(6, (3, 3)), (9, (2, 2))], ids=["6-33", "9-22"])
def test_a_solver_with_the_least_workspace_gives_the_resident_bits(norb, nelec, layout):
    from evcont_amd import _lib
    from evcont_amd.fci_device import DeviceFCI
    lib = _lib.load()
    bra, kets, _, _, _ = random_case(norb, nelec)
    _, _, na, nb = _HOST._ops(norb, nelec)
    small = DeviceFCI(workspace_bytes=lib.evc_fci_workspace_bytes(norb, na, nb, 1))
    a = packed_call(solver(), bra, kets, norb, nelec, layout)
    b = packed_call(small, bra, kets, norb, nelec, layout)
    assert "bra_resident=0" in lib.evc_profile_kernel(_lib.FCI_PROF_STAGES["fci_trdm"]).decode()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_bad_arguments_raise_before_any_launch():
    from evcont_amd._lib import EvcontHipError
    bra, kets, _, _, _ = random_case(4, (2, 2))
    ok = torch.zeros((K, ld_of("pack2", 4)), dtype=torch.float64, device="cuda:0")
    with pytest.raises(EvcontHipError, match="layout"):
        solver().trans_rdm12_rows_packed(bra, kets, 4, (2, 2), "pair5", ok)
    with pytest.raises(EvcontHipError, match="out_rows"):
        solver().trans_rdm12_rows_packed(bra, kets, 4, (2, 2), "pack2", ok[:2])
    with pytest.raises(EvcontHipError, match="ld="):
        solver().trans_rdm12_rows_packed(bra, kets, 4, (2, 2), "pack2", ok[:, :64])
    assert not ok.any().item()
