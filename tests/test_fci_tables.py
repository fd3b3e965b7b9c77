"""CPU tests of the string tables behind the device full-CI kernels (evcont_amd/fci_tables.py): they hold the content of
the CSR excitation operators of fci_small._excitation_ops entry for entry, and a numpy walk through the packed tables --
what the excite kernel does -- reproduces SmallFCI._excite_all bit for bit.  Also the host-side limits of the device
solver and of its C entry points, which are checked before anything is launched."""
import ctypes as C

import numpy as np
import pytest

from evcont_amd.fci_small import SmallFCI, _excitation_ops

CASES = [(4, 2), (6, 3), (6, 2), (8, 4), (5, 0), (5, 5),
         (9, 1), (9, 2), (9, 3), (13, 1), (13, 2), (13, 3), (16, 1), (16, 2), (16, 3)]


@pytest.mark.parametrize("norb,nocc", CASES)
def test_tables_reproduce_excitation_ops(norb, nocc):
    from evcont_amd.fci_tables import excitation_table, packed_table, npad_of
    ops, ns = _excitation_ops(norb, nocc)
    index, sign = excitation_table(norb, nocc)
    packed = packed_table(norb, nocc)
    assert index.shape == sign.shape == (norb * norb, ns) and index.dtype == np.int32
    assert packed.shape == (ns, npad_of(norb)) and packed.dtype == np.int32 and npad_of(norb) % 16 == 0
    assert not packed[:, norb * norb:].any()
    for p in range(norb):
        for q in range(norb):
            m = ops[p][q].tocoo()
            want_idx = np.full(ns, -1, dtype=np.int64)
            want_sgn = np.zeros(ns, dtype=np.int64)
            assert len(set(m.row.tolist())) == m.nnz                  # at most one J per resulting string I
            want_idx[m.row] = m.col
            want_sgn[m.row] = m.data.astype(np.int64)
            assert np.array_equal(index[p * norb + q], want_idx), (p, q)
            assert np.array_equal(sign[p * norb + q], want_sgn), (p, q)
            assert np.array_equal(packed[:, p * norb + q], want_sgn * (want_idx + 1)), (p, q)


@pytest.mark.parametrize("norb,nelec", [(4, (2, 2)), (6, (3, 3)), (6, (3, 2)), (6, (2, 3)), (8, (4, 4)), (5, (0, 5)),
                                        (5, (5, 0)), (5, (2, 0)), (9, (1, 2)), (9, (3, 3)), (13, (2, 1)),
                                        (13, (3, 2)), (16, (1, 1)), (16, (2, 2)), (16, (3, 1))])
def test_excite_through_tables_is_excite_all_bitwise(norb, nelec):
    from evcont_amd.fci_tables import excite_through_tables, packed_table
    na, nb = packed_table(norb, nelec[0]).shape[0], packed_table(norb, nelec[1]).shape[0]
    c = np.random.default_rng(norb * 100 + nelec[0] * 10 + nelec[1]).standard_normal((na, nb))
    want = SmallFCI()._excite_all(c, norb, nelec)
    got = excite_through_tables(c, norb, nelec)
    assert got.shape == want.shape == (norb * norb, na, nb)
    assert np.array_equal(got, want)


def test_table_limits():
    from evcont_amd.fci_tables import excitation_table
    for norb, nocc in ((17, 8), (0, 0), (4, 5), (4, -1)):
        with pytest.raises(ValueError):
            excitation_table(norb, nocc)


def test_device_solver_limits_raise_before_any_launch():
    """norb = 17 and a workspace too small for the problem: EvcontHipError from the host-side checks (no device here)."""
    from evcont_amd import build
    from evcont_amd._lib import EvcontHipError
    from evcont_amd.fci_device import DeviceFCI
    build.build()
    with pytest.raises(EvcontHipError, match="norb=17"):
        DeviceFCI().trans_rdm12(np.zeros(4), np.zeros(4), 17, (1, 1))
    with pytest.raises(EvcontHipError, match="norb=17"):
        DeviceFCI().kernel(np.zeros((17, 17)), np.zeros((17,) * 4), 17, (1, 1))
    with pytest.raises(EvcontHipError, match="workspace_bytes=4096"):
        DeviceFCI(workspace_bytes=4096).trans_rdm12(np.zeros((15, 15)), np.zeros((15, 15)), 6, (2, 2))
    with pytest.raises(EvcontHipError, match="workspace_bytes=4096"):
        DeviceFCI(workspace_bytes=4096).contract(np.zeros((6, 6)), np.zeros((6,) * 4), np.zeros((15, 15)), 6, (2, 2))


def test_fci_entry_points_validate_on_the_host():
    from evcont_amd import build, _lib
    build.build()
    lib = _lib.load()
    na = nb = 20                                                   # (6, (3, 3))
    least, full = lib.evc_fci_workspace_bytes(6, na, nb, 1), lib.evc_fci_workspace_bytes(6, na, nb, 0)
    assert 0 < least <= full
    assert lib.evc_fci_workspace_bytes(17, 10, 10, 0) == 0 and b"norb=17" in lib.evc_last_error()
    # the resident grant holds what the docstrings promise: two (dim, npad) excitation arrays at least
    n12 = lib.evc_fci_workspace_bytes(12, 924, 924, 0)
    assert 2 * 853776 * 144 * 8 <= n12 < 3 * 853776 * 144 * 8
    kets = (C.c_void_p * 1)(256)
    call = lambda norb=6, ws_bytes=full, k=kets, nk=1: lib.evc_fci_trdm_rows(
        norb, na, nb, 256, 256, 256, k, nk, 256, 256, 256, 256, ws_bytes, None)
    assert call(norb=17) < 0 and b"norb=17" in lib.evc_last_error()
    assert call(ws_bytes=1024) < 0 and b"workspace" in lib.evc_last_error()
    assert call(nk=0) < 0 and b"nkets" in lib.evc_last_error()
    assert call(k=(C.c_void_p * 1)(None)) < 0 and b"null" in lib.evc_last_error()
    sig = lambda norb=6, ws_bytes=full, out=512: lib.evc_fci_sigma(norb, na, nb, 256, 256, 256, 256, 256, out, 256,
                                                                   ws_bytes, None)
    assert sig(norb=0) < 0 and b"norb=0" in lib.evc_last_error()
    assert sig(ws_bytes=1024) < 0 and b"workspace" in lib.evc_last_error()
    assert sig(out=256) < 0 and b"alias" in lib.evc_last_error()
    assert lib.evc_fci_excite(6, na, nb, 256, 256, 256, 0, 64, 7, 256, 48, None) < 0
    assert b"layout" in lib.evc_last_error()
    assert lib.evc_fci_excite(6, na, nb, 256, 256, 256, 0, 64, _lib.FCI_ORB_MAJOR, 256, 48, None) < 0
    assert b"ld=" in lib.evc_last_error()
