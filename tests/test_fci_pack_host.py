"""CPU tests of the packed row call and the resident training set: argument errors of both new entry points (no device
needed: they are refused before any launch), the numpy statement of the two packings the GPU tests compare with
(tests/fci_pack_reference.py) against the project's own definitions, and the row map of ``ResidentTRDMs.prune``."""
import numpy as np
import pytest

from fci_pack_reference import pack2_row, pack_cols, sym8_row


@pytest.fixture(scope="module")
def lib():
    from evcont_amd import build, _lib
    build.build()
    return _lib.load()


def test_argument_validation_without_gpu(lib):
    """Every argument error returns rc < 0 with a message, before anything is enqueued."""
    import ctypes as C
    from evcont_amd._lib import LAYOUT_PACK2, LAYOUT_SYM8
    norb, na, nb = 4, 6, 6
    least = lib.evc_fci_rows_packed_workspace_bytes(norb, na, nb, 1)
    full = lib.evc_fci_rows_packed_workspace_bytes(norb, na, nb, 0)
    slot = 4 ** 4 * 8
    assert least == lib.evc_fci_workspace_bytes(norb, na, nb, 1) + slot
    assert full == lib.evc_fci_workspace_bytes(norb, na, nb, 0) + slot and 0 < least <= full
    assert lib.evc_fci_rows_packed_workspace_bytes(17, na, nb, 0) == 0 and b"norb=17" in lib.evc_last_error()
    assert lib.evc_fci_rows_packed_workspace_bytes(norb, 0, nb, 0) == 0 and b"na=0" in lib.evc_last_error()
    p = 4096                                                  # a non-null, 16-byte aligned address that is never read
    kets = (C.c_void_p * 1)(p)
    ld2, ld8 = 144, 64                                        # 136 and 55 columns rounded up to 16

    def call(norb=norb, tab_a=p, tab_b=p, bra=p, kets=kets, nkets=1, ovlp=p, dm1=p, layout=LAYOUT_PACK2, rows=p, ld=ld2,
             ws=p, ws_bytes=full):
        return lib.evc_fci_trdm_rows_packed(norb, na, nb, tab_a, tab_b, bra, kets, nkets, ovlp, dm1, layout, rows, ld, ws,
                                            ws_bytes, None)

    for name in ("tab_a", "tab_b", "bra", "kets", "ovlp", "dm1", "rows", "ws"):
        assert call(**{name: None}) < 0 and b"null pointer" in lib.evc_last_error(), name
    assert call(kets=(C.c_void_p * 1)(None)) < 0 and b"kets[0] is null" in lib.evc_last_error()
    for layout in (0, 3, 5, 6, 7, -1):
        assert call(layout=layout) < 0 and b"layout=" in lib.evc_last_error(), layout
    for ld in (0, 136, 128, 143, 152, -16):                   # below the columns, or no multiple of 16
        assert call(ld=ld) < 0 and b"ld=" in lib.evc_last_error(), ld
    assert call(layout=LAYOUT_SYM8, ld=48) < 0 and b"ld=48" in lib.evc_last_error()
    assert call(layout=LAYOUT_SYM8, ld=ld8 + 8) < 0 and b"ld=72" in lib.evc_last_error()
    for nkets in (0, -1, 4097):
        assert call(nkets=nkets) < 0 and b"nkets=" in lib.evc_last_error(), nkets
    for ws_bytes in (0, 16, slot, slot + 4096):               # the slot alone, or with far less than one block behind it
        assert call(ws_bytes=ws_bytes) < 0 and b"workspace of" in lib.evc_last_error(), ws_bytes
    # the boundary: at this shape the t-RDM part decides the least size, so the call needs exactly what the query
    # returns -- the slot counted once -- and says so (a call with `least` itself would be enqueued: GPU tests)
    assert lib.evc_fci_workspace_bytes(norb, na, nb, 1) == 2560 + 2 * 256 * 16 * 8     # partials | two blocks of D
    for ws_bytes in (least - 16, least - 1):
        assert call(ws_bytes=ws_bytes) < 0
        assert f"workspace of {ws_bytes} bytes, at least {least} needed".encode() in lib.evc_last_error(), ws_bytes
    assert call(ws=p + 8) < 0 and b"aligned" in lib.evc_last_error()
    assert call(norb=17) < 0 and b"norb=17" in lib.evc_last_error()


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_numpy_packings_against_the_projects_definitions(n):
    from evcont_amd.evaluator import layout_shape, sym8_column_images
    from evcont_amd.synthetic import pack_rows
    dm2 = np.random.default_rng(n).standard_normal((n, n, n, n))
    want2 = pack_rows(dm2[None, None], True, True)
    assert want2.shape == (1, pack_cols("pack2", n)) == layout_shape(2, 1, n)
    assert np.array_equal(pack2_row(dm2), want2[0])
    imgs = sym8_column_images(6, n)
    flat = dm2.reshape(-1)
    acc = flat[imgs[0]].copy()
    for ix in imgs[1:]:
        acc += flat[ix]                                       # the order of evaluator.sym8_gather_sums
    got = sym8_row(dm2)
    assert got.shape == (pack_cols("sym8", n),) == layout_shape(8, 1, n)[1:]
    assert np.array_equal(got, acc * 0.125)
    # ... and from the packed source the same classes (another summation order: to rounding)
    p2 = pack2_row(dm2 + dm2.transpose(2, 3, 0, 1))           # a bra<->ket symmetric block, as pack2 assumes
    acc2 = sum(p2[ix] for ix in sym8_column_images(2, n))
    np.testing.assert_allclose(sym8_row(dm2 + dm2.transpose(2, 3, 0, 1)), acc2 * 0.125, rtol=0, atol=1e-14)


@pytest.mark.parametrize("T,keep", [(5, [0, 2, 3]), (4, [1]), (6, [0, 1, 2, 3, 4, 5]), (7, [2, 6]), (3, [])])
def test_prune_row_map_is_ix_slicing_then_tril(T, keep):
    from evcont_amd.resident import pair_row, prune_row_map
    full = np.random.default_rng(T).standard_normal((T, T, 3))
    a, b = np.tril_indices(T)
    rows = full[a, b]                                         # the (P, .) matrix of the pairs a >= b
    assert all(pair_row(x, y) == p for p, (x, y) in enumerate(zip(a, b)))
    sliced = full[np.ix_(keep, keep)]
    i, j = np.tril_indices(len(keep))
    assert np.array_equal(rows[prune_row_map(keep)].reshape(-1, 3), sliced[i, j].reshape(-1, 3))


@pytest.mark.parametrize("keep", [[2, 0], [0, 0], [1, 2, 2], [3, 1, 2], [0, 5], [-1, 2]])
def test_prune_rejects_ids_that_are_not_strictly_increasing(keep):
    from evcont_amd.resident import check_keep_ids
    with pytest.raises(ValueError):
        check_keep_ids(keep, 5)
    assert check_keep_ids([0, 2, 4], 5) == [0, 2, 4] and check_keep_ids(np.array([1]), 5) == [1]
