"""CPU tests of the batched several-roots gradient entry point (include/evcont_hip.h evc_phase_gradient_roots_batch):
it is exported and bound without an ABI bump, every argument error is caught before anything is enqueued (rc < 0,
message set; dummy device pointers, no stream), and its workspace grows with the slot count count * npairs."""
import ctypes as C

import numpy as np
import pytest

SYMS = ("evc_phase_gradient_roots_batch", "evc_workspace_bytes_roots_batch")


@pytest.fixture(scope="module")
def lib():
    from evcont_amd import build, _lib
    build.build()
    return _lib.load()


def _set():
    from evcont_amd._lib import TrdmSet
    # H30-like packed set (T=20 pairs): the pointers are never dereferenced by the host-side checks
    return TrdmSet(n=30, ntrain=20, layout=2, rows2=210, row_offset=0, rows2_total=210, cols2=405450, ld2=405456,
                   ld1=900, two_rdm=256, one_rdm=256, s_train=256)


def _batch(count=4, natm=2, **kw):
    from evcont_amd._lib import GeometryBatch
    f = dict(natm=natm, count=count, enuc=256, S=256, hcore=256, eri=256, ipovlp=256, dhcore=256, eri_ip1=256,
             gnuc=256, aoslices=256)
    f.update(kw)
    return GeometryBatch(**f)


def test_batch_roots_symbols_exported_and_bound(lib):
    from evcont_amd import _lib
    for s in SYMS:
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    # additive: the ABI version is still the one of evc_phase_gradient_roots
    assert _lib.ABI_VERSION == 10 and lib.evc_abi_version() == 10


def test_batch_roots_argument_validation_without_gpu(lib):
    from evcont_amd._lib import OutputsRoots, FLAG_IP1_S2KL, FLAG_PARTIAL_RANK, FLAG_ENERGY_ONLY
    t, gb = _set(), _batch()
    out = OutputsRoots(grad=256, d_pred=None, g_pred=None)
    big = lib.evc_workspace_bytes_roots_batch(C.byref(t), 2, 4, 3)
    assert big > 0

    def call(coeffs=256, nvec=3, pairs=((0, 0), (1, 1), (0, 2)), out_=out, flags=0, ws=256, ws_bytes=big, geo=gb):
        P = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        pp = P.ctypes.data if P.size else None
        return lib.evc_phase_gradient_roots_batch(C.byref(t), C.byref(geo) if geo is not None else None, coeffs, nvec,
                                                  pp, P.shape[0], C.byref(out_) if out_ is not None else None, flags,
                                                  ws, ws_bytes, None)

    def bad(match, **kw):
        assert call(**kw) < 0, kw
        msg = lib.evc_last_error()
        assert match.encode() in msg, (kw, msg)
        assert b"evc_phase_gradient_roots_batch" in msg, (kw, msg)

    # NULL pointers
    bad("coeffs", coeffs=None)
    bad("null batch descriptor", geo=None)
    bad("outputs.grad", out_=None)
    bad("outputs.grad", out_=OutputsRoots(grad=None))
    bad("workspace", ws=None)
    bad("required for the gradient", geo=_batch(eri_ip1=None))
    bad("required for the gradient", geo=_batch(gnuc=None))
    bad("required for the gradient", geo=_batch(natm=0))
    bad("S/hcore/eri/enuc", geo=_batch(hcore=None))
    bad("count", geo=_batch(count=0))
    P = np.zeros((1, 2), np.int32)
    assert lib.evc_phase_gradient_roots_batch(C.byref(t), C.byref(gb), 256, 3, None, 1, C.byref(out), 0, 256, big,
                                              None) < 0
    assert b"pairs" in lib.evc_last_error()
    assert lib.evc_phase_gradient_roots_batch(C.byref(t), C.byref(gb), 256, 3, P.ctypes.data, 0, C.byref(out), 0, 256,
                                              big, None) < 0
    assert b"npairs" in lib.evc_last_error()
    # count * npairs > 4096: 4 geometries x 1025 pairs, and 4096 geometries x 2 pairs
    P = np.zeros((1025, 2), np.int32)
    assert lib.evc_phase_gradient_roots_batch(C.byref(t), C.byref(gb), 256, 3, P.ctypes.data, 1025, C.byref(out), 0,
                                              256, 1 << 62, None) < 0
    assert b"4096" in lib.evc_last_error() and b"count * npairs" in lib.evc_last_error()
    bad("count * npairs", pairs=((0, 0), (1, 1)), geo=_batch(count=4096), ws_bytes=1 << 62)
    # the largest admissible slot count passes the check (and fails later only on the workspace size)
    assert call(pairs=((0, 0),) * 1024, ws_bytes=1) < 0 and b"too small" in lib.evc_last_error()
    bad("outside", pairs=((1, 0),))                 # k > l
    bad("outside", pairs=((0, 3),))                 # l >= nvec
    bad("outside", pairs=((-1, 0),))
    bad("nvec", nvec=21)                            # nvec > T
    bad("nvec", nvec=0)
    bad("PARTIAL_RANK", flags=FLAG_PARTIAL_RANK)
    bad("flags", flags=FLAG_ENERGY_ONLY)
    bad("flags", flags=FLAG_IP1_S2KL | 64)
    bad("too small", ws_bytes=big - 1)
    bad("too small", ws_bytes=lib.evc_workspace_bytes_batch(C.byref(t), 2, 4 * 3) - 1)
    bad("too small", ws_bytes=lib.evc_workspace_bytes_roots(C.byref(t), 2, 3))     # one geometry's worth
    bad("misaligned", ws=264)


def test_batch_roots_workspace_grows_with_slots(lib):
    t = _set()
    prev = 0
    for count, p in ((1, 1), (2, 1), (3, 1), (2, 2), (8, 4), (9, 4), (32, 4), (32, 6), (4096, 1)):
        b = lib.evc_workspace_bytes_roots_batch(C.byref(t), 30, count, p)
        assert b > prev, (count, p)
        # one workspace per slot plus the per-slot nuclear term
        assert b >= lib.evc_workspace_bytes_batch(C.byref(t), 30, count * p) + count * p * 30 * 3 * 8
        prev = b
    # the slot count alone decides: (count, npairs) and (npairs, count) need the same bytes
    assert lib.evc_workspace_bytes_roots_batch(C.byref(t), 30, 4, 9) == lib.evc_workspace_bytes_roots_batch(
        C.byref(t), 30, 9, 4) == lib.evc_workspace_bytes_roots(C.byref(t), 30, 36)
    assert lib.evc_workspace_bytes_roots_batch(C.byref(t), 30, 64, 64) == prev      # 4096 slots
    for count, p in ((0, 1), (1, 0), (4097, 1), (2, 2049), (65, 64)):
        assert lib.evc_workspace_bytes_roots_batch(C.byref(t), 30, count, p) == 0, (count, p)
        assert b"evc_workspace_bytes_roots_batch" in lib.evc_last_error()
