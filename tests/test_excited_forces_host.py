"""CPU tests of the several-roots gradient entry point (include/evcont_hip.h evc_phase_gradient_roots): it is exported
and bound, its output struct has the header's layout, every argument error is caught before anything is enqueued
(rc < 0, message set; dummy device pointers, no stream), and its workspace grows with the slot count."""
import ctypes as C

import numpy as np
import pytest


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


def _geo(natm=2):
    from evcont_amd._lib import Geometry
    return Geometry(natm=natm, enuc=0.0, S=256, hcore=256, eri=256, ipovlp=256, dhcore=256, eri_ip1=256, gnuc=256,
                    aoslices=256)


def test_roots_symbols_exported_and_bound(lib):
    from evcont_amd import _lib
    for s in ("evc_phase_gradient_roots", "evc_workspace_bytes_roots"):
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 10 and lib.evc_abi_version() == 10
    assert hasattr(_lib, "OutputsRoots")


def test_outputs_roots_layout_matches_header():
    from evcont_amd._lib import OutputsRoots
    assert C.sizeof(OutputsRoots) == 3 * 8
    assert [f[0] for f in OutputsRoots._fields_] == ["grad", "d_pred", "g_pred"]


def test_roots_argument_validation_without_gpu(lib):
    from evcont_amd._lib import OutputsRoots, FLAG_IP1_S2KL, FLAG_PARTIAL_RANK, FLAG_ENERGY_ONLY
    t, g = _set(), _geo()
    out = OutputsRoots(grad=256, d_pred=None, g_pred=None)
    big = lib.evc_workspace_bytes_roots(C.byref(t), 2, 3)
    assert big > 0

    def call(coeffs=256, nvec=3, pairs=((0, 0), (1, 1), (0, 2)), out_=out, flags=0, ws=256, ws_bytes=big, geo=g):
        P = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        pp = P.ctypes.data if P.size else None
        return lib.evc_phase_gradient_roots(C.byref(t), C.byref(geo) if geo is not None else None, coeffs, nvec, pp,
                                            P.shape[0], C.byref(out_) if out_ is not None else None, flags, ws,
                                            ws_bytes, None)

    def bad(match, **kw):
        assert call(**kw) < 0, kw
        assert match.encode() in lib.evc_last_error(), (kw, lib.evc_last_error())

    bad("coeffs", coeffs=None)
    bad("geometry", geo=None)
    bad("outputs.grad", out_=None)
    bad("outputs.grad", out_=OutputsRoots(grad=None))
    bad("workspace", ws=None)
    P = np.zeros((1, 2), np.int32)
    assert lib.evc_phase_gradient_roots(C.byref(t), C.byref(g), 256, 3, None, 1, C.byref(out), 0, 256, big, None) < 0
    assert b"pairs" in lib.evc_last_error()
    assert lib.evc_phase_gradient_roots(C.byref(t), C.byref(g), 256, 3, P.ctypes.data, 0, C.byref(out), 0, 256, big,
                                        None) < 0
    assert b"npairs" in lib.evc_last_error()
    P = np.zeros((4097, 2), np.int32)
    assert lib.evc_phase_gradient_roots(C.byref(t), C.byref(g), 256, 3, P.ctypes.data, 4097, C.byref(out), 0, 256,
                                        1 << 62, None) < 0
    assert b"npairs" in lib.evc_last_error()
    bad("outside", pairs=((1, 0),))                 # k > l
    bad("outside", pairs=((0, 3),))                 # l >= nvec
    bad("outside", pairs=((-1, 0),))
    bad("nvec", nvec=21)                            # nvec > T
    bad("nvec", nvec=0)
    bad("PARTIAL_RANK", flags=FLAG_PARTIAL_RANK)
    bad("flags", flags=FLAG_ENERGY_ONLY)
    bad("flags", flags=FLAG_IP1_S2KL | 64)
    bad("too small", ws_bytes=big - 1)
    bad("too small", ws_bytes=lib.evc_workspace_bytes_batch(C.byref(t), 2, 3) - 1)
    bad("misaligned", ws=264)
    bad("geometry", geo=_geo(natm=0))


def test_roots_workspace_grows_with_slots(lib):
    t = _set()
    prev = 0
    for p in (1, 2, 3, 4, 31, 32, 33, 64, 4096):
        b = lib.evc_workspace_bytes_roots(C.byref(t), 30, p)
        assert b > prev, p
        assert b >= lib.evc_workspace_bytes_batch(C.byref(t), 30, p) + p * 30 * 3 * 8
        prev = b
    assert lib.evc_workspace_bytes_roots(C.byref(t), 30, 0) == 0
    assert lib.evc_workspace_bytes_roots(C.byref(t), 30, 4097) == 0
