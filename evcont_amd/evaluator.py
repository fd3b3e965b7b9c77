"""Device-resident continuation evaluator.

``DeviceTRDMs`` uploads the training data (overlap, one- and two-body transition RDMs,
``FCI_EVCont.py:106-131``) ONCE, in whichever of the reference's four layouts the caller
holds (``ab_initio_eigenvector_continuation.py:41-68``), as a ``(rows, ld)`` float64
matrix in HBM with 128-byte-aligned rows.  ``DeviceAO`` holds the AO integrals of one
geometry.  ``ContinuationEvaluator`` owns the workspace and the output buffers and
enqueues the per-geometry DAG through the C ABI (``include/evcont_hip.h``); results stay
on the device until the caller reads them.

PyTorch is used for device memory and streams only.
"""
from __future__ import annotations

import weakref

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import TrdmSet, Geometry, Outputs, check

F64 = torch.float64

# EVCONT_AMD_CHECK_SYM: the compressed layout (EVC_LAYOUT_SYM8) and the packed s4 / s2kl inputs are exact only for AO
# integrals with the index symmetries of real two-electron integrals (include/evcont_hip.h).  "1" (default): every
# evaluator on the compressed layout verifies them on its FIRST call (and every host-side packing helper on its first
# use) and raises instead of returning wrong forces; "2": on every call; "0": never.
_CHECK_SYM = os.environ.get("EVCONT_AMD_CHECK_SYM", "1")
_host_checks_done = set()


def check_integral_symmetry(eri, eri_ip1, n: int, tol: float = 1.0e-9, what: str = "") -> None:
    """Raise ``EvcontHipError`` unless ``eri`` is 8-fold symmetric ((pq|rs) = (qp|rs) = (pq|sr) = (rs|pq)) and
    ``eri_ip1[x,p,q,r,s] = eri_ip1[x,p,q,s,r]``, to ``tol`` relative to the largest element.  Arrays may be numpy or
    torch, with any number of leading batch axes; ``eri`` may be the packed s4 matrix (Ms, Ms) (then only the
    pair-exchange symmetry is left to check), ``eri_ip1`` packed s2kl (nothing left to check) or None."""
    npr = n * (n + 1) // 2
    is_t = torch.is_tensor(eri)
    mx = (lambda x: float(x.abs().max().item())) if is_t else (lambda x: float(np.abs(x).max()))
    bad = []
    if eri is not None and n > 1:
        if eri.shape[-1] == npr and eri.shape[-2] == npr and (eri.ndim < 4 or eri.shape[-3] != n):
            e = eri.reshape(-1, npr, npr)
            sw = (lambda x, a, b: x.transpose(a, b)) if is_t else (lambda x, a, b: np.swapaxes(x, a, b))
            scale = max(mx(e), 1e-300)
            if mx(e - sw(e, 1, 2)) > tol * scale:
                bad.append("eri (packed s4): (pq|rs) != (rs|pq)")
        else:
            e = eri.reshape(-1, n, n, n, n)
            sw = (lambda x, a, b: x.transpose(a, b)) if is_t else (lambda x, a, b: np.swapaxes(x, a, b))
            scale = max(mx(e), 1e-300)
            if mx(e - sw(e, 1, 2)) > tol * scale:
                bad.append("eri: (pq|rs) != (qp|rs)")
            if mx(e - sw(e, 3, 4)) > tol * scale:
                bad.append("eri: (pq|rs) != (pq|sr)")
            if mx(e - sw(sw(e, 1, 3), 2, 4)) > tol * scale:
                bad.append("eri: (pq|rs) != (rs|pq)")
    if eri_ip1 is not None and n > 1 and eri_ip1.shape[-1] == n and eri_ip1.ndim >= 5:
        x = eri_ip1.reshape(-1, n, n, n, n)
        sw = (lambda y, a, b: y.transpose(a, b)) if torch.is_tensor(x) else (lambda y, a, b: np.swapaxes(y, a, b))
        mxx = (lambda y: float(y.abs().max().item())) if torch.is_tensor(x) else (lambda y: float(np.abs(y).max()))
        scale = max(mxx(x), 1e-300)
        if mxx(x - sw(x, 3, 4)) > tol * scale:
            bad.append("eri_ip1[x,p,q,r,s] != eri_ip1[x,p,q,s,r]")
    if bad:
        raise _lib.EvcontHipError(
            "AO integrals without the index symmetries of real two-electron integrals (" + "; ".join(bad) + ")"
            + (f" in {what}" if what else "") + ": the 8-fold compressed t-RDM layout (compress='sym8') and the packed "
            "s4 / s2kl inputs would give wrong energies / forces for them.  Use the reference layouts (compress=None) "
            "for such tensors; EVCONT_AMD_CHECK_SYM=0 disables this check.")


def spot_check_integral_symmetry(eri, eri_ip1, n: int, samples: int = 4096, tol: float = 1.0e-9, what: str = "") -> None:
    """The same test on ``samples`` random index quadruples of full host arrays (numpy): what the host-side packing
    helpers run on EVERY call after their first, complete check -- packing keeps one triangle, so a later geometry (or
    another integral source) without the symmetries could not be noticed afterwards (EVCONT_AMD_CHECK_SYM=0: never)."""
    if n < 2:
        return
    rng = np.random.default_rng()
    p, q, r, t = (rng.integers(0, n, samples) for _ in range(4))
    bad = []
    e = np.asarray(eri)
    if e.ndim >= 4 and e.shape[-1] == n and e.shape[-4] == n:
        e = e.reshape(-1, n, n, n, n)[0]
        v = e[p, q, r, t]
        scale = max(float(np.abs(v).max()), 1e-300)
        if max(np.abs(v - e[q, p, r, t]).max(), np.abs(v - e[p, q, t, r]).max(), np.abs(v - e[r, t, p, q]).max()) > tol * scale:
            bad.append("eri is not 8-fold symmetric")
    if eri_ip1 is not None:
        x = np.asarray(eri_ip1)
        if x.ndim >= 5 and x.shape[-1] == n and x.shape[-2] == n:
            x = x.reshape(-1, n, n, n, n)
            c = rng.integers(0, x.shape[0], samples)
            v = x[c, p, q, r, t]
            scale = max(float(np.abs(v).max()), 1e-300)
            if np.abs(v - x[c, p, q, t, r]).max() > tol * scale:
                bad.append("eri_ip1[x,p,q,r,s] != eri_ip1[x,p,q,s,r]")
    if bad:
        raise _lib.EvcontHipError(
            "AO integrals without the index symmetries of real two-electron integrals (" + "; ".join(bad) + ")"
            + (f" in {what}" if what else "") + ": packing them (s4 / s2kl) would give wrong energies / forces.  Use the "
            "reference layouts (compress=None) for such tensors; EVCONT_AMD_CHECK_SYM=0 disables this check.")


class Sym8NotExact(_lib.EvcontHipError):
    """A training set whose bra<->ket partner blocks differ: the compressed layout would not represent it."""


def _host_check_once(tag: str) -> bool:
    """Whether a host-side packing helper should verify the symmetries now (EVCONT_AMD_CHECK_SYM)."""
    if _CHECK_SYM == "0":
        return False
    if _CHECK_SYM == "2" or tag not in _host_checks_done:
        _host_checks_done.add(tag)
        return True
    return False


def _dev(device=None) -> torch.device:
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.EvcontHipError("no HIP device visible: evcont_amd needs an MI355X (there is no CPU fallback)")
        return torch.device("cuda", torch.cuda.current_device())
    d = torch.device(device)
    if d.type != "cuda":
        raise _lib.EvcontHipError(f"device {d} is not a HIP device")
    return d


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def layout_shape(layout: int, T: int, n: int) -> Tuple[int, int]:
    """(rows, cols) of the matrix view of a two-body t-RDM in the given layout."""
    n2 = n * n
    rows = T * (T + 1) // 2 if layout in (5, 2, _lib.LAYOUT_SYM8) else T * T
    if layout == _lib.LAYOUT_SYM8:
        ms = n * (n + 1) // 2
        return rows, ms * (ms + 1) // 2
    cols = n2 * (n2 + 1) // 2 if layout in (3, 2) else n2 * n2
    return rows, cols


def infer_layout(two_RDM, T: int, n: int) -> int:
    nd = two_RDM.ndim
    assert nd in (6, 5, 3, 2), "two_RDM must have 6, 5, 3 or 2 dimensions"  # evcont.py:70-71
    rows, cols = layout_shape(nd, T, n)
    got = (int(np.prod(two_RDM.shape[: 2 if nd in (6, 3) else 1])), int(np.prod(two_RDM.shape[2 if nd in (6, 3) else 1:])))
    if got != (rows, cols):
        raise ValueError(f"two_RDM shape {tuple(two_RDM.shape)} inconsistent with T={T}, N={n} (layout ndim {nd})")
    return nd


def sym8_column_images(layout: int, n: int):
    """For every column ``u(u+1)/2+v`` of the 8-fold compressed layout (``u = i(i+1)/2+j``, ``i >= j``, ``v`` likewise
    from ``k >= l``, ``u >= v``) the columns of a SOURCE layout (ndim 6/5: ``N^4`` unpacked, 3/2: lower triangle of the
    ``(N^2,N^2)`` matrix) that hold the eight images of ``(i,j,k,l)`` under the index permutations of real
    two-electron integrals: a list of eight int64 arrays.  The compressed entry is the mean over them."""
    iu, ju = np.tril_indices(n)
    U, V = np.tril_indices(len(iu))
    i, j, k, l = iu[U], ju[U], iu[V], ju[V]
    if layout in (3, 2):
        def col(a_, b_, c_, d_):
            R, Cc = a_ * n + b_, c_ * n + d_
            hi, lo = np.maximum(R, Cc).astype(np.int64), np.minimum(R, Cc).astype(np.int64)
            return hi * (hi + 1) // 2 + lo
    else:
        def col(a_, b_, c_, d_):
            return ((a_.astype(np.int64) * n + b_) * n + c_) * n + d_
    images = [(i, j, k, l), (j, i, k, l), (i, j, l, k), (j, i, l, k),
              (k, l, i, j), (l, k, i, j), (k, l, j, i), (l, k, j, i)]
    return [np.ascontiguousarray(col(*im)) for im in images]


def sym8_gather_sums(blk: torch.Tensor, idx) -> torch.Tensor:
    """Per row of ``blk`` (rows of a source layout) the sums over the eight column images ``idx``
    (``sym8_column_images``): eight times the compressed row."""
    acc = blk.index_select(1, idx[0])
    for ix in idx[1:]:
        acc += blk.index_select(1, ix)
    return acc


# Relative tolerance of the bra<->ket test of compress_sym8_, of the largest sum a row can hold (8 x its largest
# element): the images of a bra<->ket symmetric pair are summed in different orders, so they agree to rounding only.
SYM8_BRA_KET_RTOL = 4.0e-13


def sym8_rows_differ(blk_ab: torch.Tensor, sums_ab: torch.Tensor, blk_ba: torch.Tensor, idx,
                     rtol: float = SYM8_BRA_KET_RTOL) -> torch.Tensor:
    """Bool per row: whether the bra<->ket partner rows ``blk_ba`` (blocks (b,a)) compress to something else than
    the rows ``blk_ab`` (blocks (a,b); ``sums_ab = sym8_gather_sums(blk_ab, idx)``), beyond rounding."""
    scale = 8.0 * torch.maximum(blk_ab.abs().amax(1), blk_ba.abs().amax(1))
    return (sym8_gather_sums(blk_ba, idx) - sums_ab).abs().amax(1) > rtol * scale


def _upload_rows(src: np.ndarray, rows: int, cols: int, r0: int, r1: int, device) -> Tuple[torch.Tensor, int]:
    """Copy rows [r0,r1) of the (rows, cols) view of `src` into a zero-padded (r1-r0, ld) device matrix."""
    ld = (cols + 15) // 16 * 16
    out = torch.zeros((max(r1 - r0, 1), ld), dtype=F64, device=device)
    lead = src.shape[: src.ndim - (4 if src.ndim in (6, 5) else 1)]
    step = max(1, (256 << 20) // (cols * 8))
    for a in range(r0, r1, step):
        b = min(r1, a + step)
        idx = np.unravel_index(np.arange(a, b), lead)
        block = np.ascontiguousarray(src[idx], dtype=np.float64).reshape(b - a, cols)
        out[a - r0:b - r0, :cols].copy_(torch.from_numpy(block), non_blocking=False)
    return out, ld


def _pad_even(mat: torch.Tensor) -> torch.Tensor:
    """(rows, cols) -> contiguous (rows, ld) with ld even (16-byte aligned rows), zero padded."""
    rows, cols = mat.shape
    if cols % 2 == 0:
        return mat.contiguous()
    out = torch.zeros((rows, cols + 1), dtype=F64, device=mat.device)
    out[:, :cols].copy_(mat)
    return out


class DeviceTRDMs:
    """Training data resident in HBM.  ``row_range`` selects the slice of two-body rows this
    rank owns (pair sharding); the one-body t-RDM and S are replicated."""

    def __init__(self, one_RDM, two_RDM, S, device=None, row_range: Optional[Tuple[int, int]] = None,
                 compress: Optional[str] = None):
        """``compress="sym8"``: keep only the 8-fold symmetrised part of the two-body t-RDMs
        (``compress_sym8_``, include/evcont_hip.h ``EVC_LAYOUT_SYM8``)."""
        self.device = _dev(device)
        one_RDM = np.asarray(one_RDM) if not torch.is_tensor(one_RDM) else one_RDM
        S = np.asarray(S) if not torch.is_tensor(S) else S
        T = int(S.shape[0])
        n = int(one_RDM.shape[-1])
        assert tuple(one_RDM.shape) == (T, T, n, n), "one_RDM must be (T,T,N,N)"
        self.T, self.n = T, n
        if torch.is_tensor(two_RDM):
            self.layout = infer_layout(two_RDM, T, n)
            rows, cols = layout_shape(self.layout, T, n)
            r0, r1 = row_range if row_range is not None else (0, rows)
            mat = two_RDM.reshape(rows, cols)[r0:r1].to(self.device, F64)
            ld = (cols + 15) // 16 * 16
            self.two = torch.zeros((max(r1 - r0, 1), ld), dtype=F64, device=self.device)
            self.two[: r1 - r0, :cols].copy_(mat)
        else:
            two_RDM = np.asarray(two_RDM)
            self.layout = infer_layout(two_RDM, T, n)
            rows, cols = layout_shape(self.layout, T, n)
            r0, r1 = row_range if row_range is not None else (0, rows)
            self.two, ld = _upload_rows(two_RDM, rows, cols, r0, r1, self.device)
        assert 0 <= r0 <= r1 <= rows
        self.rows_total, self.cols, self.ld = rows, cols, ld
        self.row_offset, self.rows_local = r0, r1 - r0
        as_t = lambda x: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)))
        self.one = _pad_even(as_t(one_RDM).to(self.device, F64).reshape(T * T, n * n))
        self.S = as_t(S).to(self.device, F64).contiguous()
        self.cstruct = TrdmSet(n=n, ntrain=T, layout=self.layout, reserved=0, rows2=self.rows_local,
                               row_offset=self.row_offset, rows2_total=rows, cols2=cols, ld2=ld,
                               ld1=self.one.shape[1],
                               two_rdm=self.two.data_ptr(), one_rdm=self.one.data_ptr(),
                               s_train=self.S.data_ptr())
        if compress is not None:
            if compress != "sym8":
                raise ValueError(f"unknown t-RDM compression {compress!r} (known: 'sym8')")
            self.compress_sym8_()

    def compress_sym8_(self) -> "DeviceTRDMs":
        """Replace the resident two-body t-RDMs by their 8-fold compressed form (``EVC_LAYOUT_SYM8``,
        in place): per pair ``a >= b`` the mean of ``Gamma`` over the index permutations under which real
        two-electron integrals are invariant, stored once per class -- N(N+1)/2 (N(N+1)/2 + 1)/2 columns
        instead of N^2 (N^2+1)/2 (3.7x fewer bytes at N = 30).

        Exact (to rounding) for the Hermitian continuation whenever the AO integrals carry those symmetries
        (``eri`` 8-fold, ``eri_ip1`` symmetric in its last two indices: every PySCF ``int2e`` /
        ``int2e_ip1``); ``predicted_two_rdm`` then is the symmetrised 2-RDM.  Not for ``hermitian=False``.

        The compressed layout keeps the pairs ``a >= b`` only, with weight ``2 c_a c_b``: that is exact only when the
        block ``(b,a)`` compresses to the same row as ``(a,b)`` (every container of the reference stores bra<->ket
        symmetric data).  For the (T,T,...) layouts (ndim 6 / 3), which hold both blocks, the ``(b,a)`` rows are
        compressed by the same gather and compared with the ``(a,b)`` rows on the device; a training set that fails
        raises ``Sym8NotExact`` and is left as it was.  (The pair layouts 5 / 2 hold one block per pair: nothing to
        compare.)"""
        if self.layout == _lib.LAYOUT_SYM8:
            return self
        T, n, d = self.T, self.n, self.device
        if self.layout in (6, 3):
            if (self.row_offset, self.rows_local) != (0, self.rows_total):
                raise ValueError("compress_sym8_: shard the pair layouts (5, 2), not the (T,T,...) ones")
            a, b = np.tril_indices(T)
            src = torch.from_numpy((a * T + b).astype(np.int64)).to(d)
            src_ba = torch.from_numpy((b * T + a).astype(np.int64)).to(d)
            r0 = 0
        else:
            src = torch.arange(self.rows_local, dtype=torch.int64, device=d)
            src_ba = None
            r0 = self.row_offset
        idx = [torch.from_numpy(ix).to(d) for ix in sym8_column_images(self.layout, n)]
        rows8, cols8 = layout_shape(_lib.LAYOUT_SYM8, T, n)
        ld8 = (cols8 + 15) // 16 * 16
        nloc = int(src.numel())
        out = torch.zeros((max(nloc, 1), ld8), dtype=F64, device=d)
        step = max(1, (256 << 20) // (self.ld * 8))
        for a0 in range(0, nloc, step):
            blk = self.two.index_select(0, src[a0:a0 + step])
            acc = sym8_gather_sums(blk, idx)
            if src_ba is not None:
                blk_ba = self.two.index_select(0, src_ba[a0:a0 + step])
                bad = sym8_rows_differ(blk, acc, blk_ba, idx)
                if bool(bad.any()):
                    r = a0 + int(torch.nonzero(bad)[0, 0].item())
                    raise Sym8NotExact(
                        f"compress='sym8': the two-body t-RDM block ({int(a[r])},{int(b[r])}) and its bra<->ket "
                        f"partner ({int(b[r])},{int(a[r])}) differ after the 8-fold symmetrisation: the compressed "
                        "layout keeps one block per pair and would give wrong forces for this training set.  Use the "
                        "layout the data is held in (compress=None).")
                del blk_ba
            out[a0:a0 + acc.shape[0], :cols8] = acc * 0.125
            del blk, acc
        self.two, self.layout = out, _lib.LAYOUT_SYM8
        self.rows_total, self.cols, self.ld = rows8, cols8, ld8
        self.row_offset, self.rows_local = r0, nloc
        self.cstruct = TrdmSet(n=n, ntrain=T, layout=self.layout, reserved=0, rows2=self.rows_local,
                               row_offset=self.row_offset, rows2_total=rows8, cols2=cols8, ld2=ld8,
                               ld1=self.one.shape[1],
                               two_rdm=self.two.data_ptr(), one_rdm=self.one.data_ptr(),
                               s_train=self.S.data_ptr())
        return self

    @classmethod
    def from_device_rows(cls, one_RDM: torch.Tensor, two_rows: torch.Tensor, S: torch.Tensor, layout: int,
                         row_offset: int = 0, rows_total: Optional[int] = None) -> "DeviceTRDMs":
        """Adopt two-body rows already on the device: ``two_rows`` is the (rows_local, cols) slice
        [row_offset, row_offset+rows_local) of the layout's matrix view (no host round trip)."""
        self = cls.__new__(cls)
        self.device = two_rows.device
        T, n = int(S.shape[0]), int(one_RDM.shape[-1])
        self.T, self.n, self.layout = T, n, int(layout)
        rows, cols = layout_shape(self.layout, T, n)
        if rows_total is not None:
            assert rows_total == rows
        assert two_rows.ndim == 2 and two_rows.shape[1] == cols and two_rows.dtype == F64
        r0, r1 = int(row_offset), int(row_offset) + int(two_rows.shape[0])
        assert 0 <= r0 <= r1 <= rows
        ld = (cols + 15) // 16 * 16
        if ld == cols and two_rows.is_contiguous() and two_rows.shape[0] > 0:
            self.two = two_rows
        else:
            self.two = torch.zeros((max(r1 - r0, 1), ld), dtype=F64, device=self.device)
            self.two[: r1 - r0, :cols].copy_(two_rows)
        self.rows_total, self.cols, self.ld = rows, cols, ld
        self.row_offset, self.rows_local = r0, r1 - r0
        self.one = _pad_even(one_RDM.to(self.device, F64).reshape(T * T, n * n))
        self.S = S.to(self.device, F64).contiguous()
        self.cstruct = TrdmSet(n=n, ntrain=T, layout=self.layout, reserved=0, rows2=self.rows_local,
                               row_offset=self.row_offset, rows2_total=rows, cols2=cols, ld2=ld,
                               ld1=self.one.shape[1],
                               two_rdm=self.two.data_ptr(), one_rdm=self.one.data_ptr(),
                               s_train=self.S.data_ptr())
        return self

    @classmethod
    def from_padded_rows(cls, one_RDM, two_padded: torch.Tensor, S, layout: int) -> "DeviceTRDMs":
        """Adopt, WITHOUT copying, an already padded two-body matrix of a pair layout (pack2, pair5 or sym8):
        ``two_padded`` is a ``(rows, ld)`` device view of unit column stride whose first ``cols`` columns hold the
        layout's rows and the others zeros (``ld`` a multiple of 16), e.g. the leading rows of a larger matrix
        (``resident.ResidentTRDMs``).  ``one_RDM (T,T,N,N)`` and ``S (T,T)``: numpy or tensors, copied."""
        self = cls.__new__(cls)
        self.device = two_padded.device
        T, n = int(S.shape[0]), int(one_RDM.shape[-1])
        self.T, self.n, self.layout = T, n, int(layout)
        rows, cols = layout_shape(self.layout, T, n)
        # the matrix is adopted as it is and reaches the library as a pointer with this pitch: refuse, not assert
        ok = (self.layout in (5, 2, _lib.LAYOUT_SYM8) and two_padded.dtype == F64 and two_padded.dim() == 2
              and two_padded.device.type == "cuda" and tuple(one_RDM.shape) == (T, T, n, n))
        ld = int(two_padded.shape[1]) if ok else 0
        ok = (ok and two_padded.shape[0] == rows and two_padded.stride(1) == 1 and (rows == 1 or two_padded.stride(0) == ld)
              and ld % 16 == 0 and ld >= cols and two_padded.data_ptr() % 16 == 0)
        if not ok:
            raise _lib.EvcontHipError(
                f"DeviceTRDMs.from_padded_rows: need a float64 device matrix of {rows} rows whose pitch is its width, a "
                f"multiple of 16 and at least {cols} (layout {self.layout}, T={T}, N={n}), with unit column stride and "
                f"16-byte aligned; got shape {tuple(two_padded.shape)}, strides {tuple(two_padded.stride())}, "
                f"{two_padded.dtype} on {two_padded.device}")
        self.two = two_padded
        self.rows_total, self.cols, self.ld = rows, cols, ld
        self.row_offset, self.rows_local = 0, rows
        as_t = lambda x: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)))
        self.one = _pad_even(as_t(one_RDM).to(self.device, F64).reshape(T * T, n * n))
        self.S = as_t(S).to(self.device, F64).contiguous()
        self.cstruct = TrdmSet(n=n, ntrain=T, layout=self.layout, reserved=0, rows2=rows, row_offset=0, rows2_total=rows,
                               cols2=cols, ld2=ld, ld1=self.one.shape[1], two_rdm=self.two.data_ptr(),
                               one_rdm=self.one.data_ptr(), s_train=self.S.data_ptr())
        return self

    @property
    def nbytes_streamed_per_pass(self) -> int:
        """Algorithmic bytes one pass over the local two-body rows reads."""
        return self.rows_local * self.cols * 8


@dataclass
class DeviceAO:
    """AO integrals of one geometry on the device (fields as in include/evcont_hip.h evc_geometry)."""
    S: torch.Tensor
    hcore: torch.Tensor
    eri: torch.Tensor
    enuc: float
    natm: int = 0
    ipovlp: Optional[torch.Tensor] = None
    dhcore: Optional[torch.Tensor] = None
    eri_ip1: Optional[torch.Tensor] = None
    gnuc: Optional[torch.Tensor] = None
    aoslices: Optional[torch.Tensor] = None
    ip1_s2kl: bool = False   # eri_ip1 is (3,N,N,N(N+1)/2): packed in its last two indices (EVC_FLAG_IP1_S2KL)
    eri_s4: bool = False     # eri is (N(N+1)/2, N(N+1)/2): packed in both index pairs (EVC_FLAG_ERI_S4)

    @property
    def nao(self) -> int:
        return int(self.S.shape[0])

    @staticmethod
    def from_arrays(ao, device=None, energy_only: bool = False, pack_ip1: bool = False,
                    pack_eri: bool = False) -> "DeviceAO":
        """From any object with the AOArrays fields (numpy).  ``pack_ip1``: upload ``eri_ip1`` packed in its last
        two AO indices (half the bytes; what ``mol.intor("int2e_ip1", aosym="s2kl")`` returns -- an ``eri_ip1`` that
        already has that shape is taken as is); ``pack_eri``: upload ``eri`` packed in both index pairs (a quarter of
        the bytes, ``aosym="s4"``; a 2-D ``eri`` of that shape is taken as is).  Both only for evaluators on the
        compressed ``sym8`` layout."""
        d = _dev(device)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(d)
        n = int(np.asarray(ao.S).shape[0])
        npr = n * (n + 1) // 2
        eri = np.asarray(ao.eri)
        s4 = eri.ndim == 2 and eri.shape == (npr, npr) and n > 1
        if (pack_eri or pack_ip1) and not energy_only:
            # complete check at the first use (per orbital count), a random sample on every later call
            if _host_check_once(f"DeviceAO.from_arrays/{n}"):
                check_integral_symmetry(eri, np.asarray(ao.eri_ip1), n, what="DeviceAO.from_arrays(pack_...=True)")
            elif _CHECK_SYM != "0":
                spot_check_integral_symmetry(eri, ao.eri_ip1, n, what="DeviceAO.from_arrays(pack_...=True)")
        if pack_eri and not s4:
            iu, ju = np.tril_indices(n)
            eri = eri.reshape(n, n, n, n)[iu, ju][:, iu, ju]
            s4 = True
        out = DeviceAO(S=up(ao.S), hcore=up(ao.hcore), eri=up(eri), enuc=float(ao.enuc),
                       natm=int(np.asarray(ao.aoslices).shape[0]), eri_s4=s4)
        if not energy_only:
            ip1 = np.asarray(ao.eri_ip1)
            n = out.nao
            if ip1.ndim == 4 or (ip1.ndim == 3 and ip1.shape[-1] == n * (n + 1) // 2):   # already s2kl
                ip1 = ip1.reshape(3, n, n, n * (n + 1) // 2)
                out.ip1_s2kl = True
            elif pack_ip1:
                iu, ju = np.tril_indices(n)
                ip1 = ip1.reshape(3, n, n, n, n)[:, :, :, iu, ju]
                out.ip1_s2kl = True
            out.ipovlp, out.dhcore, out.eri_ip1, out.gnuc = up(ao.ipovlp), up(ao.dhcore), up(ip1), up(ao.gnuc)
            out.aoslices = torch.from_numpy(np.ascontiguousarray(ao.aoslices, dtype=np.int64)).to(d)
        return out

    def packed_ip1(self, eri: bool = False) -> "DeviceAO":
        """A copy (sharing every other array) whose ``eri_ip1`` is packed in its last two indices (and, with
        ``eri=True``, whose ``eri`` is packed in both index pairs), gathered on the device from the full arrays."""
        n = self.nao
        iu, ju = np.tril_indices(n)
        idx = torch.from_numpy((iu * n + ju).astype(np.int64)).to(self.S.device)
        ip1, s2kl = self.eri_ip1, self.ip1_s2kl
        if ip1 is not None and not s2kl:
            ip1, s2kl = ip1.reshape(3, n, n, n * n).index_select(3, idx).contiguous(), True
        e, s4 = self.eri, self.eri_s4
        if eri and not s4:
            e, s4 = e.reshape(n * n, n * n).index_select(0, idx).index_select(1, idx).contiguous(), True
        return DeviceAO(S=self.S, hcore=self.hcore, eri=e, enuc=self.enuc, natm=self.natm, ipovlp=self.ipovlp,
                        dhcore=self.dhcore, eri_ip1=ip1, gnuc=self.gnuc, aoslices=self.aoslices, ip1_s2kl=s2kl,
                        eri_s4=s4)

    def cstruct(self) -> Geometry:
        p = lambda t: (t.data_ptr() if t is not None else None)
        return Geometry(natm=self.natm, reserved=0, enuc=self.enuc, S=p(self.S), hcore=p(self.hcore),
                        eri=p(self.eri), ipovlp=p(self.ipovlp), dhcore=p(self.dhcore), eri_ip1=p(self.eri_ip1),
                        gnuc=p(self.gnuc), aoslices=p(self.aoslices))


@dataclass
class DeviceAOBatch:
    """AO integrals of ``count`` geometries of one molecule, stacked along a leading batch axis
    (include/evcont_hip.h ``evc_geometry_batch``)."""
    S: torch.Tensor          # (G,N,N)
    hcore: torch.Tensor      # (G,N,N)
    eri: torch.Tensor        # (G,N,N,N,N)
    enuc: torch.Tensor       # (G,)
    natm: int
    ipovlp: Optional[torch.Tensor] = None    # (G,3,N,N)
    dhcore: Optional[torch.Tensor] = None    # (G,A,3,N,N)
    eri_ip1: Optional[torch.Tensor] = None   # (G,3,N,N,N,N)
    gnuc: Optional[torch.Tensor] = None      # (G,A,3)
    aoslices: Optional[torch.Tensor] = None  # (A,2) int64, shared
    ip1_s2kl: bool = False                   # eri_ip1 is (G,3,N,N,N(N+1)/2) (EVC_FLAG_IP1_S2KL)
    eri_s4: bool = False                     # eri is (G,N(N+1)/2,N(N+1)/2) (EVC_FLAG_ERI_S4)

    @property
    def count(self) -> int:
        return int(self.S.shape[0])

    @property
    def nao(self) -> int:
        return int(self.S.shape[1])

    @staticmethod
    def stack(aos) -> "DeviceAOBatch":
        """Stack single-geometry ``DeviceAO`` objects (device-to-device copies)."""
        aos = list(aos)
        assert len({(bool(a.ip1_s2kl), bool(a.eri_s4)) for a in aos}) == 1, "mixed full / packed integrals in one batch"
        d = aos[0].S.device
        st = lambda name: (torch.stack([getattr(a, name) for a in aos]).contiguous()
                           if getattr(aos[0], name) is not None else None)
        return DeviceAOBatch(S=st("S"), hcore=st("hcore"), eri=st("eri"),
                             enuc=torch.tensor([a.enuc for a in aos], dtype=F64, device=d), natm=aos[0].natm,
                             ipovlp=st("ipovlp"), dhcore=st("dhcore"), eri_ip1=st("eri_ip1"), gnuc=st("gnuc"),
                             aoslices=aos[0].aoslices, ip1_s2kl=bool(aos[0].ip1_s2kl), eri_s4=bool(aos[0].eri_s4))

    @staticmethod
    def from_arrays(ao_list, device=None, energy_only: bool = False, pack_ip1: bool = False,
                    pack_eri: bool = False) -> "DeviceAOBatch":
        return DeviceAOBatch.stack([DeviceAO.from_arrays(a, device, energy_only, pack_ip1, pack_eri) for a in ao_list])

    def cstruct(self) -> "_lib.GeometryBatch":
        p = lambda t: (t.data_ptr() if t is not None else None)
        return _lib.GeometryBatch(natm=self.natm, count=self.count, enuc=p(self.enuc), S=p(self.S),
                                  hcore=p(self.hcore), eri=p(self.eri), ipovlp=p(self.ipovlp), dhcore=p(self.dhcore),
                                  eri_ip1=p(self.eri_ip1), gnuc=p(self.gnuc), aoslices=p(self.aoslices))


def _check_sym_first_call(ev, ao, energy_only: bool = False) -> None:
    """First call of an evaluator on the compressed layout (every call with EVCONT_AMD_CHECK_SYM=2): verify on the
    device, on the evaluator's stream, that the integrals have the symmetries the layout relies on."""
    if ev.t.layout != _lib.LAYOUT_SYM8 or _CHECK_SYM == "0" or (_CHECK_SYM != "2" and getattr(ev, "_sym_checked", False)):
        return
    if torch.cuda.is_current_stream_capturing():
        return
    st = ev.stream if ev.stream is not None else torch.cuda.current_stream(ev.t.device)
    with torch.cuda.stream(st):
        check_integral_symmetry(ao.eri, None if energy_only else ao.eri_ip1, ev.t.n, what=type(ev).__name__)
    ev._sym_checked = True


def _ip1_flag(trdms: "DeviceTRDMs", ao) -> int:
    """EVC_FLAG_IP1_S2KL / EVC_FLAG_ERI_S4 for geometries whose integrals are handed over packed."""
    f = (_lib.FLAG_IP1_S2KL if getattr(ao, "ip1_s2kl", False) else 0) | \
        (_lib.FLAG_ERI_S4 if getattr(ao, "eri_s4", False) else 0)
    if f and (trdms.layout != _lib.LAYOUT_SYM8 or trdms.n > 64):
        raise _lib.EvcontHipError("packed (s2kl / s4) integrals need training data in the compressed sym8 layout and "
                                  "N <= 64 (DeviceAO.from_arrays(..., pack_ip1=False, pack_eri=False) otherwise)")
    if trdms.n > 32 and f not in (0, _lib.FLAG_IP1_S2KL | _lib.FLAG_ERI_S4) and getattr(ao, "eri_ip1", None) is not None:
        raise _lib.EvcontHipError("N > 32: int2e and int2e_ip1 are handed over both packed (s4 and s2kl) or both full")
    return f


def _eig_nonhermitian(H: np.ndarray, S: np.ndarray, layout: int):
    """The reference's non-Hermitian branch (:50-51,67-68,76-81) on the subspace matrix assembled by the
    device: pair layouts carry the two-body part in the lower triangle only, so the upper one is filled
    from it first; then ``scipy.linalg.eig(H, S)`` (a T x T problem, solved on the host exactly as the
    reference does) and the |Im| < 1e-5 filter."""
    import scipy.linalg
    H = np.array(H, dtype=np.float64)
    if layout in (5, 2):
        iu = np.triu_indices(H.shape[0])
        H[iu] = H.T[iu]
    vals, vecs = scipy.linalg.eig(H, np.asarray(S, dtype=np.float64))
    keep = np.abs(vals.imag) < 1.0e-5
    return vals[keep], vecs[:, keep]


def _select(vals, vecs, nroots, ground_state):
    if ground_state:
        k = int(np.argmin(vals.real))
        return float(vals[k].real), np.array(vecs[:, k].real)
    assert vals.shape[0] >= nroots                   # reference :166
    order = np.argsort(vals.real)[:nroots]
    return np.array(vals[order].real), np.array(vecs[:, order].real.T)


def _check_nonhermitian(t: "DeviceTRDMs") -> None:
    """hermitian=False solves the subspace matrix of the caller's layout, assembled from the complete t-RDM."""
    if t.layout == _lib.LAYOUT_SYM8:
        raise _lib.EvcontHipError("hermitian=False needs the training data in the layout the caller holds, not sym8")
    if (t.row_offset, t.rows_local) != (0, t.rows_total):
        raise _lib.EvcontHipError("hermitian=False needs the complete t-RDM on this device")


class _EvaluatorBase:
    """What ``ContinuationEvaluator`` (one geometry per call) and ``BatchedEvaluator`` (``count`` geometries per call)
    share: the workspace, the stream every call is enqueued on, and every library call that exists for one geometry
    and for a batch.  A subclass names its library calls by ``_suffix`` ("" / "_batch"), the leading shape of its
    per-geometry arrays by ``_lead`` and the form it hands rows of the subspace matrix over in by ``_rows_args``."""
    _suffix = ""
    _nan_message = ""

    @property
    def _lead(self) -> tuple:
        return ()

    def _workspace_bytes(self, name: str, *args) -> int:
        """``name + _suffix`` (an ``evc_workspace_bytes*`` query) for this evaluator's geometries and ``args``."""
        nbytes = getattr(self.lib, name + self._suffix)(C.byref(self.t.cstruct), self.natm, *self._lead, *args)
        if nbytes == 0:
            raise _lib.EvcontHipError(f"{name}{self._suffix}: " + self.lib.evc_last_error().decode())
        return nbytes

    def _set_workspace(self, ws: torch.Tensor) -> None:
        self.ws, self.ws_bytes = ws, int(ws.numel())
        # (the library may attach a side stream to the workspace, include/evcont_hip.h evc_release_workspace)
        self._ws_release = weakref.finalize(self, self.lib.evc_release_workspace, self.ws.data_ptr())
        self._ws_release.atexit = False

    def _init_workspace(self) -> None:
        # zero-filled once: the cached factorisation of S_train in it is recognised by content (a recycled allocator
        # block must not look like a hit)
        nbytes = self._workspace_bytes("evc_workspace_bytes")
        self._set_workspace(torch.zeros(nbytes, dtype=torch.uint8, device=self.t.device))

    def _grow_workspace(self, nbytes: int) -> None:
        """Enlarge the workspace to ``nbytes`` (never shrinks).  The geometries' slots keep their place and contents
        (the cached factorisation of S_train, the warm-start eigenvectors); the rest is zero-filled."""
        if nbytes <= self.ws_bytes:
            return
        st = self._stream()
        self._ws_release()          # waits for a side-stream launch into the old workspace, drops its events
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.t.device)
        with torch.cuda.stream(st):
            ws[: self.ws_bytes].copy_(self.ws)
        st.synchronize()
        self._set_workspace(ws)

    def _stream(self) -> "torch.cuda.Stream":
        return self.stream if self.stream is not None else torch.cuda.current_stream(self.t.device)

    def _sp(self) -> int:
        return self._stream().cuda_stream

    def synchronize(self) -> None:
        self._stream().synchronize()

    def _init_state(self, trdms: DeviceTRDMs, natm: int, stream, warm_start: bool) -> None:
        self.t, self.natm, self.stream, self.warm_start = trdms, int(natm), stream, bool(warm_start)
        self._primed = False         # the workspace holds the eigenvectors of a converged Hermitian solve (warm start)
        self._loewdin_done = False   # phase_loewdin has run: the next phase A / full call skips the Loewdin step
        self.lib = _lib.load()
        self._init_workspace()

    def _call(self, name: str, *args, sp: Optional[int] = None) -> None:
        """``name + _suffix(training set, *args, workspace, its size, stream)``; raises on a non-zero return code."""
        name += self._suffix
        check(getattr(self.lib, name)(C.byref(self.t.cstruct), *args, self.ws.data_ptr(), self.ws_bytes,
                                      self._sp() if sp is None else sp), name)

    def _flags(self, flags: int = 0, loewdin: bool = False) -> int:
        """Flag word of a call that solves something: ``flags`` plus the warm start when the workspace is primed, and
        for the calls that run the Loewdin step (``loewdin``) the note that ``phase_loewdin`` has done it already."""
        if self.warm_start and self._primed:
            flags |= _lib.FLAG_WARM_START
        if loewdin and self._loewdin_done:
            flags |= _lib.FLAG_LOEWDIN_DONE
            self._loewdin_done = False
        return flags

    def _raise_if_nan(self, e) -> None:
        if not np.all(np.isfinite(e)):
            raise np.linalg.LinAlgError(self._nan_message)

    def _check_ao(self, ao) -> None:
        pass

    def enqueue(self, ao, nroots: int = 1, energy_only: bool = False) -> None:
        """Enqueue one evaluation (``evc_energy_with_grad`` / ``_batch``) on this evaluator's stream; no
        synchronisation."""
        self._check_ao(ao)
        _check_sym_first_call(self, ao, energy_only)
        g = ao.cstruct()
        flags = self._flags((_lib.FLAG_ENERGY_ONLY if energy_only else 0) | _ip1_flag(self.t, ao), loewdin=True)
        self._call("evc_energy_with_grad", C.byref(g), C.byref(self.out), int(nroots), flags)
        self._primed = True

    # -- phase API for the pair-sharded multi-GPU host (evcont_amd/distributed.py); phase_hamiltonian: the subclasses --
    def phase_solve(self, ao, rows_all: torch.Tensor, nroots: int = 1) -> None:
        g = ao.cstruct()
        self._call("evc_phase_solve", C.byref(g), *self._rows_args(rows_all, self.t.rows_total), C.byref(self.out),
                   int(nroots), self._flags())
        self._primed = True

    def phase_gradient(self, ao, partial_rank: bool) -> None:
        g = ao.cstruct()
        self._call("evc_phase_gradient", C.byref(g), C.byref(self.out),
                   (_lib.FLAG_PARTIAL_RANK if partial_rank else 0) | _ip1_flag(self.t, ao))

    def _host_eigs(self, ao, rows: torch.Tensor) -> list:
        """hermitian=False: phase B on the ``rows`` of phase A assembles H(R) of every geometry on the device as for
        the Hermitian branch; then the reference's ``eig`` branch on the host (``_eig_nonhermitian``), one
        (values, vectors) pair per geometry.  (The caller has run ``_check_nonhermitian`` before phase A.)"""
        self.phase_solve(ao, rows, 1)
        self.synchronize()
        self._primed = False      # the workspace no longer holds a converged Hermitian solve
        S, T = self.t.S.cpu().numpy(), self.t.T
        return [_eig_nonhermitian(H, S, self.t.layout) for H in self.hmat.cpu().numpy().reshape(-1, T, T)]

    def _gradient_roots(self, ao, nroots: int, pairs, want_d: bool, want_g: bool, hermitian: bool):
        """Energies of the lowest ``nroots`` roots, then one gradient slot per root pair of ``pairs`` (default: the
        diagonal) in one pass of the gradient chain (``evc_phase_gradient_roots`` / ``_batch``).  Returns the host
        energies and coefficient rows and the device ``grads``, ``D`` and ``Gamma`` of the slots, with the leading
        shape ``(P,) + _lead``."""
        T, n = self.t.T, self.t.n
        nroots = int(nroots)
        if not 1 <= nroots <= T:
            raise ValueError(f"nroots={nroots} out of range 1..{T}")
        if pairs is None:
            pairs = [(k, k) for k in range(nroots)]
        P = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        npairs = P.shape[0]
        self._grow_workspace(self._workspace_bytes("evc_workspace_bytes_roots", npairs))
        if hermitian:
            self.enqueue(ao, nroots, energy_only=True)
            coeffs = self.coeffs                      # rows 0 .. nroots-1 of every geometry as the solver wrote them
        else:
            e, c, coeffs = self._host_coeffs(ao, nroots)
        d, lead = self.t.device, (npairs,) + self._lead
        grads = torch.zeros(lead + (max(self.natm, 1), 3), dtype=F64, device=d)
        D = torch.zeros(lead + (n, n), dtype=F64, device=d) if want_d else None
        Gm = torch.zeros(lead + (n, n, n, n), dtype=F64, device=d) if want_g else None
        p = lambda t: (t.data_ptr() if t is not None else None)
        out = _lib.OutputsRoots(grad=p(grads), d_pred=p(D), g_pred=p(Gm))
        g = ao.cstruct()
        self._call("evc_phase_gradient_roots", C.byref(g), coeffs.data_ptr(), nroots, P.ctypes.data, npairs,
                   C.byref(out), _ip1_flag(self.t, ao) & _lib.FLAG_IP1_S2KL)
        self.synchronize()        # (coeffs of the eig branch live until here)
        if hermitian:
            e = self.energy[..., :nroots].cpu().numpy().copy()
            self._raise_if_nan(e[..., 0])
            c = self.coeffs[..., :nroots, :].cpu().numpy().copy()
        return e, c, grads, D, Gm


    # -- observables of several roots (evc_properties_roots_batch; one geometry: count = 1) ------------------------
    def _properties_device(self, ao, coeffs: torch.Tensor, nvec: int, P: np.ndarray, dip, charges, coords, origin,
                           want=("dipole", "mulliken", "loewdin")) -> dict:
        """Enqueue ``evc_properties_roots_batch`` on the workspace as the energy call left it (phases A+B of ``ao``),
        for the rows 0 .. nvec-1 of ``coeffs`` and the root pairs ``P`` (npairs,2) int32.  ``want``: among "d_oao",
        "d_ao", "dipole", "mulliken", "loewdin".  Returns the device tensors, leading shape ``(npairs,) + _lead``,
        populations not charges; no synchronisation."""
        t, d = self.t, self.t.device
        if self.natm < 1:
            raise _lib.EvcontHipError("properties need an evaluator built with natm >= 1")
        count = int(np.prod(self._lead, dtype=np.int64)) if self._lead else 1
        npairs, n, A = int(P.shape[0]), t.n, self.natm
        dev = lambda x, shape: (None if x is None else
                                (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)))
                                .to(device=d, dtype=F64).reshape(shape).contiguous())
        need_dip = "dipole" in want
        dip_d = dev(dip, self._lead + (3, n, n)) if need_dip else None
        z_d = dev(charges, (A,)) if need_dip else None
        r_d = dev(coords, self._lead + (A, 3)) if need_dip else None
        if need_dip and (dip_d is None or z_d is None or r_d is None):
            raise ValueError("the dipole needs dip, charges and coords")
        need_slices = "mulliken" in want or "loewdin" in want
        if need_slices and ao.aoslices is None:
            raise ValueError("populations need the geometry's aoslices")
        nbytes = self.lib.evc_properties_workspace_bytes(n, t.T, A, count, npairs)
        if nbytes == 0:
            raise _lib.EvcontHipError("evc_properties_workspace_bytes: " + self.lib.evc_last_error().decode())
        scratch = getattr(self, "_prop_scratch", None)
        if scratch is None or scratch.numel() < nbytes:
            scratch = self._prop_scratch = torch.empty(nbytes, dtype=torch.uint8, device=d)
        lead = (npairs,) + self._lead
        shapes = {"d_oao": (n, n), "d_ao": (n, n), "dipole": (3,), "mulliken": (A,), "loewdin": (A,)}
        res = {k: torch.zeros(lead + shapes[k], dtype=F64, device=d) for k in shapes if k in want}
        p = lambda x: (x.data_ptr() if x is not None else None)
        pin = _lib.PropertyInputs(natm=A, count=count, S=p(ao.S), dip=p(dip_d), aoslices=p(ao.aoslices), charges=p(z_d),
                                  coords=p(r_d), origin=(C.c_double * 3)(*[float(x) for x in origin]))
        pout = _lib.PropertyOutputs(**{k: p(res.get(k)) for k in shapes})
        P = np.ascontiguousarray(P, dtype=np.int32)
        check(self.lib.evc_properties_roots_batch(C.byref(t.cstruct), C.byref(pin), coeffs.data_ptr(), int(nvec),
                                                  P.ctypes.data, npairs, C.byref(pout), self.ws.data_ptr(), self.ws_bytes,
                                                  scratch.data_ptr(), int(scratch.numel()), self._sp()),
              "evc_properties_roots_batch")
        res["_keep"] = (dip_d, z_d, r_d, coeffs)     # inputs live until the caller synchronises
        return res

    def _multistate_properties(self, ao, nroots: int, pairs, dip, charges, coords, origin, hermitian: bool,
                               return_dm_ao: bool, return_forces: bool, observables):
        """What ``multistate_properties`` of both evaluators does; geometry axis (if any) still behind the pair axis."""
        T = self.t.T
        nroots = int(nroots)
        if not 1 <= nroots <= T:
            raise ValueError(f"nroots={nroots} out of range 1..{T}")
        if pairs is None:
            pairs = [(k, k) for k in range(nroots)]
        P = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        grads = None
        if return_forces:
            # one solve: the gradient call and the properties call read the same phases A+B
            e, c, grads, _, _ = self._gradient_roots(ao, nroots, P, False, False, hermitian)
            if hermitian:
                coeffs = self.coeffs
            else:
                blocks = np.zeros(self._lead + (T, T))
                blocks[..., :nroots, :] = c
                coeffs = torch.from_numpy(blocks).to(self.t.device)
        elif hermitian:
            self.enqueue(ao, nroots, energy_only=True)
            coeffs = self.coeffs
        else:
            e, c, coeffs = self._host_coeffs(ao, nroots)
            if coeffs.shape[-2] != T:                       # (one geometry: (nroots, T) rows)
                blocks = torch.zeros((T, T), dtype=F64, device=self.t.device)
                blocks[:nroots] = coeffs
                coeffs = blocks
        unknown = set(observables) - {"dipole", "mulliken", "loewdin"}
        if unknown:
            raise ValueError(f"unknown observables {sorted(unknown)} (known: 'dipole', 'mulliken', 'loewdin')")
        want = tuple(observables) + (("d_ao",) if return_dm_ao else ())
        res = self._properties_device(ao, coeffs, nroots, P, dip, charges, coords, origin, want)
        self.synchronize()
        if hermitian and not return_forces:
            e = self.energy[..., :nroots].cpu().numpy().copy()
            self._raise_if_nan(e[..., 0])
            c = self.coeffs[..., :nroots, :].cpu().numpy().copy()
        res.pop("_keep")
        return e, c, P, {k: v.cpu().numpy() for k, v in res.items()}, grads

    @staticmethod
    def _property_dict(host: dict, P: np.ndarray, charges, move) -> dict:
        """Populations -> charges (``Z - pop`` on diagonal slots, ``-pop`` on transition slots); ``move``: puts the
        geometry axis in front of the pair axis."""
        from .properties import charges_from_populations
        Z = np.asarray(charges.cpu().numpy() if torch.is_tensor(charges) else charges, dtype=np.float64).reshape(-1)
        out = {}
        if "dipole" in host:
            out["dipole"] = move(host["dipole"])
        for k in ("mulliken", "loewdin"):
            if k in host:
                out[k + "_charges"] = charges_from_populations(move(host[k]), Z, P)
        if "d_ao" in host:
            out["dm_ao"] = move(host["d_ao"])
        return out


class BatchedEvaluator(_EvaluatorBase):
    """``count`` independent geometries per call (``evc_energy_with_grad_batch``): every launch covers
    the whole batch and the t-RDM is streamed once per up to 32 geometries.  Results stay on the device in
    ``energy (G,T)``, ``coeffs (G,T,T)``, ``grad (G,A,3)``."""

    def __init__(self, trdms: DeviceTRDMs, natm: int, count: int, stream: Optional["torch.cuda.Stream"] = None,
                 keep_density_matrices: bool = False, keep_hmat: bool = False, warm_start: bool = False,
                 keep_one_rdm: bool = False, energy_grad: Optional[torch.Tensor] = None):
        """``warm_start``: consecutive calls hold, slot by slot, nearby geometries (steps of ``count`` trajectories):
        from the second call on the eigensolvers start from the previous call's eigenvectors (EVC_FLAG_WARM_START).
        ``energy_grad``: caller's buffer of ``count * T + count * max(natm, 1) * 3`` doubles for the energies and the
        gradients -- e.g. PINNED HOST memory, which the device writes directly (no download copy, hosted.py)."""
        self.count = int(count)
        self._init_state(trdms, natm, stream, warm_start)
        d, n, T = trdms.device, trdms.n, trdms.T
        G = self.count
        # energies and gradients share one buffer: a caller that wants both on the host fetches them with ONE copy
        na = max(self.natm, 1)
        if energy_grad is None:
            energy_grad = torch.zeros(G * T + G * na * 3, dtype=F64, device=d)
        assert energy_grad.dtype == F64 and energy_grad.numel() == G * T + G * na * 3 and energy_grad.is_contiguous()
        self.energy_grad = energy_grad
        self.energy = self.energy_grad[: G * T].view(G, T)
        self.coeffs = torch.zeros((G, T, T), dtype=F64, device=d)
        self.grad = self.energy_grad[G * T:].view(G, na, 3)
        self.d_pred = torch.zeros((G, n, n), dtype=F64, device=d) if (keep_density_matrices or keep_one_rdm) else None
        self.g_pred = torch.zeros((G, n, n, n, n), dtype=F64, device=d) if keep_density_matrices else None
        # the subspace Hamiltonians H(R) (lower triangles as handed to the eigensolver), for subset re-solves
        self.hmat = torch.zeros((G, T, T), dtype=F64, device=d) if keep_hmat else None
        p = lambda t: (t.data_ptr() if t is not None else None)
        self.out = _lib.OutputsBatch(energy=p(self.energy), coeffs=p(self.coeffs), grad=p(self.grad),
                                     d_pred=p(self.d_pred), g_pred=p(self.g_pred), hmat=p(self.hmat))

    _suffix = "_batch"
    _nan_message = "generalised eigenproblem failed for at least one geometry of the batch"

    @property
    def _lead(self) -> tuple:
        return (self.count,)

    def _check_ao(self, aob: DeviceAOBatch) -> None:
        assert aob.count == self.count, "batch size is fixed at construction"

    def _rows_args(self, rows: torch.Tensor, need: int) -> tuple:
        """(pointer, row stride) of a (G, >= need) matrix of subspace-matrix rows."""
        assert rows.dtype == F64 and rows.dim() == 2 and rows.shape[0] == self.count
        assert rows.stride(1) == 1 and rows.shape[1] >= need
        return rows.data_ptr(), int(rows.stride(0))

    def phase_loewdin(self, aob: DeviceAOBatch, stream: Optional["torch.cuda.Stream"] = None) -> None:
        """Loewdin orthogonalisation of the batch alone (reads S and hcore only): the next ``enqueue`` of the SAME
        geometries skips it (``EVC_FLAG_LOEWDIN_DONE``).  ``stream``: enqueue it there instead of on this
        evaluator's stream (the caller orders the streams)."""
        self._check_ao(aob)
        g = aob.cstruct()
        self._call("evc_phase_loewdin", C.byref(g), self._flags(), sp=stream.cuda_stream if stream is not None else None)
        self._loewdin_done = True

    def energies_with_grads(self, aob: DeviceAOBatch):
        """(E[G], grad[G,A,3]) as numpy arrays."""
        self.enqueue(aob)
        self.synchronize()
        e = self.energy[:, 0].cpu().numpy().copy()
        self._raise_if_nan(e)
        return e, self.grad[:, : self.natm].cpu().numpy().copy()

    def phase_hamiltonian(self, aob: DeviceAOBatch, rows_out: torch.Tensor) -> None:
        """Scaled two-body rows of this rank's pairs -> ``rows_out[g, :rows_local]`` (row stride = rows_out.stride(0))."""
        rows = self._rows_args(rows_out, self.t.rows_local)
        _check_sym_first_call(self, aob)
        g = aob.cstruct()
        self._call("evc_phase_hamiltonian", C.byref(g),
                   self._flags(_ip1_flag(self.t, aob) & _lib.FLAG_ERI_S4, loewdin=True), *rows)

    # -- several roots of every geometry (evc_phase_gradient_roots_batch) -----------------------------------------
    def _host_coeffs(self, aob: DeviceAOBatch, nroots: int):
        """hermitian=False: the T x T pencil of every geometry solved on the host as
        ``ContinuationEvaluator._host_coeffs`` does; returns host E (G, nroots), C (G, nroots, T) and the device
        (G, T, T) coefficient blocks the gradient call reads."""
        _check_nonhermitian(self.t)
        G, T, d = self.count, self.t.T, self.t.device
        if self.hmat is None:
            self.hmat = torch.zeros((G, T, T), dtype=F64, device=d)
            self.out.hmat = self.hmat.data_ptr()
        rows = torch.zeros((G, max(self.t.rows_total, 1)), dtype=F64, device=d)
        self.phase_hamiltonian(aob, rows)
        enuc = aob.enuc.cpu().numpy()
        E = np.zeros((G, nroots))
        Cs = np.zeros((G, nroots, T))
        for g, eig in enumerate(self._host_eigs(aob, rows)):
            e, c = _select(*eig, nroots, False)
            E[g], Cs[g] = np.asarray(e, dtype=np.float64) + enuc[g], c
        blocks = np.zeros((G, T, T))
        blocks[:, :nroots] = Cs
        return E, Cs, torch.from_numpy(blocks).to(d)

    def multistate_energies_with_grads(self, aob: DeviceAOBatch, nroots: int, pairs=None,
                                       return_density_matrices: bool = False, hermitian: bool = True):
        """``ContinuationEvaluator.energies_with_grads`` for every geometry of the batch in one pass of the gradient
        chain (``evc_energy_with_grad_batch`` energy-only + ``evc_phase_gradient_roots_batch``): ``E (G,nroots)``,
        ``C (G,nroots,T)`` and ``grads (G,P,A,3)`` -- slot (k,k) the total gradient of root k, slot (k,l) the electronic
        coupling vector c_k^T dH/dR c_l, ``pairs`` the same (P,2) list for every geometry (default: the diagonal) --,
        with ``return_density_matrices`` also ``D (G,P,N,N)`` and ``Gamma (G,P,N^4)``.  ``hermitian=False``: the host
        eig selection per geometry (not on sym8).  G * P <= 4096."""
        assert aob.count == self.count, "batch size is fixed at construction"
        want = bool(return_density_matrices)
        # (the energy-only call checks the integrals' symmetry on the first call)
        E, Cs, grads, D, Gm = self._gradient_roots(aob, nroots, pairs, want, want, hermitian)
        res = (E, Cs, grads[:, :, : self.natm].transpose(0, 1).cpu().numpy().copy())
        if want:
            res += (D.transpose(0, 1).cpu().numpy().copy(),
                    Gm.transpose(0, 1).cpu().numpy().copy().reshape(self.count, Gm.shape[0], -1))
        return res


    def multistate_properties(self, aob: DeviceAOBatch, nroots: int, pairs=None, dip=None, charges=None, coords=None,
                              origin=(0.0, 0.0, 0.0), hermitian: bool = True, return_dm_ao: bool = False,
                              return_forces: bool = False, observables=("dipole", "mulliken", "loewdin")):
        """Dipole moments, transition dipole moments and atomic charges of the lowest ``nroots`` roots of every geometry
        of the batch, on the device from what the energy call left there (``evc_energy_with_grad_batch`` energy-only +
        ``evc_properties_roots_batch``; numpy statement: ``evcont_amd.properties``).  ``pairs``: the same (P,2) list
        k <= l < nroots for every geometry (default: the diagonal); slot (k,k) is state k, slot (k,l) the transition
        with the weighting (c_k c_l^T + c_l c_k^T) / 2.  ``dip`` (G,3,N,N) = <mu| r - origin |nu>, ``charges`` (A,),
        ``coords`` (G,A,3) Bohr: numpy or device tensors.  Returns ``E (G,nroots)``, ``C (G,nroots,T)`` and a dict of
        ``dipole (G,P,3)`` (atomic units; diagonal slots: total, nuclei included; transition slots: -tr(P r)),
        ``mulliken_charges`` and ``loewdin_charges (G,P,A)`` (``Z - pop`` on diagonal slots, ``-pop`` on transition
        slots; plain Mulliken, not the reference script's meta-Loewdin ``mulliken_meta``) and, with ``return_dm_ao``,
        ``dm_ao (G,P,N,N)``.  ``return_forces``: also ``grads (G,P,A,3)`` of the same slots as
        ``multistate_energies_with_grads`` returns them, from the same energy phase (one solve per step).
        ``observables``: which of "dipole", "mulliken", "loewdin" to compute and download.
        ``hermitian=False``: the host eig selection (not on sym8).  G * P <= 4096."""
        assert aob.count == self.count, "batch size is fixed at construction"
        e, c, P, host, grads = self._multistate_properties(aob, nroots, pairs, dip, charges, coords, origin, hermitian,
                                                           return_dm_ao, return_forces, observables)
        props = self._property_dict(host, P, charges, lambda x: np.ascontiguousarray(np.swapaxes(x, 0, 1)))
        if return_forces:
            return e, c, props, grads[:, :, : self.natm].transpose(0, 1).cpu().numpy().copy()
        return e, c, props


class PipelinedBatchedEvaluator:
    """Batches submitted one after another by a caller that uses ONE stream, kept ``depth`` deep in flight inside the
    library: every batch runs on one of ``depth`` internal streams (each with its own workspace and result buffers),
    forked from the caller's stream at submission and joined to it only when its results are asked for.  The
    latency-bound single-workgroup kernels of one batch (Loewdin orthogonalisation, subspace solve, gradient tail:
    a quarter of a batch's time on 32 of 256 CUs) then run beside the chip-filling kernels of its neighbours -- what a
    caller would otherwise have to arrange with several streams of its own.

        pe = PipelinedBatchedEvaluator(trdms, natm, G)            # depth 3
        tickets = [pe.enqueue(aob) for aob in batches[:3]]
        for k, aob in enumerate(batches[3:]):
            r = pe.results(tickets[k])        # caller's stream now waits for THAT batch (no host synchronisation)
            ... consume r.energy / r.grad on the caller's stream ...
            tickets.append(pe.enqueue(aob))   # reuses the slot just consumed

    Ordering guarantees: a batch starts after everything the caller's stream held at ``enqueue`` (inputs uploaded
    asynchronously on that stream are complete), and after the previous batch of ITS slot has finished; a slot's
    buffers are overwritten ``depth`` submissions later, so results must be consumed (or ``results`` called) before
    then.  ``next_aob`` is accepted for compatibility with the round-2 interface and ignored."""

    def __init__(self, trdms: DeviceTRDMs, natm: int, count: int, stream: Optional["torch.cuda.Stream"] = None,
                 depth: int = 3, **kw):
        d = trdms.device
        self.device = d
        self._caller = stream          # None: torch's current stream at call time
        self.depth = max(1, int(depth))
        self.streams = [torch.cuda.Stream(d) for _ in range(self.depth)]
        self.evs = [BatchedEvaluator(trdms, natm, count, stream=self.streams[k], **kw) for k in range(self.depth)]
        self._submitted = [torch.cuda.Event() for _ in range(self.depth)]   # caller's stream at submission
        self._done = [torch.cuda.Event() for _ in range(self.depth)]        # internal stream: the slot's batch finished
        self._busy = [False] * self.depth
        self._k = 0

    def _cs(self) -> "torch.cuda.Stream":
        return self._caller if self._caller is not None else torch.cuda.current_stream(self.device)

    def enqueue(self, aob: DeviceAOBatch, next_aob: Optional[DeviceAOBatch] = None, nroots: int = 1,
                energy_only: bool = False) -> int:
        """Enqueue one batch; returns its slot (the ticket for ``results``)."""
        slot = self._k % self.depth
        self._k += 1
        st = self.streams[slot]
        self._submitted[slot].record(self._cs())
        st.wait_event(self._submitted[slot])                   # fork (the slot's previous batch precedes on `st` itself)
        self.evs[slot].enqueue(aob, nroots, energy_only)
        self._done[slot].record(st)
        self._busy[slot] = True
        return slot

    def results(self, slot: int) -> "BatchedEvaluator":
        """The evaluator holding the results of the batch submitted under this ticket; the caller's stream is made to
        wait for it (join)."""
        if self._busy[slot]:
            self._cs().wait_event(self._done[slot])
            self._busy[slot] = False
        return self.evs[slot]

    def synchronize(self) -> None:
        for st in self.streams:
            st.synchronize()
        self._cs().synchronize()


class ContinuationEvaluator(_EvaluatorBase):
    """Energy / energy+force of the continuation at one geometry per call
    (``get_energy_with_grad``, ``ab_initio_gradients_loewdin.py:308-379``)."""

    def __init__(self, trdms: DeviceTRDMs, natm: int, stream: Optional["torch.cuda.Stream"] = None,
                 warm_start: bool = False, want_two_rdm: bool = True):
        """``stream``: HIP stream every call of this evaluator is enqueued on (default: torch's current
        stream at call time).  Several evaluators on different streams may share one ``DeviceTRDMs``:
        each owns its workspace and outputs, so independent geometries overlap on the device.

        ``warm_start``: consecutive calls are steps of one trajectory (``EVC_FLAG_WARM_START``): from the
        second call on, the two Jacobi eigensolvers start from the eigenvectors the previous call left in the
        workspace.  Same results to solver tolerance (~1e-14), not bit for bit."""
        self._init_state(trdms, natm, stream, warm_start)
        d, n, T = trdms.device, trdms.n, trdms.T
        self.energy = torch.zeros(T, dtype=F64, device=d)
        self.coeffs = torch.zeros((T, T), dtype=F64, device=d)
        self.grad = torch.zeros((max(self.natm, 1), 3), dtype=F64, device=d)
        self.d_pred = torch.zeros((n, n), dtype=F64, device=d)
        self.g_pred = torch.zeros((n, n, n, n), dtype=F64, device=d) if want_two_rdm else None
        self.hmat = torch.zeros((T, T), dtype=F64, device=d)
        self.out = Outputs(energy=self.energy.data_ptr(), coeffs=self.coeffs.data_ptr(), grad=self.grad.data_ptr(),
                           d_pred=self.d_pred.data_ptr(),
                           g_pred=(self.g_pred.data_ptr() if want_two_rdm else None), hmat=self.hmat.data_ptr())

    # scipy.linalg.eigh raises LinAlgError when S is not positive definite (evcont.py:75)
    _nan_message = "generalised eigenproblem failed: overlap matrix not positive definite or non-finite input"

    def _rows_args(self, rows: torch.Tensor, need: int) -> tuple:
        assert rows.dtype == F64 and rows.numel() == need and rows.is_contiguous()
        return (rows.data_ptr(),)

    # -- single-device fused path -------------------------------------------------------------
    def energy_with_grad(self, ao: DeviceAO, return_density_matrices: bool = False):
        self.enqueue(ao, 1, False)
        self.synchronize()
        e = float(self.energy[0].item())
        self._raise_if_nan(e)
        g = self.grad[: self.natm].cpu().numpy().copy()
        if return_density_matrices:
            if self.g_pred is None:
                raise _lib.EvcontHipError("this evaluator was built with want_two_rdm=False")
            return e, g, self.d_pred.cpu().numpy().copy(), self.g_pred.cpu().numpy().copy()
        return e, g

    def energies(self, ao: DeviceAO, nroots: int = 1):
        """Lowest ``nroots`` total energies and their coefficient vectors (rows)."""
        self.enqueue(ao, nroots, True)
        self.synchronize()
        e = self.energy[:nroots].cpu().numpy().copy()
        self._raise_if_nan(e[0])
        return e, self.coeffs.reshape(-1)[: nroots * self.t.T].reshape(nroots, self.t.T).cpu().numpy().copy()

    # -- phase API for the pair-sharded multi-GPU host (evcont_amd/distributed.py) -----------------
    def phase_hamiltonian(self, ao: DeviceAO) -> torch.Tensor:
        """Returns a view of this rank's scaled two-body rows (length rows_local) in the workspace."""
        _check_sym_first_call(self, ao)
        g = ao.cstruct()
        p_rows, p_h1 = C.c_void_p(), C.c_void_p()
        flags = self._flags(_ip1_flag(self.t, ao) & _lib.FLAG_ERI_S4, loewdin=True)
        rc = self.lib.evc_phase_hamiltonian(C.byref(self.t.cstruct), C.byref(g), flags, self.ws.data_ptr(),
                                            self.ws_bytes, C.byref(p_rows), C.byref(p_h1), self._sp())
        check(rc, "evc_phase_hamiltonian")
        off = p_rows.value - self.ws.data_ptr()
        return self.ws[off: off + 8 * self.t.rows_local].view(F64)

    def phase_set_coeffs(self, coeffs: torch.Tensor) -> None:
        """Row weights of the predicted RDMs from a caller-supplied coefficient vector (``evc_phase_set_coeffs``)."""
        assert coeffs.dtype == F64 and coeffs.numel() == self.t.T and coeffs.is_contiguous()
        self._call("evc_phase_set_coeffs", coeffs.data_ptr(), self.natm)

    def energy_with_grad_nonhermitian(self, ao: DeviceAO, return_density_matrices: bool = False):
        """``get_energy_with_grad(..., hermitian=False)`` (``ab_initio_gradients_loewdin.py:341-379`` with the ``eig``
        branch of ``ab_initio_eigenvector_continuation.py:76-88``): the device assembles H(R) as for the Hermitian
        branch; the T x T non-symmetric pencil goes to ``scipy.linalg.eig`` on the host, as in the reference (pair
        layouts: upper triangle filled from the lower one, ``|Im| < 1e-5`` filter, ``argmin``), and ITS 2-norm
        eigenvector -- real part, as the reference takes it -- defines the predicted RDMs and the gradient."""
        e, vec = _select(*self._host_eig(ao), 1, True)
        self.phase_set_coeffs(torch.from_numpy(vec).to(self.t.device))
        self.phase_gradient(ao, False)
        self.synchronize()
        g = self.grad[: self.natm].cpu().numpy().copy()
        if return_density_matrices:
            if self.g_pred is None:
                raise _lib.EvcontHipError("this evaluator was built with want_two_rdm=False")
            return e + ao.enuc, g, self.d_pred.cpu().numpy().copy(), self.g_pred.cpu().numpy().copy()
        return e + ao.enuc, g

    def _host_eig(self, ao: DeviceAO):
        """hermitian=False: H(R) assembled on the device as for the Hermitian branch, then the reference's ``eig``
        branch on the host (``_eig_nonhermitian``)."""
        _check_nonhermitian(self.t)
        return self._host_eigs(ao, self.phase_hamiltonian(ao))[0]

    # -- several roots of one geometry (evc_phase_gradient_roots) ------------------------------------------
    def _host_coeffs(self, ao: DeviceAO, nroots: int):
        """hermitian=False: the reference's eig branch for every root (2-norm eigenvectors, real part, |Im| < 1e-5,
        ascending); returns host E (nroots,), C (nroots, T) and the device copy of C the gradient call reads."""
        e, c = _select(*self._host_eig(ao), nroots, False)
        c = np.ascontiguousarray(c, dtype=np.float64)
        return np.asarray(e, dtype=np.float64) + ao.enuc, c, torch.from_numpy(c).to(self.t.device)

    def _roots(self, ao: DeviceAO, nroots: int, pairs, want_d: bool, want_g: bool, hermitian: bool):
        """Enqueue energies + the gradient slots of ``pairs``; returns host E, C and the device output tensors."""
        if hermitian:
            _check_sym_first_call(self, ao)           # (with eri_ip1: the energy-only call checks eri alone)
        return self._gradient_roots(ao, nroots, pairs, want_d, want_g, hermitian)

    def energies_with_grads(self, ao: DeviceAO, nroots: int, pairs=None, return_density_matrices: bool = False,
                            hermitian: bool = True):
        """Lowest ``nroots`` total energies ``E (nroots,)``, their coefficient rows ``C (nroots,T)`` and one gradient
        per slot ``grads (P,A,3)`` in ONE pass of the gradient chain (``evc_phase_gradient_roots``).  ``pairs``: (P,2)
        root pairs k <= l < nroots, default ``[(k, k) for k < nroots]``; slot (k,k) is the total gradient of root k,
        slot (k,l) the electronic coupling vector c_k^T dH/dR c_l.  ``return_density_matrices``: also ``D (P,N,N)``
        and ``Gamma (P,N,N,N,N)``, the predicted (transition) RDMs of each slot.  ``hermitian=False``: the roots of
        the reference's ``eig`` branch (host solve of the T x T pencil), every root as ``get_energy_with_grad``
        takes root 0.  At (near-)degenerate roots the forces follow whichever eigenvectors the solver returned."""
        if return_density_matrices and self.g_pred is None:
            raise _lib.EvcontHipError("this evaluator was built with want_two_rdm=False")
        e, c, grads, D, G = self._roots(ao, nroots, pairs, return_density_matrices, return_density_matrices,
                                        hermitian)
        gr = grads[:, : self.natm].cpu().numpy().copy()
        if return_density_matrices:
            return e, c, gr, D.cpu().numpy(), G.cpu().numpy()
        return e, c, gr


    def multistate_properties(self, ao: DeviceAO, nroots: int, pairs=None, dip=None, charges=None, coords=None,
                              origin=(0.0, 0.0, 0.0), hermitian: bool = True, return_dm_ao: bool = False,
                              return_forces: bool = False, observables=("dipole", "mulliken", "loewdin")):
        """``BatchedEvaluator.multistate_properties`` for one geometry (``evc_properties_roots_batch`` with count = 1 on
        this evaluator's workspace): ``E (nroots,)``, ``C (nroots,T)`` and the dict of ``dipole (P,3)``,
        ``mulliken_charges`` / ``loewdin_charges (P,A)`` and, on request, ``dm_ao (P,N,N)``; ``return_forces``: also
        ``grads (P,A,3)``.  ``dip`` (3,N,N), ``charges`` (A,), ``coords`` (A,3)."""
        e, c, P, host, grads = self._multistate_properties(ao, nroots, pairs, dip, charges, coords, origin, hermitian,
                                                           return_dm_ao, return_forces, observables)
        props = self._property_dict(host, P, charges, lambda x: x)
        if return_forces:
            return e, c, props, grads[:, : self.natm].cpu().numpy().copy()
        return e, c, props
