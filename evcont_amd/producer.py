"""The base of the three device integral producers (``hchain_device.DeviceSGaussians``, ``gto_device.DeviceGaussians``,
``gto_spd_device.DeviceSpdGaussians``): everything about a call that does not depend on the kind of shells.  It owns the
staging of host coordinates, the output buffers kept per ``(G, need_grad, packed)``, the workspace, the dipole tensors
kept per G and, for a uniform electric field (``csrc/field.hip``; host statement: ``evcont_amd.field``), the fold of one
field per geometry into the arrays an ``integrals`` call has just written.

Every C call of a route has the form ``f(A, nsets, G, coords, [charges,] *basis, ...)``; a subclass names its four calls,
``_nsets``, ``_basis_args()`` and ``_workspace_args(G)``, and says what ``nao`` is.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from .evaluator import DeviceAOBatch, F64, _dev

_FIELDS = ("enuc", "S", "hcore", "eri", "ipovlp", "dhcore", "eri_ip1", "gnuc")


class DeviceProducer:
    """AO integrals of one molecule on the device from its coordinates.  A subclass sets ``_charges`` (device (A,)),
    ``_charges_host`` and ``_aoslices`` (device (A,2) int64), at the latest in ``_setup``."""

    # the C calls of the route (names in ``include/evcont_hip.h``)
    _WORKSPACE = _INTEGRALS = _DIPOLE = _DIPOLE_GRAD = None

    def __init__(self, device=None):
        self.lib = _lib.load()
        self.device = _dev(device)
        self._charges = self._charges_host = self._aoslices = None
        self._buffers = {}         # (G, need_grad, packed) -> dict of output tensors
        self._coords = {}          # G -> device (G,A,3) staging of host coordinates
        self._dip = {}             # G -> device (G,3,N,N) dipole integrals
        self._ipdip = {}           # G -> device (G,3,3,N,N) their gradient
        self._field = {}           # G -> device (G,3) staging of host fields
        self._ws = None

    @property
    def natm(self) -> Optional[int]:
        return None if self._charges is None else int(self._charges.shape[0])

    @property
    def charges(self) -> torch.Tensor:
        """Nuclear charges, device (A,)."""
        return self._charges

    def _setup(self, A: int) -> None:
        """Called with the centre count of every coordinate array before it is used."""
        if A != self.natm:
            raise ValueError(f"coordinates of {A} centres for a molecule of {self.natm}")

    def allocate(self, G: int, need_grad: bool = True, packed: bool = False) -> dict:
        """Output tensors of a call of ``G`` geometries (what ``integrals(..., out=...)`` accepts)."""
        A, n = self.natm, self.nao
        ms = n * (n + 1) // 2
        z = lambda *shape: torch.zeros(shape, dtype=F64, device=self.device)
        out = {"enuc": z(G), "S": z(G, n, n), "hcore": z(G, n, n), "eri": z(G, ms, ms) if packed else z(G, n, n, n, n)}
        if need_grad:
            out.update(ipovlp=z(G, 3, n, n), dhcore=z(G, A, 3, n, n), gnuc=z(G, A, 3),
                       eri_ip1=z(G, 3, n, n, ms) if packed else z(G, 3, n, n, n, n))
        return out

    def _device_coords(self, coords) -> torch.Tensor:
        """``coords`` ((G,A,3) or (A,3); numpy or a device tensor) as a contiguous device (G,A,3) tensor; host
        coordinates go through the staging tensor kept per G."""
        if not torch.is_tensor(coords):
            coords = np.ascontiguousarray(coords, dtype=np.float64)
        shape = tuple(coords.shape)
        if len(shape) < 2 or shape[-1] != 3:
            raise ValueError("coords must be (G,A,3) or (A,3)")
        A = int(shape[-2])
        self._setup(A)
        if torch.is_tensor(coords):
            return coords.to(device=self.device, dtype=F64).reshape(-1, A, 3).contiguous()
        host = coords.reshape(-1, A, 3)
        G = host.shape[0]
        R = self._coords.get(G)
        if R is None:
            R = self._coords[G] = torch.empty((G, A, 3), dtype=F64, device=self.device)
        R.copy_(torch.from_numpy(host))
        return R

    def staged_coords(self, G: int) -> torch.Tensor:
        """The device (G,A,3) copy of the HOST coordinates the last ``integrals`` / ``dipole_integrals`` call of ``G``
        geometries uploaded: what a following device call on the same geometries reads without a second upload."""
        return self._coords[int(G)]

    def _call(self, name: str, R: torch.Tensor, *args) -> None:
        """One C call of the route on the geometries ``R`` (device (G,A,3)), enqueued on the current stream."""
        _lib.check(getattr(self.lib, name)(int(R.shape[1]), self._nsets, int(R.shape[0]), R.data_ptr(), *args,
                                           torch.cuda.current_stream(self.device).cuda_stream), name)

    def _kept(self, cache: dict, G: int, *shape) -> torch.Tensor:
        t = cache.get(G)
        if t is None:
            t = cache[G] = torch.zeros((G,) + shape, dtype=F64, device=self.device)
        return t

    def integrals(self, coords, need_grad: bool = True, packed: bool = False, out: Optional[dict] = None, field=None,
                  origin=(0.0, 0.0, 0.0)) -> DeviceAOBatch:
        """The integrals at ``coords`` ((G,A,3) or (A,3), Bohr; numpy or a device tensor), enqueued on the current
        stream of the device.  ``packed``: ``eri`` as the dense (Ms,Ms) s4 matrix and ``eri_ip1`` packed in its last two
        indices (s2kl), what evaluators on the compressed layout read (at most 64 functions).  ``out``: a dict of tensors
        as ``allocate`` returns to write into, instead of the buffers this object keeps for the shape.
        ``field``: None, or a uniform electric field ((3,) or one per geometry (G,3), atomic units; numpy or a device
        tensor) with the dipole operator's ``origin``: behind the integrals the call then enqueues the dipole integrals,
        their gradient (with ``need_grad``) and the fold of the field into ``hcore``, ``dhcore``, ``enuc`` and ``gnuc``
        (``evc_field_fold_batch``).  Without a field nothing more than the integrals is enqueued."""
        R = self._device_coords(coords)
        G = int(R.shape[0])
        need_grad, packed = bool(need_grad), bool(packed)
        if out is None:
            key = (G, need_grad, packed)
            out = self._buffers.get(key)
            if out is None:
                out = self._buffers[key] = self.allocate(G, need_grad, packed)
        nbytes = getattr(self.lib, self._WORKSPACE)(*self._workspace_args(G))
        if nbytes == 0:
            raise _lib.EvcontHipError(self._WORKSPACE + ": " + self.lib.evc_last_error().decode())
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        flags = (0 if need_grad else _lib.FLAG_ENERGY_ONLY) | \
                ((_lib.FLAG_ERI_S4 | _lib.FLAG_IP1_S2KL) if packed else 0)
        cs = _lib.SgtoOutputs(**{k: (out[k].data_ptr() if out.get(k) is not None else None) for k in _FIELDS})
        self._call(self._INTEGRALS, R, self._charges.data_ptr(), *self._basis_args(), C.byref(cs), flags,
                   self._ws.data_ptr(), int(self._ws.numel()))
        if field is not None:
            self._fold_field(R, out, need_grad, field, origin)
        return DeviceAOBatch(S=out["S"], hcore=out["hcore"], eri=out["eri"], enuc=out["enuc"], natm=self.natm,
                             ipovlp=out.get("ipovlp"), dhcore=out.get("dhcore"), eri_ip1=out.get("eri_ip1"),
                             gnuc=out.get("gnuc"), aoslices=self._aoslices, ip1_s2kl=packed and need_grad,
                             eri_s4=packed)

    def dipole_integrals(self, coords, origin=(0.0, 0.0, 0.0)) -> torch.Tensor:
        """AO dipole integrals ``<mu| r - origin |nu>`` at ``coords`` as a device (G,3,N,N) tensor (host statement:
        ``dipole_integrals`` of the molecule classes), enqueued on the current stream.  The tensor is kept per G: a
        later call of the same G overwrites it."""
        R = self._device_coords(coords)
        dip = self._kept(self._dip, int(R.shape[0]), 3, self.nao, self.nao)
        o = (C.c_double * 3)(*[float(x) for x in origin])
        self._call(self._DIPOLE, R, *self._basis_args(), C.cast(o, C.c_void_p), dip.data_ptr())
        return dip

    def dipole_grad_integrals(self, coords, origin=(0.0, 0.0, 0.0)) -> torch.Tensor:
        """``ipdip[g,x,c,mu,nu] = <d_x mu| r_c - origin_c |nu>`` at ``coords`` as a device (G,3,3,N,N) tensor (host
        statement: ``dipole_grad_integrals`` of the molecule classes), enqueued on the current stream.  The tensor is kept
        per G: a later call of the same G overwrites it."""
        R = self._device_coords(coords)
        ipdip = self._kept(self._ipdip, int(R.shape[0]), 3, 3, self.nao, self.nao)
        o = (C.c_double * 3)(*[float(x) for x in origin])
        self._call(self._DIPOLE_GRAD, R, *self._basis_args(), C.cast(o, C.c_void_p), ipdip.data_ptr())
        return ipdip

    def _device_field(self, field, G: int) -> torch.Tensor:
        """``field`` ((3,) or (G,3); numpy or a device tensor) as a contiguous device (G,3) tensor; a host field goes
        through a staging tensor kept per G."""
        if torch.is_tensor(field):
            F = field.to(device=self.device, dtype=F64)
            F = F.reshape(1, 3).expand(G, 3) if F.numel() == 3 else F.reshape(G, 3)
            return F.contiguous()
        host = np.asarray(field, dtype=np.float64)
        host = np.broadcast_to(host.reshape(1, 3), (G, 3)) if host.size == 3 else host.reshape(G, 3)
        F = self._field.get(G)
        if F is None:
            F = self._field[G] = torch.empty((G, 3), dtype=F64, device=self.device)
        F.copy_(torch.from_numpy(np.ascontiguousarray(host)))
        return F

    def _fold_field(self, R: torch.Tensor, out: dict, need_grad: bool, field, origin) -> None:
        """After the integrals of ``R`` (device (G,A,3)) were enqueued into ``out``: the dipole integrals, their gradient
        (with ``need_grad``) and ``evc_field_fold_batch``, on the same stream in this order."""
        G, A = int(R.shape[0]), int(R.shape[1])
        F = self._device_field(field, G)
        dip = self.dipole_integrals(R, origin)
        ipdip = self.dipole_grad_integrals(R, origin) if need_grad else None
        o = (C.c_double * 3)(*[float(x) for x in origin])
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(self.lib.evc_field_fold_batch(
            int(dip.shape[-1]), A, G, dip.data_ptr(), ptr(ipdip), self._aoslices.data_ptr(), self.charges.data_ptr(),
            R.data_ptr(), F.data_ptr(), C.cast(o, C.c_void_p), 0 if need_grad else _lib.FLAG_ENERGY_ONLY,
            out["hcore"].data_ptr(), ptr(out.get("dhcore")) if need_grad else None, out["enuc"].data_ptr(),
            ptr(out.get("gnuc")) if need_grad else None, torch.cuda.current_stream(self.device).cuda_stream),
            "evc_field_fold_batch")
