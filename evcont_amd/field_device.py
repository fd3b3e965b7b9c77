"""What the three device integral producers (``hchain_device.DeviceSGaussians``, ``gto_device.DeviceGaussians``,
``gto_spd_device.DeviceSpdGaussians``) share for a uniform electric field (``csrc/field.hip``; host statement:
``evcont_amd.field``): the nuclear derivative of the dipole integrals as a device tensor kept per G, and the fold of one
field per geometry into the arrays an ``integrals`` call has just written.

A producer provides ``_ipdip_call(R, G, origin_ptr, ipdip)`` (its C call), ``_nao_now()``, the dicts ``_ipdip`` and
``_field`` (kept per G), ``dipole_integrals``, ``_device_coords``, ``charges``, ``_aoslices``, ``lib`` and ``device``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

F64 = torch.float64


class FieldProducer:
    """Mixin of the device integral producers."""

    def dipole_grad_integrals(self, coords, origin=(0.0, 0.0, 0.0)) -> torch.Tensor:
        """``ipdip[g,x,c,mu,nu] = <d_x mu| r_c - origin_c |nu>`` at ``coords`` as a device (G,3,3,N,N) tensor (host
        statement: ``dipole_grad_integrals`` of the molecule classes), enqueued on the current stream.  The tensor is kept
        per G: a later call of the same G overwrites it."""
        R = self._device_coords(coords)
        G = int(R.shape[0])
        ipdip = self._ipdip.get(G)
        if ipdip is None:
            n = self._nao_now()
            ipdip = self._ipdip[G] = torch.zeros((G, 3, 3, n, n), dtype=F64, device=self.device)
        o = (C.c_double * 3)(*[float(x) for x in origin])
        self._ipdip_call(R, G, C.cast(o, C.c_void_p), ipdip)
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
