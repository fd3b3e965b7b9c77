"""Device route of ``evcont_amd.hchain.s_gaussian_mol``: the AO integrals (and their first nuclear derivatives) of a
molecule built from one contracted s Gaussian per centre, computed on the GPU from the coordinates
(``evc_sgto_integrals_batch``, ``csrc/sgto.hip``) and written straight into the arrays the evaluators read.

    sg = DeviceSGaussians.from_mol(hydrogen_chain(10, 1.8))
    aob = sg.integrals(R)                      # R (G,A,3) Bohr, numpy or a device tensor -> DeviceAOBatch
    E, C, grads = batched_evaluator.multistate_energies_with_grads(aob, nroots)

The outputs live in buffers the object keeps per ``(G, need_grad, packed)``, so a steady MD loop allocates nothing per
step; a later call of the same shape overwrites what the previous one returned.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .evaluator import DeviceAOBatch, F64, _dev
from .field_device import FieldProducer
from .hchain import STO3G_H_COEFFICIENTS, STO3G_H_EXPONENTS

_FIELDS = ("enuc", "S", "hcore", "eri", "ipovlp", "dhcore", "eri_ip1", "gnuc")


class DeviceSGaussians(FieldProducer):
    """One contracted s function (``exponents``, ``coefficients`` of normalised primitives) on every centre of a molecule
    with nuclear ``charges`` (default: 1 on each of the centres of the first ``integrals`` call)."""

    def __init__(self, charges: Optional[Sequence[float]] = None, exponents: Sequence[float] = STO3G_H_EXPONENTS,
                 coefficients: Sequence[float] = STO3G_H_COEFFICIENTS, nelec: Optional[Tuple[int, int]] = None,
                 device=None):
        self.lib = _lib.load()
        self.device = _dev(device)
        self.exponents = np.ascontiguousarray(exponents, dtype=np.float64)
        self.coefficients = np.ascontiguousarray(coefficients, dtype=np.float64)
        if self.exponents.ndim != 1 or self.exponents.shape != self.coefficients.shape:
            raise ValueError("exponents and coefficients must be one-dimensional and of one length")
        self.nelec = None if nelec is None else tuple(nelec)
        self._charges_host = None if charges is None else np.ascontiguousarray(charges, dtype=np.float64).reshape(-1)
        self._charges = None       # device (A,)
        self._aoslices = None      # device (A,2) int64, built once
        self._buffers = {}         # (G, need_grad, packed) -> dict of output tensors
        self._coords = {}          # G -> device (G,A,3) staging of host coordinates
        self._dip = {}             # G -> device (G,3,N,N) dipole integrals
        self._ipdip = {}           # G -> device (G,3,3,N,N) their gradient (field_device.FieldProducer)
        self._field = {}           # G -> device (G,3) staging of host fields
        self._ws = None

    @classmethod
    def from_mol(cls, mol, device=None) -> "DeviceSGaussians":
        """For an ``HChainMol``: its charges, contraction and electron numbers."""
        return cls(charges=mol.charges, exponents=mol.exponents, coefficients=mol.coefficients, nelec=mol.nelec,
                   device=device)

    @property
    def natm(self) -> Optional[int]:
        return None if self._charges is None else int(self._charges.shape[0])

    def _setup(self, A: int) -> None:
        if self._charges is None:
            z = np.ones(A) if self._charges_host is None else self._charges_host
            self._charges = torch.from_numpy(z).to(self.device)
            self._aoslices = torch.from_numpy(
                np.stack([np.arange(len(z)), np.arange(len(z)) + 1], axis=1).astype(np.int64)).to(self.device)
        if A != self.natm:
            raise ValueError(f"coordinates of {A} centres for a molecule of {self.natm}")

    def allocate(self, G: int, need_grad: bool = True, packed: bool = False) -> dict:
        """Output tensors of a call of ``G`` geometries (what ``integrals(..., out=...)`` accepts)."""
        A = n = self.natm
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
        if torch.is_tensor(coords):
            R = coords.to(device=self.device, dtype=F64).reshape((-1,) + tuple(coords.shape[-2:])).contiguous()
            self._setup(int(R.shape[1]))
        else:
            host = np.ascontiguousarray(coords, dtype=np.float64)
            host = host.reshape((-1,) + host.shape[-2:])
            G, A = host.shape[0], host.shape[1]
            self._setup(A)
            R = self._coords.get(G)
            if R is None:
                R = self._coords[G] = torch.empty((G, A, 3), dtype=F64, device=self.device)
            R.copy_(torch.from_numpy(host))
        if R.shape[-1] != 3:
            raise ValueError("coords must be (G,A,3) or (A,3)")
        return R

    def staged_coords(self, G: int) -> torch.Tensor:
        """The device (G,A,3) copy of the HOST coordinates the last ``integrals`` / ``dipole_integrals`` call of ``G``
        geometries uploaded: what a following device call on the same geometries reads without a second upload."""
        return self._coords[int(G)]

    @property
    def charges(self) -> torch.Tensor:
        """Nuclear charges, device (A,)."""
        return self._charges

    def dipole_integrals(self, coords, origin=(0.0, 0.0, 0.0)) -> torch.Tensor:
        """AO dipole integrals ``<mu| r - origin |nu>`` at ``coords`` as a device (G,3,N,N) tensor
        (``evc_sgto_dipole_batch``; host statement: ``HChainMol.dipole_integrals``), enqueued on the current stream.  The
        tensor is kept per G: a later call of the same G overwrites it."""
        R = self._device_coords(coords)
        G, A = int(R.shape[0]), int(R.shape[1])
        dip = self._dip.get(G)
        if dip is None:
            dip = self._dip[G] = torch.zeros((G, 3, A, A), dtype=F64, device=self.device)
        o = (C.c_double * 3)(*[float(x) for x in origin])
        _lib.check(self.lib.evc_sgto_dipole_batch(
            A, int(self.exponents.shape[0]), G, R.data_ptr(), self.exponents.ctypes.data, self.coefficients.ctypes.data,
            C.cast(o, C.c_void_p), dip.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream),
            "evc_sgto_dipole_batch")
        return dip

    def _nao_now(self) -> int:
        return self.natm

    def _ipdip_call(self, R, G, origin, ipdip) -> None:
        _lib.check(self.lib.evc_sgto_dipole_grad_batch(
            int(R.shape[1]), int(self.exponents.shape[0]), G, R.data_ptr(), self.exponents.ctypes.data,
            self.coefficients.ctypes.data, origin, ipdip.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream),
            "evc_sgto_dipole_grad_batch")

    def integrals(self, coords, need_grad: bool = True, packed: bool = False, out: Optional[dict] = None, field=None,
                  origin=(0.0, 0.0, 0.0)) -> DeviceAOBatch:
        """The integrals at ``coords`` ((G,A,3) or (A,3), Bohr; numpy or a device tensor), enqueued on the current
        stream of the device.  ``packed``: ``eri`` as the dense (Ms,Ms) s4 matrix and ``eri_ip1`` packed in its last two
        indices (s2kl), what evaluators on the compressed layout read (at most 64 centres).  ``out``: a dict of tensors
        as ``allocate`` returns to write into, instead of the buffers this object keeps for the shape.
        ``field``: None, or a uniform electric field ((3,) or one per geometry (G,3), atomic units; numpy or a device
        tensor) with the dipole operator's ``origin``: behind the integrals the call then enqueues the dipole integrals,
        their gradient (with ``need_grad``) and the fold of the field into ``hcore``, ``dhcore``, ``enuc`` and ``gnuc``
        (``evc_field_fold_batch``).  Without a field nothing more than the integrals is enqueued."""
        if torch.is_tensor(coords):
            R = coords.to(device=self.device, dtype=F64).reshape((-1,) + tuple(coords.shape[-2:])).contiguous()
            G, A = int(R.shape[0]), int(R.shape[1])
            self._setup(A)
        else:
            host = np.ascontiguousarray(coords, dtype=np.float64)
            host = host.reshape((-1,) + host.shape[-2:])
            G, A = host.shape[0], host.shape[1]
            self._setup(A)
            R = self._coords.get(G)
            if R is None:
                R = self._coords[G] = torch.empty((G, A, 3), dtype=F64, device=self.device)
            R.copy_(torch.from_numpy(host))
        if R.shape[-1] != 3:
            raise ValueError("coords must be (G,A,3) or (A,3)")
        need_grad, packed = bool(need_grad), bool(packed)
        if out is None:
            key = (G, need_grad, packed)
            out = self._buffers.get(key)
            if out is None:
                out = self._buffers[key] = self.allocate(G, need_grad, packed)
        nprim = int(self.exponents.shape[0])
        nbytes = self.lib.evc_sgto_workspace_bytes(A, nprim, G)
        if nbytes == 0:
            raise _lib.EvcontHipError("evc_sgto_workspace_bytes: " + self.lib.evc_last_error().decode())
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        flags = (0 if need_grad else _lib.FLAG_ENERGY_ONLY) | \
                ((_lib.FLAG_ERI_S4 | _lib.FLAG_IP1_S2KL) if packed else 0)
        cs = _lib.SgtoOutputs(**{k: (out[k].data_ptr() if out.get(k) is not None else None) for k in _FIELDS})
        _lib.check(self.lib.evc_sgto_integrals_batch(
            A, nprim, G, R.data_ptr(), self._charges.data_ptr(), self.exponents.ctypes.data,
            self.coefficients.ctypes.data, C.byref(cs), flags, self._ws.data_ptr(), int(self._ws.numel()),
            torch.cuda.current_stream(self.device).cuda_stream), "evc_sgto_integrals_batch")
        if field is not None:
            self._fold_field(R, out, need_grad, field, origin)
        return DeviceAOBatch(S=out["S"], hcore=out["hcore"], eri=out["eri"], enuc=out["enuc"], natm=A,
                             ipovlp=out.get("ipovlp"), dhcore=out.get("dhcore"), eri_ip1=out.get("eri_ip1"),
                             gnuc=out.get("gnuc"), aoslices=self._aoslices, ip1_s2kl=packed and need_grad,
                             eri_s4=packed)
