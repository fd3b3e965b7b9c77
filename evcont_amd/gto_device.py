"""Device route of ``evcont_amd.gto_small.sp_gaussian_mol``: the AO integrals (and their first nuclear derivatives) of a
molecule of contracted Cartesian s and p Gaussian shells, computed on the GPU from the coordinates
(``evc_spgto_integrals_batch``, ``csrc/spgto.hip``) and written straight into the arrays the evaluators read.

    dg = DeviceGaussians.from_mol(gto_small.water("sto-3g"))
    aob = dg.integrals(R)                      # R (G,A,3) Bohr, numpy or a device tensor -> DeviceAOBatch
    E, C, grads = batched_evaluator.multistate_energies_with_grads(aob, nroots)

The interface is that of ``hchain_device.DeviceSGaussians`` (which stays the route for one s function per centre).  The
outputs live in buffers the object keeps per ``(G, need_grad, packed)``, so a steady MD loop allocates nothing per step;
a later call of the same shape overwrites what the previous one returned.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .evaluator import DeviceAOBatch, F64, _dev
from .field_device import FieldProducer
from .gto_small import contraction_coefficients, flatten_shells

_FIELDS = ("enuc", "S", "hcore", "eri", "ipovlp", "dhcore", "eri_ip1", "gnuc")


class DeviceGaussians(FieldProducer):
    """``shells``: per atom a list of ``gto_small.Shell``; ``charges``: the nuclear charges; ``renormalize``: scale every
    contracted function to unit self-overlap (on the host, once), as ``sp_gaussian_mol`` does."""

    # the C calls and the host normalisation of the route; ``gto_spd_device.DeviceSpdGaussians`` names its own
    _WORKSPACE, _INTEGRALS, _DIPOLE = "evc_spgto_workspace_bytes", "evc_spgto_integrals_batch", "evc_spgto_dipole_batch"
    _coefficients = staticmethod(contraction_coefficients)

    def __init__(self, charges: Sequence[float], shells, nelec: Optional[Tuple[int, int]] = None,
                 renormalize: bool = True, device=None):
        self.lib = _lib.load()
        self.device = _dev(device)
        self.shells = [list(atom) for atom in shells]
        self._charges_host = np.ascontiguousarray(charges, dtype=np.float64).reshape(-1)
        if len(self.shells) != self._charges_host.shape[0]:
            raise ValueError(f"{len(self.shells)} shell lists for {self._charges_host.shape[0]} charges")
        self.nelec = None if nelec is None else tuple(nelec)
        self.renormalize = bool(renormalize)
        # the HOST description of the basis every call passes
        (self.shell_atom, self.shell_l, self.shell_prim_offset, self.exponents, self.coefficients, slices,
         self.nao) = flatten_shells(self.shells, self._coefficients(self.shells, renormalize))
        self._charges = torch.from_numpy(self._charges_host).to(self.device)
        self._aoslices = torch.from_numpy(slices).to(self.device)
        self._buffers = {}         # (G, need_grad, packed) -> dict of output tensors
        self._coords = {}          # G -> device (G,A,3) staging of host coordinates
        self._dip = {}             # G -> device (G,3,N,N) dipole integrals
        self._ipdip = {}           # G -> device (G,3,3,N,N) their gradient (field_device.FieldProducer)
        self._field = {}           # G -> device (G,3) staging of host fields
        self._ws = None

    @classmethod
    def from_mol(cls, mol, device=None) -> "DeviceGaussians":
        """For a ``GaussianMol``: its charges, shells, normalisation and electron numbers."""
        return cls(charges=mol.charges, shells=mol.shells, nelec=mol.nelec, renormalize=mol.renormalize, device=device)

    @property
    def natm(self) -> int:
        return int(self._charges_host.shape[0])

    @property
    def charges(self) -> torch.Tensor:
        """Nuclear charges, device (A,)."""
        return self._charges

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
        shape = tuple(coords.shape)
        if len(shape) < 2 or shape[-1] != 3:
            raise ValueError("coords must be (G,A,3) or (A,3)")
        if shape[-2] != self.natm:
            raise ValueError(f"coordinates of {shape[-2]} centres for a molecule of {self.natm}")
        if torch.is_tensor(coords):
            return coords.to(device=self.device, dtype=F64).reshape(-1, self.natm, 3).contiguous()
        host = np.ascontiguousarray(coords, dtype=np.float64).reshape(-1, self.natm, 3)
        G = host.shape[0]
        R = self._coords.get(G)
        if R is None:
            R = self._coords[G] = torch.empty((G, self.natm, 3), dtype=F64, device=self.device)
        R.copy_(torch.from_numpy(host))
        return R

    def staged_coords(self, G: int) -> torch.Tensor:
        """The device (G,A,3) copy of the HOST coordinates the last ``integrals`` / ``dipole_integrals`` call of ``G``
        geometries uploaded: what a following device call on the same geometries reads without a second upload."""
        return self._coords[int(G)]

    def _basis_args(self):
        return (self.shell_atom.ctypes.data, self.shell_l.ctypes.data, self.shell_prim_offset.ctypes.data,
                self.exponents.ctypes.data, self.coefficients.ctypes.data)

    def dipole_integrals(self, coords, origin=(0.0, 0.0, 0.0)) -> torch.Tensor:
        """AO dipole integrals ``<mu| r - origin |nu>`` at ``coords`` as a device (G,3,N,N) tensor
        (``evc_spgto_dipole_batch``; host statement: ``GaussianMol.dipole_integrals``), enqueued on the current stream.
        The tensor is kept per G: a later call of the same G overwrites it."""
        R = self._device_coords(coords)
        G = int(R.shape[0])
        dip = self._dip.get(G)
        if dip is None:
            dip = self._dip[G] = torch.zeros((G, 3, self.nao, self.nao), dtype=F64, device=self.device)
        o = (C.c_double * 3)(*[float(x) for x in origin])
        _lib.check(getattr(self.lib, self._DIPOLE)(
            self.natm, int(self.shell_l.shape[0]), G, R.data_ptr(), *self._basis_args(), C.cast(o, C.c_void_p),
            dip.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream), self._DIPOLE)
        return dip

    def _nao_now(self) -> int:
        return self.nao

    def _ipdip_call(self, R, G, origin, ipdip) -> None:
        """One general kernel for l <= 2 serves this class and ``DeviceSpdGaussians``."""
        _lib.check(self.lib.evc_gto_dipole_grad_batch(
            self.natm, int(self.shell_l.shape[0]), G, R.data_ptr(), *self._basis_args(), origin, ipdip.data_ptr(),
            torch.cuda.current_stream(self.device).cuda_stream), "evc_gto_dipole_grad_batch")

    def integrals(self, coords, need_grad: bool = True, packed: bool = False, out: Optional[dict] = None, field=None,
                  origin=(0.0, 0.0, 0.0)) -> DeviceAOBatch:
        """The integrals at ``coords`` ((G,A,3) or (A,3), Bohr; numpy or a device tensor), enqueued on the current
        stream of the device.  ``packed``: ``eri`` as the dense (Ms,Ms) s4 matrix and ``eri_ip1`` packed in its last two
        indices (s2kl), what evaluators on the compressed layout read.  ``out``: a dict of tensors as ``allocate``
        returns to write into, instead of the buffers this object keeps for the shape.
        ``field``: None, or a uniform electric field ((3,) or one per geometry (G,3), atomic units; numpy or a device
        tensor) with the dipole operator's ``origin``: behind the integrals the call then enqueues the dipole integrals,
        their gradient (with ``need_grad``) and the fold of the field into ``hcore``, ``dhcore``, ``enuc`` and ``gnuc``
        (``evc_field_fold_batch``).  Without a field nothing more than the integrals is enqueued."""
        R = self._device_coords(coords)
        G, A = int(R.shape[0]), self.natm
        need_grad, packed = bool(need_grad), bool(packed)
        if out is None:
            key = (G, need_grad, packed)
            out = self._buffers.get(key)
            if out is None:
                out = self._buffers[key] = self.allocate(G, need_grad, packed)
        nshell = int(self.shell_l.shape[0])
        nbytes = getattr(self.lib, self._WORKSPACE)(A, nshell, int(self.exponents.shape[0]), self.nao, G)
        if nbytes == 0:
            raise _lib.EvcontHipError(self._WORKSPACE + ": " + self.lib.evc_last_error().decode())
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        flags = (0 if need_grad else _lib.FLAG_ENERGY_ONLY) | \
                ((_lib.FLAG_ERI_S4 | _lib.FLAG_IP1_S2KL) if packed else 0)
        cs = _lib.SgtoOutputs(**{k: (out[k].data_ptr() if out.get(k) is not None else None) for k in _FIELDS})
        _lib.check(getattr(self.lib, self._INTEGRALS)(
            A, nshell, G, R.data_ptr(), self._charges.data_ptr(), *self._basis_args(), C.byref(cs), flags,
            self._ws.data_ptr(), int(self._ws.numel()), torch.cuda.current_stream(self.device).cuda_stream),
            self._INTEGRALS)
        if field is not None:
            self._fold_field(R, out, need_grad, field, origin)
        return DeviceAOBatch(S=out["S"], hcore=out["hcore"], eri=out["eri"], enuc=out["enuc"], natm=A,
                             ipovlp=out.get("ipovlp"), dhcore=out.get("dhcore"), eri_ip1=out.get("eri_ip1"),
                             gnuc=out.get("gnuc"), aoslices=self._aoslices, ip1_s2kl=packed and need_grad,
                             eri_s4=packed)
