"""Device route of ``evcont_amd.hchain.s_gaussian_mol``: the AO integrals (and their first nuclear derivatives) of a
molecule built from one contracted s Gaussian per centre, computed on the GPU from the coordinates
(``evc_sgto_integrals_batch``, ``csrc/sgto.hip``) and written straight into the arrays the evaluators read.

    sg = DeviceSGaussians.from_mol(hydrogen_chain(10, 1.8))
    aob = sg.integrals(R)                      # R (G,A,3) Bohr, numpy or a device tensor -> DeviceAOBatch
    E, C, grads = batched_evaluator.multistate_energies_with_grads(aob, nroots)

The outputs live in buffers the object keeps per ``(G, need_grad, packed)``, so a steady MD loop allocates nothing per
step; a later call of the same shape overwrites what the previous one returned.  All of that is
``producer.DeviceProducer``; this class holds the contraction and names the C calls of the s route.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .hchain import STO3G_H_COEFFICIENTS, STO3G_H_EXPONENTS
from .producer import DeviceProducer


class DeviceSGaussians(DeviceProducer):
    """One contracted s function (``exponents``, ``coefficients`` of normalised primitives) on every centre of a molecule
    with nuclear ``charges`` (default: 1 on each of the centres of the first ``integrals`` call)."""

    _WORKSPACE, _INTEGRALS = "evc_sgto_workspace_bytes", "evc_sgto_integrals_batch"
    _DIPOLE, _DIPOLE_GRAD = "evc_sgto_dipole_batch", "evc_sgto_dipole_grad_batch"

    def __init__(self, charges: Optional[Sequence[float]] = None, exponents: Sequence[float] = STO3G_H_EXPONENTS,
                 coefficients: Sequence[float] = STO3G_H_COEFFICIENTS, nelec: Optional[Tuple[int, int]] = None,
                 device=None):
        super().__init__(device)
        self.exponents = np.ascontiguousarray(exponents, dtype=np.float64)
        self.coefficients = np.ascontiguousarray(coefficients, dtype=np.float64)
        if self.exponents.ndim != 1 or self.exponents.shape != self.coefficients.shape:
            raise ValueError("exponents and coefficients must be one-dimensional and of one length")
        self.nelec = None if nelec is None else tuple(nelec)
        self._charges_host = None if charges is None else np.ascontiguousarray(charges, dtype=np.float64).reshape(-1)
        self._nsets = int(self.exponents.shape[0])          # the primitives of the one contraction

    @classmethod
    def from_mol(cls, mol, device=None) -> "DeviceSGaussians":
        """For an ``HChainMol``: its charges, contraction and electron numbers."""
        return cls(charges=mol.charges, exponents=mol.exponents, coefficients=mol.coefficients, nelec=mol.nelec,
                   device=device)

    @property
    def nao(self) -> Optional[int]:
        return self.natm

    def _setup(self, A: int) -> None:
        """The charges (and with them ``natm``, None until then) are fixed at the first call."""
        if self._charges is None:
            z = np.ones(A) if self._charges_host is None else self._charges_host
            self._charges = torch.from_numpy(z).to(self.device)
            self._aoslices = torch.from_numpy(
                np.stack([np.arange(len(z)), np.arange(len(z)) + 1], axis=1).astype(np.int64)).to(self.device)
        super()._setup(A)

    def _basis_args(self):
        return self.exponents.ctypes.data, self.coefficients.ctypes.data

    def _workspace_args(self, G: int):
        return self.natm, self._nsets, G
