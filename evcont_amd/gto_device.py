"""Device route of ``evcont_amd.gto_small.sp_gaussian_mol``: the AO integrals (and their first nuclear derivatives) of a
molecule of contracted Cartesian s and p Gaussian shells, computed on the GPU from the coordinates
(``evc_spgto_integrals_batch``, ``csrc/spgto.hip``) and written straight into the arrays the evaluators read.

    dg = DeviceGaussians.from_mol(gto_small.water("sto-3g"))
    aob = dg.integrals(R)                      # R (G,A,3) Bohr, numpy or a device tensor -> DeviceAOBatch
    E, C, grads = batched_evaluator.multistate_energies_with_grads(aob, nroots)

The interface is that of ``hchain_device.DeviceSGaussians`` (which stays the route for one s function per centre).  The
outputs live in buffers the object keeps per ``(G, need_grad, packed)``, so a steady MD loop allocates nothing per step;
a later call of the same shape overwrites what the previous one returned.  All of that is ``producer.DeviceProducer``;
this class holds the flattened shells and names the C calls of the s+p route.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .gto_host import contraction_coefficients, flatten_shells
from .producer import DeviceProducer


class DeviceGaussians(DeviceProducer):
    """``shells``: per atom a list of ``gto_small.Shell``; ``charges``: the nuclear charges; ``renormalize``: scale every
    contracted function to unit self-overlap (on the host, once), as ``sp_gaussian_mol`` does."""

    # ``gto_spd_device.DeviceSpdGaussians`` names its own three; one dipole-gradient kernel for l <= 2 serves both
    _WORKSPACE, _INTEGRALS, _DIPOLE = "evc_spgto_workspace_bytes", "evc_spgto_integrals_batch", "evc_spgto_dipole_batch"
    _DIPOLE_GRAD = "evc_gto_dipole_grad_batch"

    def __init__(self, charges: Sequence[float], shells, nelec: Optional[Tuple[int, int]] = None,
                 renormalize: bool = True, device=None):
        super().__init__(device)
        self.shells = [list(atom) for atom in shells]
        self._charges_host = np.ascontiguousarray(charges, dtype=np.float64).reshape(-1)
        if len(self.shells) != self._charges_host.shape[0]:
            raise ValueError(f"{len(self.shells)} shell lists for {self._charges_host.shape[0]} charges")
        self.nelec = None if nelec is None else tuple(nelec)
        self.renormalize = bool(renormalize)
        # the HOST description of the basis every call passes
        (self.shell_atom, self.shell_l, self.shell_prim_offset, self.exponents, self.coefficients, slices,
         self.nao) = flatten_shells(self.shells, contraction_coefficients(self.shells, renormalize))
        self._nsets = int(self.shell_l.shape[0])            # the shells
        self._charges = torch.from_numpy(self._charges_host).to(self.device)
        self._aoslices = torch.from_numpy(slices).to(self.device)

    @classmethod
    def from_mol(cls, mol, device=None) -> "DeviceGaussians":
        """For a ``GaussianMol``: its charges, shells, normalisation and electron numbers."""
        return cls(charges=mol.charges, shells=mol.shells, nelec=mol.nelec, renormalize=mol.renormalize, device=device)

    def _basis_args(self):
        return (self.shell_atom.ctypes.data, self.shell_l.ctypes.data, self.shell_prim_offset.ctypes.data,
                self.exponents.ctypes.data, self.coefficients.ctypes.data)

    def _workspace_args(self, G: int):
        return self.natm, self._nsets, int(self.exponents.shape[0]), self.nao, G
