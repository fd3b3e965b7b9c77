"""Device route of ``evcont_amd.gto_spd.spd_gaussian_mol``: the AO integrals (and their first nuclear derivatives) of a
molecule of contracted s, p and real spherical d Gaussian shells, computed on the GPU from the coordinates
(``evc_spdgto_integrals_batch``, ``csrc/spdgto.hip``) and written straight into the arrays the evaluators read.

    dg = DeviceSpdGaussians(*gto_spd.water_shells("cc-pvdz"))
    aob = dg.integrals(R)                      # R (G,A,3) Bohr, numpy or a device tensor -> DeviceAOBatch
    mol = dg.to_mol(R0)                        # one geometry's arrays as a host molecule, for the training containers

The interface, the buffers kept per shape and the staging of host coordinates are those of
``gto_device.DeviceGaussians`` (which stays the route for molecules of s and p shells alone); this class names its own C
calls.  ``to_mol`` downloads one geometry into the host molecule class of
``gto_spd`` without running the numpy statement, which takes minutes at N = 24.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from .gto_device import DeviceGaussians
from .gto_spd import SpdGaussianMol

_HOST_FIELDS = ("S", "hcore", "eri", "ipovlp", "dhcore", "eri_ip1", "gnuc")


@dataclass
class DeviceMadeMol(SpdGaussianMol):
    """A ``SpdGaussianMol`` whose arrays came from the device; ``with_coords`` goes back through the device."""
    producer: Optional["DeviceSpdGaussians"] = None

    def with_coords(self, coords, need_grad: bool = True) -> "DeviceMadeMol":
        from .field import keep_field
        return keep_field(self, self.producer.to_mol(coords, need_grad))

    def dipole_integrals(self, origin=(0.0, 0.0, 0.0)) -> np.ndarray:
        return self.producer.dipole_integrals(self.coords, origin)[0].cpu().numpy()

    def dipole_grad_integrals(self, origin=(0.0, 0.0, 0.0)) -> np.ndarray:
        return self.producer.dipole_grad_integrals(self.coords, origin)[0].cpu().numpy()


class DeviceSpdGaussians(DeviceGaussians):
    """``shells``: per atom a list of ``gto_spd.Shell`` (l <= 2); ``charges``: the nuclear charges; ``renormalize``: scale
    every contracted function to unit self-overlap (on the host, once), as ``spd_gaussian_mol`` does."""

    _WORKSPACE, _INTEGRALS, _DIPOLE = ("evc_spdgto_workspace_bytes", "evc_spdgto_integrals_batch",
                                       "evc_spdgto_dipole_batch")
    # what ``gto_spdf_device.DeviceSpdfGaussians`` sets anew: the accepted l and the molecule class of ``to_mol``
    _LS = (0, 1, 2)
    _MOL = DeviceMadeMol

    def __init__(self, charges, shells, nelec=None, renormalize: bool = True, device=None):
        for atom in shells:
            for sh in atom:
                if sh.l not in self._LS:
                    raise ValueError(f"{type(self).__name__}: shell with l={sh.l}, supported "
                                     f"{', '.join(map(str, self._LS[:-1]))} and {self._LS[-1]}")
        super().__init__(charges, shells, nelec=nelec, renormalize=renormalize, device=device)

    def to_mol(self, coords, need_grad: bool = True) -> DeviceMadeMol:
        """The arrays of ONE geometry (``coords`` (A,3) Bohr) as a host molecule (full forms); without ``need_grad`` the
        derivative arrays are zeros of the shapes ``spd_gaussian_mol`` gives them."""
        R = np.ascontiguousarray(coords, dtype=np.float64).reshape(1, self.natm, 3)
        out = self.allocate(1, need_grad, packed=False)
        self.integrals(R, need_grad=need_grad, packed=False, out=out)
        host = {k: out[k][0].cpu().numpy() for k in _HOST_FIELDS if k in out}
        n, A = self.nao, self.natm
        if not need_grad:
            host.update(ipovlp=np.zeros((3, n, n)), dhcore=np.zeros((A, 3, n, n)), eri_ip1=np.zeros((3, 0)),
                        gnuc=np.zeros((A, 3)))
        nelec = self.nelec
        if nelec is None:
            ne = int(round(float(self._charges_host.sum())))
            nelec = ((ne + 1) // 2, ne // 2)
        return self._MOL(aoslices=self._aoslices.cpu().numpy(), enuc=float(out["enuc"][0].cpu()),
                         integral_symmetry=True, coords=R[0].copy(), nelec=tuple(nelec),
                         charges=self._charges_host.copy(), shells=self.shells, renormalize=self.renormalize,
                         producer=self, **host)
