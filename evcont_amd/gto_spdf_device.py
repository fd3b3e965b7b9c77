"""Device route of ``evcont_amd.gto_spdf.spdf_gaussian_mol``: the AO integrals (and their first nuclear derivatives) of a
molecule of contracted s, p, real spherical d and real spherical f Gaussian shells, computed on the GPU from the
coordinates (``evc_spdfgto_integrals_batch``, ``csrc/spdfgto.hip``) and written straight into the arrays the evaluators
read.

    dg = DeviceSpdfGaussians(*gto_spdf.water_shells(table))
    aob = dg.integrals(R)                      # R (G,A,3) Bohr, numpy or a device tensor -> DeviceAOBatch
    mol = dg.to_mol(R0)                        # one geometry's arrays as a host molecule, for the training containers

The interface, the buffers kept per shape, the staging of host coordinates, the dipole integrals and the fold of a
uniform field are those of ``gto_spd_device.DeviceSpdGaussians`` (which stays the route for molecules with l <= 2); this
class names its own four C calls, the dipole-gradient call included (``evc_gto_dipole_grad_batch`` stops at l = 2).
``to_mol`` downloads one geometry into the host molecule class of ``gto_spdf`` without running the numpy statement.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from .gto_spd_device import DeviceSpdGaussians
from .gto_spdf import SpdfGaussianMol


@dataclass
class DeviceMadeSpdfMol(SpdfGaussianMol):
    """A ``SpdfGaussianMol`` whose arrays came from the device; ``with_coords`` goes back through the device."""
    producer: Optional["DeviceSpdfGaussians"] = None

    def with_coords(self, coords, need_grad: bool = True) -> "DeviceMadeSpdfMol":
        from .field import keep_field
        return keep_field(self, self.producer.to_mol(coords, need_grad))

    def dipole_integrals(self, origin=(0.0, 0.0, 0.0)) -> np.ndarray:
        return self.producer.dipole_integrals(self.coords, origin)[0].cpu().numpy()

    def dipole_grad_integrals(self, origin=(0.0, 0.0, 0.0)) -> np.ndarray:
        return self.producer.dipole_grad_integrals(self.coords, origin)[0].cpu().numpy()


class DeviceSpdfGaussians(DeviceSpdGaussians):
    """``shells``: per atom a list of ``gto_spdf.Shell`` (l <= 3); ``charges``: the nuclear charges; ``renormalize``:
    scale every contracted function to unit self-overlap (on the host, once), as ``spdf_gaussian_mol`` does."""

    _WORKSPACE, _INTEGRALS, _DIPOLE = ("evc_spdfgto_workspace_bytes", "evc_spdfgto_integrals_batch",
                                       "evc_spdfgto_dipole_batch")
    _DIPOLE_GRAD = "evc_spdfgto_dipole_grad_batch"
    _LS = (0, 1, 2, 3)
    _MOL = DeviceMadeSpdfMol
