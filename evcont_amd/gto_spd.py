"""AO integrals (and their first nuclear derivatives) for molecules built from contracted s, p and d Gaussian shells, the
d shells as the five REAL SPHERICAL functions: water in cc-pVDZ, the system of the reference's
``md_H2O_vdz_CAS_continuation.py``, with nothing third-party.  The arrays, their meanings and their signs are those of
``evcont_amd.gto_small`` (which remains the entry point, and the route, for molecules of s and p shells alone):

    S, hcore, eri, ipovlp, dhcore, eri_ip1, enuc, gnuc

AO order: atoms, then the atom's shells in the given order, p as x, y, z, d as m = -2 ... 2 (PySCF's order):

    xy, yz, 2z^2 - x^2 - y^2, xz, x^2 - y^2

This module is the s+p+d entry point of the host statement ``evcont_amd.gto_host`` (numpy, clarity over speed: water /
cc-pVDZ takes minutes), which it always calls with the Hermite orders of lmax = 2, whether the molecule has d shells or
not; it holds the molecule class and the cc-pVDZ table.  ``evcont_amd.gto_spd_device`` computes the same arrays on the
device from the coordinates (``csrc/spdgto.hip``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

from . import gto_host, gto_small
from .gto_host import (D_MONOMIALS, Shell, boys, contraction_coefficients, dipole_grad_integrals,   # noqa: F401
                       dipole_integrals, element_shells, flatten_shells, hermite_E, hermite_R, monomials,
                       primitive_norm, shell_self_overlap)                                   # (re-exported)
from .gto_small import ANGSTROM, GaussianMol, _ELEMENTS, water_coords                        # noqa: F401 (re-exported)

# ---- basis tables (data) ---------------------------------------------------------------------------------------------
# cc-pVDZ (Dunning 1989) for H and O: element -> list of (l, exponents, coefficients).  The table is generally
# contracted; it is written here as segmented shells that repeat the primitives.
_O_S = (11720.0, 1759.0, 400.8, 113.7, 37.03, 13.27, 5.025, 1.013)
CCPVDZ = {
    "H": [(0, (13.01, 1.962, 0.4446), (0.019685, 0.137977, 0.478148)),
          (0, (0.122,), (1.0,)),
          (1, (0.727,), (1.0,))],
    "O": [(0, _O_S, (0.000710, 0.005470, 0.027837, 0.104800, 0.283062, 0.448719, 0.270952, 0.015458)),
          (0, _O_S, (-0.000160, -0.001263, -0.006267, -0.025716, -0.070924, -0.165411, -0.116955, 0.557368)),
          (0, (0.3023,), (1.0,)),
          (1, (17.70, 3.854, 1.046), (0.043018, 0.228913, 0.508728)),
          (1, (0.2753,), (1.0,)),
          (2, (1.185,), (1.0,))],
}
BASES = dict(gto_small.BASES)
BASES["cc-pvdz"] = CCPVDZ


@dataclass
class SpdGaussianMol(GaussianMol):
    """``GaussianMol`` of a molecule whose shells may have l = 2 (``shells``: per atom a list of this module's
    ``Shell``)."""

    def with_coords(self, coords, need_grad: bool = True) -> "SpdGaussianMol":
        """The same molecule (basis, charges, electrons, field) at new nuclear positions (Bohr)."""
        from .field import keep_field
        return keep_field(self, spd_gaussian_mol(coords, self.charges, self.shells, need_grad, self.nelec,
                                                 self.renormalize))


def spd_gaussian_mol(coords, charges, shells, need_grad: bool = True, nelec: Optional[Tuple[int, int]] = None,
                     renormalize: bool = True) -> SpdGaussianMol:
    """AO arrays of a molecule of s, p and spherical d shells (``coords`` (A,3) Bohr, ``shells`` per atom a list of
    ``Shell``)."""
    return SpdGaussianMol(**gto_host.gaussian_arrays("spd_gaussian_mol", 2, coords, charges, shells, need_grad, nelec,
                                                     renormalize))


def molecule(symbols: Sequence[str], coords, basis="sto-3g", need_grad: bool = True, charge: int = 0) -> SpdGaussianMol:
    """A molecule of H and O atoms (``coords`` Bohr) in a tabulated basis ("sto-3g", "6-31g", "cc-pvdz" or a table)."""
    table = BASES[basis.lower()] if isinstance(basis, str) else basis
    Z = [_ELEMENTS[s][0] for s in symbols]
    ne = int(round(sum(Z))) - int(charge)
    return spd_gaussian_mol(coords, Z, [element_shells(table, s) for s in symbols], need_grad,
                            ((ne + 1) // 2, ne // 2))


def water(basis="sto-3g", r_oh: float = 0.9572 * ANGSTROM, angle: float = 104.52, need_grad: bool = True) -> SpdGaussianMol:
    """H2O in the xy plane, O at the origin, ``r_oh`` in Bohr and ``angle`` (HOH) in degrees; atoms O, H, H."""
    return molecule(("O", "H", "H"), water_coords(r_oh, angle), basis, need_grad)


def water_shells(basis="cc-pvdz"):
    """(charges, shells per atom) of water, atoms O, H, H, without any integral: what the device object needs."""
    table = BASES[basis.lower()] if isinstance(basis, str) else basis
    return [_ELEMENTS[s][0] for s in "OHH"], [element_shells(table, s) for s in "OHH"]
