"""AO integrals (and their first nuclear derivatives) for molecules built from contracted s, p, d and f Gaussian shells,
d and f as the five and seven REAL SPHERICAL functions, with nothing third-party: the shape of water in cc-pVTZ (an f
shell on O, a d shell on each H), the system of the reference's ``md_H2O_vtz_CAS_continuation.py``.  The arrays, their
meanings and their signs are those of ``evcont_amd.gto_spd`` (which remains the entry point, and the route, for molecules
with l <= 2):

    S, hcore, eri, ipovlp, dhcore, eri_ip1, enuc, gnuc

AO order: atoms, then the atom's shells in the given order, p as x, y, z, d as m = -2 ... 2, f as m = -3 ... 3 (PySCF's
order), for primitives normalised as x y z exp(-a r^2):

    y (3x^2 - y^2) / sqrt(24), x y z, y (4z^2 - x^2 - y^2) / sqrt(40), z (2z^2 - 3x^2 - 3y^2) / sqrt(60),
    x (4z^2 - x^2 - y^2) / sqrt(40), z (x^2 - y^2) / 2, x (x^2 - 3y^2) / sqrt(24)

This module is the s+p+d+f entry point of the host statement ``evcont_amd.gto_host`` (numpy, clarity over speed), which
it always calls with the Hermite orders of lmax = 3 (Hermite total 13 in ``eri_ip1``, Boys functions F0 ... F13), whether
the molecule has f shells or not.  It holds no basis table: nothing here can check the numbers of cc-pVTZ, so a basis is
passed as a table of ``(l, exponents, coefficients)`` entries.  ``evcont_amd.gto_spdf_device`` computes the same arrays on
the device from the coordinates (``csrc/spdfgto.hip``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

from . import gto_host
from .gto_host import (D_MONOMIALS, F_MONOMIALS, boys, contraction_coefficients, dipole_grad_integrals,   # noqa: F401
                       dipole_integrals, flatten_shells, hermite_E, hermite_R, monomials, primitive_norm,
                       shell_self_overlap)                                                   # (re-exported)
from .gto_small import ANGSTROM, GaussianMol, _ELEMENTS, water_coords                        # noqa: F401 (re-exported)


class Shell(gto_host.Shell):
    """A contracted shell: ``l`` 0 (s), 1 (p: x, y, z), 2 (d: five real spherical functions) or 3 (f: seven), exponents
    and the contraction coefficients of NORMALISED primitives, as published tables give them."""
    _LS = (0, 1, 2, 3)


def element_shells(table, symbol: str):
    """The shells of one atom from a basis table whose entries are (l, exponents, coefficients), l <= 3."""
    return [Shell(*entry) for entry in table[symbol]]


@dataclass
class SpdfGaussianMol(GaussianMol):
    """``GaussianMol`` of a molecule whose shells may have l = 3 (``shells``: per atom a list of this module's
    ``Shell``)."""

    def with_coords(self, coords, need_grad: bool = True) -> "SpdfGaussianMol":
        """The same molecule (basis, charges, electrons, field) at new nuclear positions (Bohr)."""
        from .field import keep_field
        return keep_field(self, spdf_gaussian_mol(coords, self.charges, self.shells, need_grad, self.nelec,
                                                  self.renormalize))


def spdf_gaussian_mol(coords, charges, shells, need_grad: bool = True, nelec: Optional[Tuple[int, int]] = None,
                      renormalize: bool = True) -> SpdfGaussianMol:
    """AO arrays of a molecule of s, p, spherical d and spherical f shells (``coords`` (A,3) Bohr, ``shells`` per atom a
    list of ``Shell``)."""
    return SpdfGaussianMol(**gto_host.gaussian_arrays("spdf_gaussian_mol", 3, coords, charges, shells, need_grad, nelec,
                                                      renormalize))


def molecule(symbols: Sequence[str], coords, basis, need_grad: bool = True, charge: int = 0) -> SpdfGaussianMol:
    """A molecule of H and O atoms (``coords`` Bohr) in the basis ``basis``: a table element -> list of
    (l, exponents, coefficients)."""
    Z = [_ELEMENTS[s][0] for s in symbols]
    ne = int(round(sum(Z))) - int(charge)
    return spdf_gaussian_mol(coords, Z, [element_shells(basis, s) for s in symbols], need_grad,
                             ((ne + 1) // 2, ne // 2))


def water(basis, r_oh: float = 0.9572 * ANGSTROM, angle: float = 104.52, need_grad: bool = True) -> SpdfGaussianMol:
    """H2O in the xy plane, O at the origin, ``r_oh`` in Bohr and ``angle`` (HOH) in degrees; atoms O, H, H."""
    return molecule(("O", "H", "H"), water_coords(r_oh, angle), basis, need_grad)


def water_shells(basis):
    """(charges, shells per atom) of water, atoms O, H, H, without any integral: what the device object needs."""
    return [_ELEMENTS[s][0] for s in "OHH"], [element_shells(basis, s) for s in "OHH"]
