"""AO integrals (and their first nuclear derivatives) for molecules built from contracted Cartesian s and p Gaussian
shells: water, the H2O-H3O+ dimer and Zundel in STO-3G or 6-31G, the systems of the reference's MD workloads
(``md_H2O_6_31G_FCI.py``), with nothing third-party.  The arrays, their meanings and their signs are those of
``evcont_amd.hchain`` (which remains the statement, and the fast route, for one s function per centre):

    S, hcore, eri, ipovlp, dhcore, eri_ip1, enuc, gnuc

AO order: atoms, then the atom's shells in the given order, then p as x, y, z.

This module is the s+p entry point of the host statement ``evcont_amd.gto_host`` (numpy, clarity over speed), which it
always calls with the Hermite orders of lmax = 1; it holds the molecule class, the s+p basis tables and the geometries.
``evcont_amd.gto_device`` computes the same arrays on the device from the coordinates (``csrc/spgto.hip``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import gto_host
from .gto_host import (BOYS_CROSSOVER, BOYS_SERIES_TERMS, boys, contraction_coefficients,   # noqa: F401 (re-exported)
                       dipole_grad_from_primitives, element_shells, flatten_shells, hermite_E, hermite_R,
                       primitive_norm, shell_self_overlap)
from .synthetic import AOArrays


class Shell(gto_host.Shell):
    """A contracted Cartesian shell: ``l`` 0 (s) or 1 (p: x, y, z), exponents and the contraction coefficients of
    NORMALISED primitives, as published tables give them."""

    def __post_init__(self):
        if int(self.l) not in (0, 1):
            raise ValueError(f"Shell: l={int(self.l)}, supported 0 and 1")
        super().__post_init__()


# ---- basis tables (data): element -> list of (exponents, s coefficients, p coefficients or None) -------------------
STO3G = {
    "H": [((3.42525091, 0.62391373, 0.16885540), (0.15432897, 0.53532814, 0.44463454), None)],
    "O": [((130.70932, 23.808861, 6.4436083), (0.15432897, 0.53532814, 0.44463454), None),
          ((5.0331513, 1.1695961, 0.3803890), (-0.09996723, 0.39951283, 0.70011547),
           (0.15591627, 0.60768372, 0.39195739))],
}
G631 = {
    "H": [((18.7311370, 2.8253937, 0.6401217), (0.03349460, 0.23472695, 0.81375733), None),
          ((0.1612778,), (1.0,), None)],
    "O": [((5484.6717, 825.23495, 188.04696, 52.9645, 16.89757, 5.7996353),
           (0.0018311, 0.0139501, 0.0684451, 0.2327143, 0.470193, 0.3585209), None),
          ((15.539616, 3.5999336, 1.0137618), (-0.1107775, -0.1480263, 1.130767), (0.0708743, 0.3397528, 0.7271586)),
          ((0.2700058,), (1.0,), (1.0,))],
}
BASES = {"sto-3g": STO3G, "6-31g": G631}
_ELEMENTS = {"H": (1.0, 1.008), "O": (8.0, 15.999)}          # symbol -> (nuclear charge, mass in amu)


@dataclass
class GaussianMol(AOArrays):
    """``AOArrays`` of a geometry plus what the training-state generators and the MD drivers ask a ``mol`` for."""
    coords: Optional[np.ndarray] = None   # (A,3) Bohr
    nelec: Tuple[int, int] = (0, 0)
    charges: Optional[np.ndarray] = None
    shells: Optional[list] = None         # per atom: list of Shell
    renormalize: bool = True
    field: Optional[np.ndarray] = None    # (3,) the uniform electric field the arrays carry (``with_field``)
    field_origin: Tuple[float, float, float] = (0.0, 0.0, 0.0)

    def energy_nuc(self) -> float:
        return float(self.enuc)

    def atom_coords(self) -> np.ndarray:
        return np.array(self.coords, copy=True)

    def atom_mass_list(self) -> np.ndarray:
        """Atomic masses in amu, by nuclear charge (H and O)."""
        by_charge = {int(z): m for z, m in _ELEMENTS.values()}
        out = []
        for z in np.asarray(self.charges):
            if float(z) != int(z) or int(z) not in by_charge:
                raise ValueError(f"atom_mass_list: no mass for nuclear charge {z} (known: H, O)")
            out.append(by_charge[int(z)])
        return np.array(out)

    def with_coords(self, coords, need_grad: bool = True) -> "GaussianMol":
        """The same molecule (basis, charges, electrons, field) at new nuclear positions (Bohr)."""
        from .field import keep_field
        return keep_field(self, sp_gaussian_mol(coords, self.charges, self.shells, need_grad, self.nelec,
                                                self.renormalize))

    def with_field(self, F, origin=(0.0, 0.0, 0.0)) -> "GaussianMol":
        """A copy in the uniform electric field ``F`` (3,) (``evcont_amd.field.with_field``)."""
        from .field import with_field
        return with_field(self, F, origin)

    def dipole_grad_integrals(self, origin=(0.0, 0.0, 0.0)) -> np.ndarray:
        """``ipdip[x,c,mu,nu] = <d_x mu| r_c - origin_c |nu>`` (3,3,N,N): the electron-coordinate gradient on the bra
        (the convention of ``ipovlp``), so ``d dip_c[mu,nu] / dR_Ax = -ipdip[x,c,mu,nu] [mu in A] - ipdip[x,c,nu,mu]
        [nu in A]``."""
        return gto_host.dipole_grad_integrals(self.coords, self.shells, origin, self.renormalize)

    def dipole_integrals(self, origin=(0.0, 0.0, 0.0)) -> np.ndarray:
        """AO dipole integrals ``<mu| r - origin |nu>`` (3,N,N) (PySCF: ``int1e_r`` under ``with_common_orig``)."""
        return gto_host.dipole_integrals(self.coords, self.shells, origin, self.renormalize)


def sp_gaussian_mol(coords, charges, shells, need_grad: bool = True, nelec: Optional[Tuple[int, int]] = None,
                    renormalize: bool = True) -> GaussianMol:
    """AO arrays of a molecule of s and p shells (``coords`` (A,3) Bohr, ``shells`` per atom a list of ``Shell``)."""
    return GaussianMol(**gto_host.gaussian_arrays("sp_gaussian_mol", 1, coords, charges, shells, need_grad, nelec,
                                                  renormalize))


ANGSTROM = 1.8897261246257702          # Bohr per Angstrom


def molecule(symbols: Sequence[str], coords, basis="sto-3g", need_grad: bool = True, charge: int = 0) -> GaussianMol:
    """A molecule of H and O atoms (``coords`` Bohr) in a tabulated basis ("sto-3g", "6-31g" or a table)."""
    table = BASES[basis.lower()] if isinstance(basis, str) else basis
    Z = [_ELEMENTS[s][0] for s in symbols]
    ne = int(round(sum(Z))) - int(charge)
    return sp_gaussian_mol(coords, Z, [element_shells(table, s) for s in symbols], need_grad,
                           ((ne + 1) // 2, ne // 2))


def water_coords(r_oh: float = 0.9572 * ANGSTROM, angle: float = 104.52) -> np.ndarray:
    """H2O in the xy plane, O at the origin, ``r_oh`` in Bohr and ``angle`` (HOH) in degrees; atoms O, H, H."""
    h = np.radians(angle) / 2.0
    return np.array([[0.0, 0.0, 0.0], [r_oh * np.sin(h), r_oh * np.cos(h), 0.0], [-r_oh * np.sin(h), r_oh * np.cos(h), 0.0]])


def water(basis="sto-3g", r_oh: float = 0.9572 * ANGSTROM, angle: float = 104.52, need_grad: bool = True) -> GaussianMol:
    """H2O at ``water_coords(r_oh, angle)``."""
    return molecule(("O", "H", "H"), water_coords(r_oh, angle), basis, need_grad)


def zundel(basis="6-31g", r_oo: float = 2.4 * ANGSTROM, need_grad: bool = True) -> GaussianMol:
    """H5O2+ (Zundel): two waters facing a shared proton at the midpoint of O ... O (along x), the water planes twisted
    by 90 degrees against each other; atoms O, H, H, O, H, H, H.  A plausible start geometry, not a minimum."""
    r, h = 0.97 * ANGSTROM, np.radians(109.0) / 2.0
    out, side = r * np.cos(h) * 0.6, r * np.sin(h)
    half = r_oo / 2.0
    coords = np.array([[-half, 0.0, 0.0], [-half - out, side, 0.3], [-half - out, -side, 0.3],
                       [half, 0.0, 0.0], [half + out, 0.3, side], [half + out, 0.3, -side],
                       [0.0, 0.0, 0.0]])
    return molecule(("O", "H", "H", "O", "H", "H", "H"), coords, basis, need_grad, charge=1)
