"""Self-contained AO integrals (and their first nuclear derivatives) for molecules built from contracted s, p and d
Gaussian shells, the d shells as the five REAL SPHERICAL functions: water in cc-pVDZ, the system of the reference's
``md_H2O_vdz_CAS_continuation.py``, with nothing third-party.  The arrays, their meanings and their signs are those of
``evcont_amd.gto_small`` (which remains the statement, and the route, for molecules of s and p shells alone):

    S, hcore, eri, ipovlp, dhcore, eri_ip1, enuc, gnuc

AO order: atoms, then the atom's shells in the given order, p as x, y, z, d as m = -2 ... 2 (PySCF's order):

    xy, yz, 2z^2 - x^2 - y^2, xz, x^2 - y^2

Each d function is a fixed linear combination (``D_MONOMIALS``) of the Cartesian monomials of ONE primitive set; the
Cartesian s-type combination x^2 + y^2 + z^2 never appears.

Method: McMurchie-Davidson as in ``gto_small`` (whose ``hermite_E``, ``hermite_R`` and ``boys`` are general in their
orders and are used as they are), with general powers per dimension.  What is new here: the primitive FUNCTIONS carry a
power triple and a spherical weight (``_Primitives``), the primitive norm of l = 2, and the term ``j (j - 1)`` of the
kinetic energy that vanishes for j <= 1.  Highest orders: the derivative raises the first index to l + 1 = 3, the kinetic
energy the second to l + 2 = 4; Hermite total 9 in ``eri_ip1`` (8 in ``eri``), Boys functions F0 ... F9.

This module is the host statement (numpy, clarity over speed: water / cc-pVDZ takes minutes);
``evcont_amd.gto_spd_device`` computes the same arrays on the device from the coordinates (``csrc/spdgto.hip``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import gto_small
from .gto_small import ANGSTROM, GaussianMol, _ELEMENTS, boys, hermite_E, hermite_R   # noqa: F401 (re-exported)


@dataclass(frozen=True)
class Shell:
    """A contracted shell: ``l`` 0 (s), 1 (p: x, y, z) or 2 (d: the five real spherical functions), exponents and the
    contraction coefficients of NORMALISED primitives, as published tables give them."""
    l: int
    exponents: Tuple[float, ...]
    coefficients: Tuple[float, ...]

    def __post_init__(self):
        object.__setattr__(self, "l", int(self.l))
        object.__setattr__(self, "exponents", tuple(float(x) for x in self.exponents))
        object.__setattr__(self, "coefficients", tuple(float(x) for x in self.coefficients))
        if self.l not in (0, 1, 2):
            raise ValueError(f"Shell: l={self.l}, supported 0, 1 and 2")
        if len(self.exponents) != len(self.coefficients) or not self.exponents:
            raise ValueError("Shell: exponents and coefficients must have one length >= 1")
        if min(self.exponents) <= 0.0:
            raise ValueError("Shell: exponents must be positive")


# Per component of a d shell: ((powers of x, y, z), weight) of its monomials, for primitives normalised as x y exp(-a r^2)
# (``primitive_norm(2, a)``): every component then has the norm of the primitive.
_R3, _R12 = 1.0 / np.sqrt(3.0), 1.0 / np.sqrt(12.0)
D_MONOMIALS = (
    (((1, 1, 0), 1.0),),                                              # xy
    (((0, 1, 1), 1.0),),                                              # yz
    (((0, 0, 2), _R3), ((2, 0, 0), -_R12), ((0, 2, 0), -_R12)),       # 2 z^2 - x^2 - y^2
    (((1, 0, 1), 1.0),),                                              # xz
    (((2, 0, 0), 0.5), ((0, 2, 0), -0.5)),                            # x^2 - y^2
)


def monomials(l: int, comp: int):
    """((powers), weight) of the monomials of component ``comp`` of a shell of angular momentum ``l``."""
    if l == 0:
        return (((0, 0, 0), 1.0),)
    if l == 1:
        return ((tuple(int(comp == d) for d in range(3)), 1.0),)
    return D_MONOMIALS[comp]


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


def element_shells(table, symbol: str):
    """The shells of one atom: from a table of this module ((l, exponents, coefficients) entries) or from one of
    ``gto_small`` ((exponents, s coefficients, p coefficients or None) entries)."""
    out = []
    for entry in table[symbol]:
        if isinstance(entry[0], (int, np.integer)):
            out.append(Shell(*entry))
        else:
            ex, cs, cp = entry
            out.append(Shell(0, ex, cs))
            if cp is not None:
                out.append(Shell(1, ex, cp))
    return out


def primitive_norm(l: int, a):
    """Norm of a Cartesian primitive: exp(-a r^2), x exp(-a r^2) or x y exp(-a r^2) for l = 0, 1, 2."""
    a = np.asarray(a, dtype=np.float64)
    return (2.0 * a / np.pi) ** 0.75 * (1.0, 2.0 * np.sqrt(a), 4.0 * a)[l]


def shell_self_overlap(shell) -> float:
    """<f|f> of one contracted function of the shell with the tabulated coefficients (the same for every component)."""
    a = np.asarray(shell.exponents)
    c = np.asarray(shell.coefficients) * primitive_norm(shell.l, a)
    p = a[:, None] + a[None, :]
    s = (np.pi / p) ** 1.5 * (1.0, 0.5 / p, 0.25 / (p * p))[shell.l]
    return float(c @ s @ c)


def contraction_coefficients(shells, renormalize: bool = True):
    """Per atom and shell the coefficients of normalised primitives the integrals use: the tabulated ones, scaled to
    unit self-overlap of the contracted function with ``renormalize``."""
    return [[tuple(np.asarray(sh.coefficients) / (np.sqrt(shell_self_overlap(sh)) if renormalize else 1.0))
             for sh in atom] for atom in shells]


class _Primitives:
    """The primitive FUNCTIONS of a molecule, one per AO, primitive and monomial: exponent, weight (coefficient x norm x
    spherical weight), centre, power triple, and their pair quantities."""

    def __init__(self, coords, shells, renormalize):
        R = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
        coef = contraction_coefficients(shells, renormalize)
        a, cn, ctr, pw, ao, slices = [], [], [], [], [], []
        n = 0
        for at, atom in enumerate(shells):
            start = n
            for sh, cs in zip(atom, coef[at]):
                for comp in range(2 * sh.l + 1):
                    for ex, c in zip(sh.exponents, cs):
                        for powers, w in monomials(sh.l, comp):
                            a.append(ex)
                            cn.append(c * float(primitive_norm(sh.l, ex)) * w)
                            ctr.append(R[at])
                            pw.append(powers)
                            ao.append(n)
                    n += 1
            slices.append((start, n))
        self.a, self.cn, self.ctr = np.array(a), np.array(cn), np.array(ctr).reshape(-1, 3)
        self.pw, self.ao = np.array(pw, dtype=np.int64).reshape(-1, 3), np.array(ao, dtype=np.int64)
        self.nao, self.nprim = n, len(a)
        self.aoslices = np.array(slices, dtype=np.int64).reshape(-1, 2)
        self.Cm = np.zeros((self.nprim, n))
        self.Cm[np.arange(self.nprim), self.ao] = self.cn
        self.p = self.a[:, None] + self.a[None, :]
        self.AB = self.ctr[:, None, :] - self.ctr[None, :, :]
        # P = (a A + b B) / p; where A_x = B_x the centre exactly, so that P - Q and P - C vanish where they do
        # mathematically
        self.P = np.where(self.AB == 0.0, self.ctr[:, None, :],
                          (self.a[:, None, None] * self.ctr[:, None, :] + self.a[None, :, None] * self.ctr[None, :, :])
                          / self.p[:, :, None])

    def contract2(self, M):                                  # (..., Np, Np) -> (..., n, n)
        return np.einsum("pi,...pq,qj->...ij", self.Cm, M, self.Cm, optimize=True)

    def pair_E(self, imax, jmax):
        """Per dimension the array of ``hermite_E`` over all pairs of primitive functions."""
        return [hermite_E(imax, jmax, self.a[:, None], self.a[None, :], self.AB[:, :, d]) for d in range(3)]

    def pick(self, E, d, di, dj, rows=None):
        """``E_t`` (t first) of dimension d for every pair with the powers of the pair's functions shifted by di, dj;
        a power below 0 gives zeros.  ``rows``: restrict the first index."""
        i = self.pw[:, d][:, None] + di + 0 * self.pw[:, d][None, :]
        j = 0 * self.pw[:, d][:, None] + self.pw[:, d][None, :] + dj
        r, c = np.indices(i.shape)
        e = np.moveaxis(E[d][np.maximum(i, 0), np.maximum(j, 0), :, r, c], -1, 0) * ((i >= 0) & (j >= 0))
        return e if rows is None else e[:, rows]

    def center_derivative(self, f, d):
        """d/dA_d of a pair quantity given as ``f(di)`` (the first function's power in dimension d shifted by di):
        ``2a f(+1) - l f(-1)``."""
        return 2.0 * self.a[:, None] * f(1) - self.pw[:, d][:, None] * f(-1)


@dataclass
class SpdGaussianMol(GaussianMol):
    """``GaussianMol`` of a molecule whose shells may have l = 2 (``shells``: per atom a list of this module's
    ``Shell``)."""

    def with_coords(self, coords, need_grad: bool = True) -> "SpdGaussianMol":
        """The same molecule (basis, charges, electrons, field) at new nuclear positions (Bohr)."""
        from .field import keep_field
        return keep_field(self, spd_gaussian_mol(coords, self.charges, self.shells, need_grad, self.nelec,
                                                 self.renormalize))

    def dipole_integrals(self, origin=(0.0, 0.0, 0.0)) -> np.ndarray:
        """AO dipole integrals ``<mu| r - origin |nu>`` (3,N,N)."""
        return dipole_integrals(self.coords, self.shells, origin, self.renormalize)

    def dipole_grad_integrals(self, origin=(0.0, 0.0, 0.0)) -> np.ndarray:
        """``<d_x mu| r_c - origin_c |nu>`` (3,3,N,N), the convention of ``GaussianMol.dipole_grad_integrals``."""
        return dipole_grad_integrals(self.coords, self.shells, origin, self.renormalize)


def dipole_integrals(coords, shells, origin=(0.0, 0.0, 0.0), renormalize: bool = True) -> np.ndarray:
    """``<mu| r - origin |nu>`` (3,N,N): x - O = (x - A) + (A - O), one more power on the first function."""
    pr = _Primitives(coords, shells, renormalize)
    E = pr.pair_E(3, 2)
    root = np.sqrt(np.pi / pr.p)
    s1 = [pr.pick(E, d, 0, 0)[0] * root for d in range(3)]
    dip = np.zeros((3, pr.nao, pr.nao))
    for d in range(3):
        x1 = pr.pick(E, d, 1, 0)[0] * root + (pr.ctr[:, None, d] - float(origin[d])) * s1[d]
        dip[d] = pr.contract2(x1 * s1[(d + 1) % 3] * s1[(d + 2) % 3])
    return 0.5 * (dip + dip.transpose(0, 2, 1))


def dipole_grad_integrals(coords, shells, origin=(0.0, 0.0, 0.0), renormalize: bool = True) -> np.ndarray:
    """``ipdip[x,c,mu,nu] = <d_x mu| r_c - origin_c |nu>`` (3,3,N,N): the electron-coordinate gradient on the bra, first
    index up to l + 2 = 4 (``gto_small.dipole_grad_from_primitives`` on this module's primitive functions)."""
    pr = _Primitives(coords, shells, renormalize)
    return gto_small.dipole_grad_from_primitives(pr, pr.pair_E(4, 2), origin)


def spd_gaussian_mol(coords, charges, shells, need_grad: bool = True, nelec: Optional[Tuple[int, int]] = None,
                     renormalize: bool = True) -> SpdGaussianMol:
    """AO arrays of a molecule of s, p and spherical d shells (``coords`` (A,3) Bohr, ``shells`` per atom a list of
    ``Shell``)."""
    R = np.ascontiguousarray(np.asarray(coords, dtype=np.float64).reshape(-1, 3))
    A = R.shape[0]
    Z = np.asarray(charges, dtype=np.float64).reshape(-1)
    shells = [list(atom) for atom in shells]
    if len(shells) != A or Z.shape[0] != A:
        raise ValueError(f"spd_gaussian_mol: {A} centres, {len(shells)} shell lists, {Z.shape[0]} charges")
    for atom in shells:
        for sh in atom:
            if sh.l not in (0, 1, 2):
                raise ValueError(f"spd_gaussian_mol: shell with l={sh.l}")
    pr = _Primitives(R, shells, renormalize)
    n, Np, a, p, P = pr.nao, pr.nprim, pr.a, pr.p, pr.P
    # first index up to l + 1 (centre derivative), second up to l + 2 (kinetic energy)
    E = pr.pair_E(3, 4)
    root = np.sqrt(np.pi / p)

    def overlap_kinetic(shift):
        """Overlap and kinetic energy of every pair with the first function's powers shifted by ``shift``."""
        s1 = [pr.pick(E, d, shift[d], 0)[0] * root for d in range(3)]
        b, lb = a[None, :], pr.pw[None, :, :]
        # -1/2 d^2/dx^2 on the second function: 4 b^2 (j+2) - 2 b (2j+1) (j) + j (j-1) (j-2)
        t1 = [-0.5 * (4.0 * b * b * pr.pick(E, d, shift[d], 2)[0] * root - 2.0 * b * (2 * lb[:, :, d] + 1) * s1[d]
                      + lb[:, :, d] * (lb[:, :, d] - 1) * pr.pick(E, d, shift[d], -2)[0] * root)
              for d in range(3)]
        return s1[0] * s1[1] * s1[2], t1[0] * s1[1] * s1[2] + s1[0] * t1[1] * s1[2] + s1[0] * s1[1] * t1[2]

    def unit(d, k):
        return tuple(k * int(x == d) for x in range(3))

    def attraction(eb, L):
        """(value, operator derivatives (A,3)) of sum_C -Z_C/|r - C| for bra Hermite coefficients ``eb`` (per
        dimension, t first) of total order <= L."""
        V = np.zeros((Np, Np))
        dop = np.zeros((A, 3, Np, Np))
        for c in range(A):
            PC = P - R[c][None, None, :]
            Rt = hermite_R(L + 1, p, PC[..., 0], PC[..., 1], PC[..., 2])
            pref = -Z[c] * 2.0 * np.pi / p
            for t in range(eb[0].shape[0]):
                for u in range(min(eb[1].shape[0], L + 1 - t)):
                    for v in range(min(eb[2].shape[0], L + 1 - t - u)):
                        w = pref * eb[0][t] * eb[1][u] * eb[2][v]
                        V += w * Rt[(t, u, v)]
                        # d/dC of R_tuv(P - C) = -R_{t+1,u,v}
                        dop[c, 0] -= w * Rt[(t + 1, u, v)]
                        dop[c, 1] -= w * Rt[(t, u + 1, v)]
                        dop[c, 2] -= w * Rt[(t, u, v + 1)]
        return V, dop

    base = [pr.pick(E, d, 0, 0)[:5] for d in range(3)]                 # t <= 4
    Sp, Tp = overlap_kinetic((0, 0, 0))
    Vp, dVop = attraction(base, 4)
    S = pr.contract2(Sp)
    hcore = pr.contract2(Tp + Vp)
    S = 0.5 * (S + S.T)
    hcore = 0.5 * (hcore + hcore.T)

    # ---- nuclear repulsion
    enuc = 0.0
    gnuc = np.zeros((A, 3))
    for i in range(A):
        for j in range(A):
            if i == j:
                continue
            d = R[i] - R[j]
            r = np.linalg.norm(d)
            if j > i:
                enuc += Z[i] * Z[j] / r
            gnuc[i] -= Z[i] * Z[j] * d / r ** 3

    def bra_derivative(d, rows=None):
        """Hermite coefficients (t <= 5) of d/dA_d of the bra pair, dimension d."""
        up, dn = pr.pick(E, d, 1, 0, rows)[:6], pr.pick(E, d, -1, 0, rows)[:6]
        ar = a[:, None] if rows is None else a[rows][:, None]
        lr = pr.pw[:, d][:, None] if rows is None else pr.pw[rows, d][:, None]
        return 2.0 * ar * up - lr * dn

    if need_grad:
        ipovlp = np.zeros((3, n, n))
        dH1 = np.zeros((3, n, n))
        for d in range(3):
            st = lambda k: overlap_kinetic(unit(d, k))
            dS = pr.center_derivative(lambda k: st(k)[0], d)
            dT = pr.center_derivative(lambda k: st(k)[1], d)
            eb = list(base)
            eb[d] = bra_derivative(d)
            ipovlp[d] = -pr.contract2(dS)                    # <grad mu | nu>: electron gradient = - centre gradient
            dH1[d] = pr.contract2(dT + attraction(eb, 5)[0])     # d/d(centre of mu) of hcore_{mu nu}, nuclei fixed
        dop = pr.contract2(dVop)                             # (A,3,n,n) operator part
        dhcore = dop.copy()
        for at, (s0, s1) in enumerate(pr.aoslices):
            # the functions of atom `at` move with it: their rows and, by symmetry, their columns
            dhcore[at, :, s0:s1, :] += dH1[:, s0:s1, :]
            dhcore[at, :, :, s0:s1] += dH1[:, s0:s1, :].transpose(0, 2, 1)
            # both functions on the atom: row, column and the atom's own operator term cancel but for the other nuclei
            # (translational invariance), d/dR_at = - sum_{C != at} d/dC
            dhcore[at, :, s0:s1, s0:s1] = -(dop.sum(axis=0) - dop[at])[:, s0:s1, s0:s1]
    else:
        ipovlp = np.zeros((3, n, n))
        dhcore = np.zeros((A, 3, n, n))

    # ---- two-electron integrals, one first primitive function at a time
    q = p.reshape(-1)
    Q = P.reshape(-1, 3)
    sign = np.array([1.0, -1.0, 1.0, -1.0, 1.0])
    ket = [e.reshape(5, -1) * sign[:, None] for e in base]                            # (-1)^tau E_tau
    eri = np.zeros((n, n, n, n))
    eri_ip1 = np.zeros((3, n, n, n, n)) if need_grad else np.zeros((3, 0))
    L2 = 9 if need_grad else 8

    def convolve(eb, ek):                                     # (tb, Np) x (5, Np^2) -> (tb + 4, Np, Np^2)
        out = np.zeros((eb.shape[0] + ek.shape[0] - 1, eb.shape[1], ek.shape[1]))
        for t in range(eb.shape[0]):
            for tau in range(ek.shape[0]):
                out[t + tau] += eb[t][:, None] * ek[tau][None, :]
        return out

    def fold(X, m):                                           # (Np, Np^2) of first primitive m -> (n, n, n)
        Y = (pr.Cm.T @ X).reshape(n, Np, Np)
        return pr.cn[m] * np.einsum("jrs,rk,sl->jkl", Y, pr.Cm, pr.Cm, optimize=True)

    for m in range(Np):
        pm = p[m][:, None]
        PQ = P[m][:, None, :] - Q[None, :, :]
        Rt = hermite_R(L2, pm * q[None, :] / (pm + q[None, :]), PQ[..., 0], PQ[..., 1], PQ[..., 2])
        pref = 2.0 * np.pi ** 2.5 / (pm * q[None, :] * np.sqrt(pm + q[None, :]))
        cb = [convolve(base[d][:, m], ket[d]) for d in range(3)]

        def hermite_sum(c):
            out = 0.0
            for t in range(c[0].shape[0]):
                for u in range(c[1].shape[0]):
                    ctu = c[0][t] * c[1][u]
                    for v in range(c[2].shape[0]):
                        if (t, u, v) in Rt:
                            out = out + ctu * c[2][v] * Rt[(t, u, v)]
            return pref * out

        eri[pr.ao[m]] += fold(hermite_sum(cb), m)
        if need_grad:
            for d in range(3):
                c = list(cb)
                c[d] = convolve(bra_derivative(d, [m])[:, 0], ket[d])
                eri_ip1[d, pr.ao[m]] -= fold(hermite_sum(c), m)      # electron gradient = - centre gradient

    ne = int(round(float(np.sum(Z))))
    if nelec is None:
        nelec = ((ne + 1) // 2, ne // 2)
    return SpdGaussianMol(S=S, hcore=hcore, eri=eri, ipovlp=ipovlp, dhcore=dhcore, eri_ip1=eri_ip1,
                          aoslices=pr.aoslices, enuc=float(enuc), gnuc=gnuc, integral_symmetry=True, coords=R,
                          nelec=tuple(nelec), charges=Z, shells=shells, renormalize=bool(renormalize))


def molecule(symbols: Sequence[str], coords, basis="sto-3g", need_grad: bool = True, charge: int = 0) -> SpdGaussianMol:
    """A molecule of H and O atoms (``coords`` Bohr) in a tabulated basis ("sto-3g", "6-31g", "cc-pvdz" or a table)."""
    table = BASES[basis.lower()] if isinstance(basis, str) else basis
    Z = [_ELEMENTS[s][0] for s in symbols]
    ne = int(round(sum(Z))) - int(charge)
    return spd_gaussian_mol(coords, Z, [element_shells(table, s) for s in symbols], need_grad,
                            ((ne + 1) // 2, ne // 2))


def water_coords(r_oh: float = 0.9572 * ANGSTROM, angle: float = 104.52) -> np.ndarray:
    """H2O in the xy plane, O at the origin; atoms O, H, H (the geometry of ``gto_small.water``)."""
    h = np.radians(angle) / 2.0
    return np.array([[0.0, 0.0, 0.0], [r_oh * np.sin(h), r_oh * np.cos(h), 0.0], [-r_oh * np.sin(h), r_oh * np.cos(h), 0.0]])


def water(basis="sto-3g", r_oh: float = 0.9572 * ANGSTROM, angle: float = 104.52, need_grad: bool = True) -> SpdGaussianMol:
    """H2O in the xy plane, O at the origin, ``r_oh`` in Bohr and ``angle`` (HOH) in degrees; atoms O, H, H."""
    return molecule(("O", "H", "H"), water_coords(r_oh, angle), basis, need_grad)


def water_shells(basis="cc-pvdz"):
    """(charges, shells per atom) of water, atoms O, H, H, without any integral: what the device object needs."""
    table = BASES[basis.lower()] if isinstance(basis, str) else basis
    return [_ELEMENTS[s][0] for s in "OHH"], [element_shells(table, s) for s in "OHH"]
