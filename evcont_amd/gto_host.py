"""The host statement of the AO integrals (and their first nuclear derivatives) of molecules built from contracted
Gaussian shells, with nothing third-party: s and p as Cartesian functions, d and f as the five and seven REAL SPHERICAL
functions.  ``evcont_amd.gto_small`` (s and p: water, the H2O-H3O+ dimer and Zundel in STO-3G or 6-31G),
``evcont_amd.gto_spd`` (s, p and d: water in cc-pVDZ) and ``evcont_amd.gto_spdf`` (up to f) are its entry points; each
calls ``gaussian_arrays`` with a fixed ``lmax`` of its own (1, 2 and 3), which sets the Hermite orders and with them the
rounding and the run time.  The
arrays, their meanings and their signs are those of ``evcont_amd.hchain`` (which remains the statement, and the fast
route, for one s function per centre):

    S, hcore, eri, ipovlp, dhcore, eri_ip1, enuc, gnuc

``dhcore`` has ``hcore_generator`` semantics: the operator term of nucleus A plus the rows and columns of ALL functions
in ``aoslices[A]``.  AO order: atoms, then the atom's shells in the given order, p as x, y, z, d as m = -2 ... 2
(PySCF's order):

    xy, yz, 2z^2 - x^2 - y^2, xz, x^2 - y^2

Each d function is a fixed linear combination (``D_MONOMIALS``) of the Cartesian monomials of ONE primitive set; the
Cartesian s-type combination x^2 + y^2 + z^2 never appears.

Method: McMurchie-Davidson.  A product of two primitive functions (``_Primitives``: exponent, weight, centre and power
triple) is expanded in Hermite Gaussians about P with the coefficients ``E_t^{ij}`` of each dimension (``hermite_E``); a
Coulomb integral is then a sum over Hermite Coulomb integrals ``R_tuv`` (``hermite_R``), which come from the Boys
functions (``boys``).  The derivative of a primitive with respect to its centre is ``2a (l+1) - l (l-1)`` in the power
of that dimension, so the first index goes up to lmax + 1; the kinetic energy raises the second to lmax + 2.  Hermite
total 4 lmax + 1 in ``eri_ip1`` (4 lmax in ``eri``): Boys functions F0 ... F5 for s and p, F0 ... F9 with d.

This is numpy, clarity over speed (water / cc-pVDZ takes minutes); ``evcont_amd.gto_device`` and
``evcont_amd.gto_spd_device`` compute the same arrays on the device from the coordinates (``csrc/spgto.hip``,
``csrc/spdgto.hip``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
from scipy.special import erf

# Below the crossover F_nmax comes from its convergent series and the lower orders by downward recursion; above it F0
# comes from erf and the higher orders by upward recursion (stable there: exp(-t) is small against (2n+1) F_n).
BOYS_CROSSOVER = 12.0
BOYS_SERIES_TERMS = 64


@dataclass(frozen=True)
class Shell:
    """A contracted shell: ``l`` 0 (s), 1 (p: x, y, z) or 2 (d: the five real spherical functions), exponents and the
    contraction coefficients of NORMALISED primitives, as published tables give them."""
    l: int
    exponents: Tuple[float, ...]
    coefficients: Tuple[float, ...]
    _LS = (0, 1, 2)                       # the accepted l (``gto_spdf.Shell`` accepts 3 as well)

    def __post_init__(self):
        object.__setattr__(self, "l", int(self.l))
        object.__setattr__(self, "exponents", tuple(float(x) for x in self.exponents))
        object.__setattr__(self, "coefficients", tuple(float(x) for x in self.coefficients))
        if self.l not in self._LS:
            raise ValueError(f"Shell: l={self.l}, supported {', '.join(map(str, self._LS[:-1]))} and {self._LS[-1]}")
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
# Per component of an f shell (m = -3 ... 3, PySCF's order), for primitives normalised as x y z exp(-a r^2)
# (``primitive_norm(3, a)``); used by the entry point ``evcont_amd.gto_spdf`` alone.
_R24, _R40, _R60 = 1.0 / np.sqrt(24.0), 1.0 / np.sqrt(40.0), 1.0 / np.sqrt(60.0)
F_MONOMIALS = (
    (((2, 1, 0), 3.0 * _R24), ((0, 3, 0), -_R24)),                              # y (3 x^2 - y^2)
    (((1, 1, 1), 1.0),),                                                        # x y z
    (((0, 1, 2), 4.0 * _R40), ((2, 1, 0), -_R40), ((0, 3, 0), -_R40)),          # y (4 z^2 - x^2 - y^2)
    (((0, 0, 3), 2.0 * _R60), ((2, 0, 1), -3.0 * _R60), ((0, 2, 1), -3.0 * _R60)),   # z (2 z^2 - 3 x^2 - 3 y^2)
    (((1, 0, 2), 4.0 * _R40), ((3, 0, 0), -_R40), ((1, 2, 0), -_R40)),          # x (4 z^2 - x^2 - y^2)
    (((2, 0, 1), 0.5), ((0, 2, 1), -0.5)),                                      # z (x^2 - y^2)
    (((3, 0, 0), _R24), ((1, 2, 0), -3.0 * _R24)),                              # x (x^2 - 3 y^2)
)


def monomials(l: int, comp: int):
    """((powers), weight) of the monomials of component ``comp`` of a shell of angular momentum ``l``."""
    if l == 0:
        return (((0, 0, 0), 1.0),)
    if l == 1:
        return ((tuple(int(comp == d) for d in range(3)), 1.0),)
    return F_MONOMIALS[comp] if l == 3 else D_MONOMIALS[comp]


def element_shells(table, symbol: str):
    """The shells of one atom from a basis table, whose entries are (l, exponents, coefficients) or (exponents,
    s coefficients, p coefficients or None): an s set and behind it the p set on the same exponents (an SP shell)."""
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
    """Norm of a Cartesian primitive: exp(-a r^2), x exp(-a r^2), x y exp(-a r^2) or x y z exp(-a r^2) for
    l = 0, 1, 2, 3."""
    a = np.asarray(a, dtype=np.float64)
    if l == 3:
        return (2.0 * a / np.pi) ** 0.75 * (8.0 * a * np.sqrt(a))
    return (2.0 * a / np.pi) ** 0.75 * (1.0, 2.0 * np.sqrt(a), 4.0 * a)[l]


def shell_self_overlap(shell) -> float:
    """<f|f> of one contracted function of the shell with the tabulated coefficients (the same for every component)."""
    a = np.asarray(shell.exponents)
    c = np.asarray(shell.coefficients) * primitive_norm(shell.l, a)
    p = a[:, None] + a[None, :]
    s = (np.pi / p) ** 1.5 * (1.0, 0.5 / p, 0.25 / (p * p), 0.125 / (p * p * p))[shell.l]
    return float(c @ s @ c)


def contraction_coefficients(shells, renormalize: bool = True):
    """Per atom and shell the coefficients of normalised primitives the integrals use: the tabulated ones, scaled to
    unit self-overlap of the contracted function with ``renormalize`` (what PySCF does on input)."""
    return [[tuple(np.asarray(sh.coefficients) / (np.sqrt(shell_self_overlap(sh)) if renormalize else 1.0))
             for sh in atom] for atom in shells]


def flatten_shells(shells, coef):
    """The basis as the device calls take it, from per-atom shell lists and their ``contraction_coefficients``:
    (shell_atom, shell_l, shell_prim_offset, exponents, coefficients, aoslices (A,2), nao)."""
    atom, l, off, ex, co, slices, n = [], [], [0], [], [], [], 0
    for at, (shs, cs) in enumerate(zip(shells, coef)):
        start = n
        for sh, c in zip(shs, cs):
            atom.append(at)
            l.append(sh.l)
            off.append(off[-1] + len(sh.exponents))
            ex += list(sh.exponents)
            co += list(c)
            n += 2 * sh.l + 1
        slices.append((start, n))
    return (np.array(atom, dtype=np.int32), np.array(l, dtype=np.int32), np.array(off, dtype=np.int32),
            np.array(ex, dtype=np.float64), np.array(co, dtype=np.float64),
            np.array(slices, dtype=np.int64).reshape(-1, 2), n)


def boys(nmax: int, t) -> np.ndarray:
    """F_0 ... F_nmax of ``t`` (>= 0), shape (nmax+1,) + t.shape."""
    t = np.asarray(t, dtype=np.float64)
    small = t < BOYS_CROSSOVER
    out = np.empty((nmax + 1,) + t.shape)
    # series F_n(t) = exp(-t) sum_k (2t)^k / ((2n+1)(2n+3)...(2n+2k+1)), all terms positive
    ts = np.where(small, t, 0.0)
    term = np.full(t.shape, 1.0 / (2 * nmax + 1))
    s = term.copy()
    for k in range(1, BOYS_SERIES_TERMS):
        term = term * (2.0 * ts) / (2 * nmax + 2 * k + 1)
        s = s + term
    et = np.exp(-ts)
    fs = [None] * (nmax + 1)
    fs[nmax] = et * s
    for n in range(nmax, 0, -1):
        fs[n - 1] = (2.0 * ts * fs[n] + et) / (2 * n - 1)
    tl = np.where(small, BOYS_CROSSOVER, t)
    rt = np.sqrt(tl)
    fl = [0.5 * np.sqrt(np.pi) / rt * erf(rt)]
    el = np.exp(-tl)
    for n in range(nmax):
        fl.append(((2 * n + 1) * fl[n] - el) / (2.0 * tl))
    for n in range(nmax + 1):
        out[n] = np.where(small, fs[n], fl[n])
    return out


def hermite_E(imax: int, jmax: int, a, b, AB):
    """One dimension: ``E[i][j][t]`` with x_A^i x_B^j exp(-a x_A^2 - b x_B^2) = sum_t E_t^{ij} Lambda_t(p, x_P), for
    0 <= i <= imax, 0 <= j <= jmax, as an array (imax+1, jmax+1, imax+jmax+1) + shape; ``AB`` = A - B.  P - A and P - B
    are formed from A - B, so they vanish exactly on one centre."""
    p = a + b
    mu = a * b / p
    xpa, xpb = -(b / p) * AB, (a / p) * AB
    shape = np.broadcast(a, b, AB).shape
    E = np.zeros((imax + 1, jmax + 1, imax + jmax + 3) + shape)
    E[0, 0, 0] = np.exp(-mu * AB * AB)
    for i in range(imax + 1):
        for j in range(jmax + 1):
            if i == j == 0:
                continue
            src, x = (E[i - 1, j], xpa) if j == 0 else (E[i, j - 1], xpb)
            for t in range(i + j + 1):
                E[i, j, t] = (src[t - 1] / (2.0 * p) if t > 0 else 0.0) + x * src[t] + (t + 1) * src[t + 1]
    return E[:, :, : imax + jmax + 1]


def hermite_R(L: int, alpha, X, Y, Z):
    """Hermite Coulomb integrals ``R_tuv`` = d^t_X d^u_Y d^v_Z F0(alpha R^2) for t + u + v <= L, as a dict.  The
    auxiliary ``R_tuv^n`` of total order k = t + u + v (n <= L - k) come from those of the orders k - 1 and k - 2 alone,
    so they are made order by order and an order is dropped once the next two are done, instead of keeping all 2 380
    auxiliaries of L = 13 to the end (the arithmetic of an entry is the same either way)."""
    F = boys(L, alpha * (X * X + Y * Y + Z * Z))
    below, last = {}, {(0, 0, 0, n): (-2.0 * alpha) ** n * F[n] for n in range(L + 1)}
    out = {(0, 0, 0): last[(0, 0, 0, 0)]}
    for k in range(1, L + 1):
        level = {}
        for t in range(k, -1, -1):
            for u in range(k - t, -1, -1):
                v = k - t - u
                for n in range(L - k + 1):
                    if t > 0:
                        r = X * last[(t - 1, u, v, n + 1)]
                        r = r + (t - 1) * below[(t - 2, u, v, n + 1)] if t > 1 else r
                    elif u > 0:
                        r = Y * last[(t, u - 1, v, n + 1)]
                        r = r + (u - 1) * below[(t, u - 2, v, n + 1)] if u > 1 else r
                    else:
                        r = Z * last[(t, u, v - 1, n + 1)]
                        r = r + (v - 1) * below[(t, u, v - 2, n + 1)] if v > 1 else r
                    level[(t, u, v, n)] = r
                out[(t, u, v)] = level[(t, u, v, 0)]
        below, last = last, level
    return out


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
        self.lmax = max((sh.l for atom in shells for sh in atom), default=0)
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


def dipole_integrals(coords, shells, origin=(0.0, 0.0, 0.0), renormalize: bool = True) -> np.ndarray:
    """AO dipole integrals ``<mu| r - origin |nu>`` (3,N,N) (PySCF: ``int1e_r`` under ``with_common_orig``):
    x - O = (x - A) + (A - O), one more power on the first function.  An ``E_t^{ij}`` does not depend on the orders it
    is tabulated to, so the orders follow the shells here."""
    pr = _Primitives(coords, shells, renormalize)
    E = pr.pair_E(pr.lmax + 1, pr.lmax)
    root = np.sqrt(np.pi / pr.p)
    s1 = [pr.pick(E, d, 0, 0)[0] * root for d in range(3)]
    dip = np.zeros((3, pr.nao, pr.nao))
    for d in range(3):
        x1 = pr.pick(E, d, 1, 0)[0] * root + (pr.ctr[:, None, d] - float(origin[d])) * s1[d]
        dip[d] = pr.contract2(x1 * s1[(d + 1) % 3] * s1[(d + 2) % 3])
    return 0.5 * (dip + dip.transpose(0, 2, 1))


def dipole_grad_integrals(coords, shells, origin=(0.0, 0.0, 0.0), renormalize: bool = True) -> np.ndarray:
    """``ipdip[x,c,mu,nu] = <d_x mu| r_c - origin_c |nu>`` (3,3,N,N): the electron-coordinate gradient on the bra (the
    convention of ``ipovlp``), so ``d dip_c[mu,nu] / dR_Ax = -ipdip[x,c,mu,nu] [mu in A] - ipdip[x,c,nu,mu]
    [nu in A]``.  First index up to l + 2."""
    pr = _Primitives(coords, shells, renormalize)
    return dipole_grad_from_primitives(pr, pr.pair_E(pr.lmax + 2, pr.lmax), origin)


def dipole_grad_from_primitives(pr, E, origin) -> np.ndarray:
    """``<d_x mu| r_c - O_c |nu>`` (3,3,N,N) from the primitive functions ``pr`` and their ``pair_E(l + 2, l)``: the
    bra derivative ``2a E^{i+1,j} - i E^{i-1,j}`` in dimension x of the dipole factor ``(x - O) = (x - A) + (A - O)``,
    one more power on the first function, in dimension c."""
    O = np.asarray(origin, dtype=np.float64).reshape(3)
    root = np.sqrt(np.pi / pr.p)
    # one dimension of the overlap / of the dipole integral with the first function's power shifted by k
    s = lambda d, k: pr.pick(E, d, k, 0)[0] * root
    r = lambda d, k: pr.pick(E, d, k + 1, 0)[0] * root + (pr.ctr[:, None, d] - O[d]) * s(d, k)
    out = np.zeros((3, 3, pr.nao, pr.nao))
    for x in range(3):
        for c in range(3):
            def f(k):
                val = 1.0
                for d in range(3):
                    kd = k if d == x else 0
                    val = val * (r(d, kd) if d == c else s(d, kd))
                return val
            out[x, c] = -pr.contract2(pr.center_derivative(f, x))    # electron gradient = - centre gradient
    return out


def gaussian_arrays(entry: str, lmax: int, coords, charges, shells, need_grad: bool = True,
                    nelec: Optional[Tuple[int, int]] = None, renormalize: bool = True) -> dict:
    """The AO arrays of a molecule of shells with l <= ``lmax`` (``coords`` (A,3) Bohr, ``shells`` per atom a list of
    ``Shell``) as the fields of a ``gto_small.GaussianMol``.  ``lmax`` fixes the Hermite orders and belongs to the entry
    point ``entry`` (the name its errors carry), not to the molecule."""
    R = np.ascontiguousarray(np.asarray(coords, dtype=np.float64).reshape(-1, 3))
    A = R.shape[0]
    Z = np.asarray(charges, dtype=np.float64).reshape(-1)
    shells = [list(atom) for atom in shells]
    if len(shells) != A or Z.shape[0] != A:
        raise ValueError(f"{entry}: {A} centres, {len(shells)} shell lists, {Z.shape[0]} charges")
    for atom in shells:
        for sh in atom:
            if not 0 <= sh.l <= lmax:
                raise ValueError(f"{entry}: shell with l={sh.l}")
    pr = _Primitives(R, shells, renormalize)
    n, Np, a, p, P = pr.nao, pr.nprim, pr.a, pr.p, pr.P
    # first index up to l + 1 (centre derivative), second up to l + 2 (kinetic energy)
    E = pr.pair_E(lmax + 1, lmax + 2)
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

    base = [pr.pick(E, d, 0, 0)[:2 * lmax + 1] for d in range(3)]      # t <= 2 lmax
    Sp, Tp = overlap_kinetic((0, 0, 0))
    Vp, dVop = attraction(base, 2 * lmax)
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
        """Hermite coefficients (t <= 2 lmax + 1) of d/dA_d of the bra pair, dimension d."""
        up, dn = pr.pick(E, d, 1, 0, rows)[:2 * lmax + 2], pr.pick(E, d, -1, 0, rows)[:2 * lmax + 2]
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
            # d/d(centre of mu) of hcore_{mu nu}, nuclei fixed
            dH1[d] = pr.contract2(dT + attraction(eb, 2 * lmax + 1)[0])
        dop = pr.contract2(dVop)                             # (A,3,n,n) operator part
        dhcore = dop.copy()
        for at, (s0, s1) in enumerate(pr.aoslices):
            # the functions of atom `at` move with it: their rows and, by symmetry, their columns
            dhcore[at, :, s0:s1, :] += dH1[:, s0:s1, :]
            dhcore[at, :, :, s0:s1] += dH1[:, s0:s1, :].transpose(0, 2, 1)
            # both functions on the atom: row, column and the atom's own operator term cancel but for the other nuclei
            # (translational invariance), d/dR_at = - sum_{C != at} d/dC; summing the large cancelling terms instead
            # costs digits with tight functions
            dhcore[at, :, s0:s1, s0:s1] = -(dop.sum(axis=0) - dop[at])[:, s0:s1, s0:s1]
    else:
        ipovlp = np.zeros((3, n, n))
        dhcore = np.zeros((A, 3, n, n))

    # ---- two-electron integrals, one first primitive function at a time
    q = p.reshape(-1)
    Q = P.reshape(-1, 3)
    sign = (-1.0) ** np.arange(2 * lmax + 1)
    ket = [e.reshape(2 * lmax + 1, -1) * sign[:, None] for e in base]                 # (-1)^tau E_tau
    eri = np.zeros((n, n, n, n))
    eri_ip1 = np.zeros((3, n, n, n, n)) if need_grad else np.zeros((3, 0))
    L2 = 4 * lmax + (1 if need_grad else 0)

    def convolve(eb, ek):                                     # (tb, Np) x (tk, Np^2) -> (tb + tk - 1, Np, Np^2)
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
    return dict(S=S, hcore=hcore, eri=eri, ipovlp=ipovlp, dhcore=dhcore, eri_ip1=eri_ip1, aoslices=pr.aoslices,
                enuc=float(enuc), gnuc=gnuc, integral_symmetry=True, coords=R, nelec=tuple(nelec), charges=Z,
                shells=shells, renormalize=bool(renormalize))
