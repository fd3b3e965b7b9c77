"""A small determinant full-CI solver with the two calls the FCI training-state container makes
on a PySCF ``cisolver`` (``FCI_EVCont.py:72-74,118-121``):

    e, ci = solver.kernel(h1, h2, norb, nelec, nroots=k)
    dm1, dm2 = solver.trans_rdm12(cibra, ciket, norb, nelec)

so that hydrogen-chain training data (BASELINE configs 0-1) can be generated without PySCF
(SURVEY.md §8f-2).  Conventions follow ``pyscf.fci.direct_spin1``: CI vectors are ``(na, nb)`` arrays
over alpha/beta occupation strings ordered by their integer value; ``dm1[p,q] = <q^+ p>`` and
``dm2[p,q,r,s] = <p^+ r^+ s q>`` (chemists' order, spin summed), so that
``E = h1:dm1 + 1/2 h2:dm2`` with ``h2`` in chemists' notation.

``spin_square_vector(c, norb, nelec)`` is ``S^2 c``; ``SmallFCI(spin_penalty=shift)`` adds ``shift (S^2 - S(S+1))`` to the
operator the eigensolver sees, so that the lowest roots have the chosen multiplicity (PySCF's ``fix_spin_``).

``transform_ci(ci, nelec, u)`` rotates a CI vector under an orbital transformation (PySCF's ``fci.addons.transform_ci``),
so that a state solved in the canonical basis can be stored in the OAO basis.

Host code for up to ~12 orbitals (training-state generation is outside the accelerated hot path).
"""
from __future__ import annotations

from itertools import combinations
import warnings
from functools import lru_cache
from typing import List, Optional, Tuple

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import LinearOperator, eigsh


def _strings(norb: int, nocc: int) -> List[int]:
    return sorted(sum(1 << i for i in occ) for occ in combinations(range(norb), nocc))


def _excitation_ops(norb: int, nocc: int):
    """E[p][q] = a_p^+ a_q on the occupation strings, as CSR matrices (rows = resulting string)."""
    strs = _strings(norb, nocc)
    index = {s: i for i, s in enumerate(strs)}
    ns = len(strs)
    ops = [[None] * norb for _ in range(norb)]
    for p in range(norb):
        for q in range(norb):
            rows, cols, vals = [], [], []
            for j, s in enumerate(strs):
                if not (s >> q) & 1:
                    continue
                if p == q:
                    rows.append(j); cols.append(j); vals.append(1.0)
                    continue
                if (s >> p) & 1:
                    continue
                t = (s ^ (1 << q)) | (1 << p)
                lo, hi = (p, q) if p < q else (q, p)
                between = bin(s & (((1 << hi) - 1) ^ ((1 << (lo + 1)) - 1))).count("1")
                rows.append(index[t]); cols.append(j); vals.append(-1.0 if between & 1 else 1.0)
            ops[p][q] = sp.csr_matrix((vals, (rows, cols)), shape=(ns, ns))
    return ops, ns


def _nelec_pair(nelec) -> Tuple[int, int]:
    if isinstance(nelec, (int, np.integer)):
        return (int(nelec) + 1) // 2, int(nelec) // 2
    return int(nelec[0]), int(nelec[1])


def minor_matrix(u, norb: int, nocc: int) -> np.ndarray:
    """``T[I, J] = det(u[occ(I)][:, occ(J)])`` over the strings of ``nocc`` electrons in ``norb`` orbitals, ordered by
    integer value; ``occ(I)`` ascending.  ``[[1]]`` for ``nocc == 0``."""
    u = np.asarray(u, dtype=np.float64)
    if u.shape != (norb, norb):
        raise ValueError(f"transform_ci: u of shape {u.shape} for {norb} orbitals (square u only)")
    occ = [[p for p in range(norb) if (s >> p) & 1] for s in _strings(norb, nocc)]
    if nocc == 0:
        return np.ones((1, 1))
    occ = np.array(occ)
    ns = len(occ)
    T = np.empty((ns, ns))
    rows = max(1, (1 << 21) // (ns * nocc * nocc))          # row blocks of about 16 MB of (rows, ns, k, k) submatrices
    for i0 in range(0, ns, rows):
        T[i0:i0 + rows] = np.linalg.det(u[occ[i0:i0 + rows, None, :, None], occ[None, :, None, :]])
    return T


def transform_ci(ci, nelec, u) -> np.ndarray:
    """The CI vector in the orbitals ``new_q = sum_p old_p u[p, q]`` (``pyscf.fci.addons.transform_ci`` for a square
    ``u``, or a pair ``(u_a, u_b)``): ``T_a^T c T_b`` with the matrices of minors above.  Nothing assumes ``u``
    orthogonal."""
    na_el, nb_el = _nelec_pair(nelec)
    if isinstance(u, (tuple, list)):
        ua, ub = (np.asarray(x, dtype=np.float64) for x in u)
    else:
        ua = ub = np.asarray(u, dtype=np.float64)
    norb = ua.shape[0]
    Ta = minor_matrix(ua, norb, na_el)
    Tb = Ta if (ub is ua and nb_el == na_el) else minor_matrix(ub, norb, nb_el)
    c = np.asarray(ci, dtype=np.float64).reshape(Ta.shape[0], Tb.shape[0])
    return Ta.T @ c @ Tb


@lru_cache(maxsize=8)
def _spin_ops(norb: int, nelec: Tuple[int, int]):
    ea, na = _excitation_ops(norb, nelec[0])
    eb, nb = (ea, na) if nelec[1] == nelec[0] else _excitation_ops(norb, nelec[1])
    return ea, [[eb[p][q].T.tocsr() for q in range(norb)] for p in range(norb)], na, nb


def spin_constant(nelec) -> float:
    """``Sz (Sz + 1) + n_beta``: what ``S^2 = Sz (Sz + 1) + n_beta - sum_pq E^alpha_pq E^beta_qp`` has on its diagonal
    before the pair term."""
    na_el, nb_el = _nelec_pair(nelec)
    sz = 0.5 * (na_el - nb_el)
    return sz * (sz + 1.0) + nb_el


def spin_square_vector(c, norb: int, nelec, _ops=None) -> np.ndarray:
    """``S^2 c``, ``(na, nb)``: ``k c - sum_pq ea[p][q] @ c @ eb[q][p].T`` with the CSR operators of
    ``_excitation_ops`` and ``k = Sz (Sz + 1) + n_beta``."""
    nelec = _nelec_pair(nelec)
    ea, ebT, na, nb = _ops if _ops is not None else _spin_ops(norb, nelec)
    c = np.asarray(c, dtype=np.float64).reshape(na, nb)
    out = spin_constant(nelec) * c
    for p in range(norb):
        for q in range(norb):
            if ea[p][q].nnz and ebT[q][p].nnz:
                out -= (ea[p][q] @ c) @ ebT[q][p]
    return out


def spin_targets(nelec) -> List[float]:
    """The values ``S (S + 1)`` that ``nelec`` allows: ``S = |Sz|, |Sz| + 1, ... <= (n_alpha + n_beta) / 2``."""
    na_el, nb_el = _nelec_pair(nelec)
    s, top, out = 0.5 * abs(na_el - nb_el), 0.5 * (na_el + nb_el), []
    while s <= top:
        out.append(s * (s + 1.0))
        s += 1.0
    return out


def resolve_spin_target(spin_target: Optional[float], nelec) -> float:
    """``spin_target`` as a float, ``None`` meaning ``Sz (Sz + 1)``; ``ValueError`` unless it is one of
    ``spin_targets(nelec)``."""
    allowed = spin_targets(nelec)
    if spin_target is None:
        return allowed[0]
    hit = [v for v in allowed if abs(v - float(spin_target)) <= 1e-12]
    if not hit:
        raise ValueError(f"spin_target={spin_target} is no S(S+1) that nelec={_nelec_pair(nelec)} allows "
                         f"(expected one of {allowed})")
    return hit[0]


def multiplicity_of(ss: float) -> float:
    """``2 S + 1`` from ``<S^2> = S (S + 1)`` (PySCF's ``spin_square`` convention)."""
    return 2.0 * (np.sqrt(ss + 0.25) - 0.5) + 1.0


SPIN_WARN = 1e-6     # a returned root whose <S^2> is further than this from the target raises a RuntimeWarning


def unshift_roots(theta, spin_squares, shift: float, target: float):
    """The energies of H from the eigenvalues ``theta`` of ``H + shift (S^2 - target)`` and the measured ``<S^2>`` of
    their (spin-pure) eigenvectors, in the solver's order; warns about every root of another multiplicity."""
    out = []
    for k, (t, ss) in enumerate(zip(theta, spin_squares)):
        out.append(float(t) - shift * (float(ss) - target))
        if abs(ss - target) > SPIN_WARN:
            warnings.warn(f"root {k} has <S^2> = {ss:.6f}, not the target {target:.6f}: another multiplicity lies inside "
                          f"the window of the {len(theta)} lowest shifted roots; use a larger spin_penalty (now {shift}) "
                          f"or fewer roots", RuntimeWarning, stacklevel=3)
    return out


def fix_spin_(solver, shift: float = 0.2, ss: Optional[float] = None):
    """PySCF's ``fci.addons.fix_spin_`` for a ``SmallFCI`` or ``DeviceFCI``: sets ``spin_penalty = shift`` and
    ``spin_target = ss`` (an ``S (S + 1)`` value, ``None`` for the lowest multiplicity) and returns the solver."""
    solver.spin_penalty = float(shift)
    solver.spin_target = ss
    return solver


class SmallFCI:
    """Spin-adapted through Ms, ``nelec = (nalpha, nbeta)``, and, with ``spin_penalty != 0``, through a penalty on S^2:
    the eigensolver then sees ``H + spin_penalty (S^2 - spin_target)`` (``contract`` returns that operator's product, as
    PySCF's ``contract_2e`` does after ``fix_spin_``), while ``kernel`` returns energies of H,
    ``theta - spin_penalty (<S^2> - spin_target)`` with ``<S^2>`` measured per root and kept in ``spin_squares``.
    ``spin_target`` is an ``S (S + 1)`` value, ``None`` meaning ``Sz (Sz + 1)``, the lowest multiplicity the electron
    numbers allow.  A target above ``|Sz|`` pushes the lower multiplicities down instead of up (their penalty is
    negative), as in PySCF: for such states choose ``nelec`` with ``Ms = S`` and leave ``spin_target`` alone.  With the
    default ``spin_penalty = 0`` nothing changes and ``spin_squares`` stays ``None``."""

    def __init__(self, tol: float = 1e-13, dense_limit: int = 1500, spin_penalty: float = 0.0,
                 spin_target: Optional[float] = None):
        self.tol = tol
        self.dense_limit = dense_limit
        self.spin_penalty = float(spin_penalty)
        self.spin_target = spin_target
        self.spin_squares = None
        self._cache = {}
        self.converged = True

    def _ops(self, norb: int, nelec: Tuple[int, int]):
        key = (norb, tuple(nelec))
        if key not in self._cache:
            ea, na = _excitation_ops(norb, nelec[0])
            eb, nb = (ea, na) if nelec[1] == nelec[0] else _excitation_ops(norb, nelec[1])
            ebT = [[eb[p][q].T.tocsr() for q in range(norb)] for p in range(norb)]
            self._cache[key] = (ea, ebT, na, nb)
        return self._cache[key]

    def _excite_all(self, c, norb, nelec):
        """D[p*norb+q] = E_pq c for all p, q; shape (norb^2, na, nb)."""
        ea, ebT, na, nb = self._ops(norb, nelec)
        c = np.asarray(c, dtype=np.float64).reshape(na, nb)
        D = np.empty((norb * norb, na, nb))
        for p in range(norb):
            for q in range(norb):
                D[p * norb + q] = ea[p][q] @ c + (ebT[p][q].T @ c.T).T
        return D

    def contract(self, h1, h2, c, norb, nelec):
        """sigma = H c with H = sum h'_pq E_pq + 1/2 sum (pq|rs) E_pq E_rs, h'_pq = h_pq - 1/2 sum_r (pr|rq)."""
        ea, ebT, na, nb = self._ops(norb, nelec)
        h2 = np.asarray(h2, dtype=np.float64).reshape(norb, norb, norb, norb)
        hp = np.asarray(h1, dtype=np.float64) - 0.5 * np.einsum("prrq->pq", h2)
        D = self._excite_all(c, norb, nelec)
        sigma = np.tensordot(hp.reshape(-1), D, axes=(0, 0))
        G = (h2.reshape(norb * norb, norb * norb) @ D.reshape(norb * norb, -1)).reshape(D.shape)
        for p in range(norb):
            for q in range(norb):
                g = G[p * norb + q]
                sigma += 0.5 * (ea[p][q] @ g + (ebT[p][q].T @ g.T).T)
        if self.spin_penalty != 0.0:
            nelec = _nelec_pair(nelec)
            c = np.asarray(c, dtype=np.float64).reshape(na, nb)
            target = resolve_spin_target(self.spin_target, nelec)
            sigma += self.spin_penalty * (spin_square_vector(c, norb, nelec, self._ops(norb, nelec)) - target * c)
        return sigma

    def spin_square(self, ci, norb, nelec):
        """``(<S^2>, multiplicity)`` of a normalised CI vector, ``multiplicity = 2 (sqrt(<S^2> + 1/4) - 1/2) + 1``."""
        nelec = _nelec_pair(nelec)
        c = np.asarray(ci, dtype=np.float64).reshape(-1)
        ss = float(c @ spin_square_vector(c, norb, nelec, self._ops(norb, nelec)).reshape(-1))
        return ss, multiplicity_of(ss)

    def kernel(self, h1, h2, norb, nelec, nroots: int = 1, **_):
        """Lowest ``nroots`` eigenpairs.  Like PySCF: scalars/array for nroots == 1, lists otherwise."""
        if isinstance(nelec, (int, np.integer)):
            nelec = ((int(nelec) + 1) // 2, int(nelec) // 2)
        nelec = (int(nelec[0]), int(nelec[1]))
        _, _, na, nb = self._ops(norb, nelec)
        dim = na * nb
        self.spin_squares = None
        if self.spin_penalty != 0.0:
            target = resolve_spin_target(self.spin_target, nelec)      # refused before any work
        mv = lambda v: self.contract(h1, h2, v.reshape(na, nb), norb, nelec).reshape(-1)
        if dim <= self.dense_limit:
            H = np.empty((dim, dim))
            eye = np.zeros(dim)
            for k in range(dim):
                eye[k] = 1.0
                H[:, k] = mv(eye)
                eye[k] = 0.0
            H = 0.5 * (H + H.T)
            w, v = np.linalg.eigh(H)
        else:
            op = LinearOperator((dim, dim), matvec=mv, dtype=np.float64)
            rng = np.random.default_rng(0)
            w, v = eigsh(op, k=max(nroots, 1), which="SA", tol=self.tol, v0=rng.standard_normal(dim),
                         ncv=max(20, 2 * nroots + 10))
            order = np.argsort(w)
            w, v = w[order], v[:, order]
        vecs = []
        for k in range(nroots):
            x = v[:, k].copy()
            x *= np.sign(x[np.argmax(np.abs(x))])     # fixed sign convention
            vecs.append(x.reshape(na, nb))
        w = w[:nroots]
        if self.spin_penalty != 0.0:
            self.spin_squares = [self.spin_square(x, norb, nelec)[0] for x in vecs]
            w = unshift_roots(w, self.spin_squares, self.spin_penalty, target)
        if nroots == 1:
            return float(w[0]), vecs[0]
        return [float(x) for x in w[:nroots]], vecs

    def trans_rdm12(self, cibra, ciket, norb, nelec):
        if isinstance(nelec, (int, np.integer)):
            nelec = ((int(nelec) + 1) // 2, int(nelec) // 2)
        nelec = (int(nelec[0]), int(nelec[1]))
        n2 = norb * norb
        Dk = self._excite_all(ciket, norb, nelec).reshape(n2, -1)
        Db = self._excite_all(cibra, norb, nelec).reshape(n2, -1)
        bra = np.asarray(cibra, dtype=np.float64).reshape(-1)
        g1 = (Dk @ bra).reshape(norb, norb)                     # <bra| E_pq |ket>
        # <bra| E_pq E_rs |ket> = <E_qp bra | E_rs ket>
        DbT = Db.reshape(norb, norb, -1).transpose(1, 0, 2).reshape(n2, -1)
        M = (DbT @ Dk.T).reshape(norb, norb, norb, norb)
        dm2 = M - np.einsum("qr,ps->pqrs", np.eye(norb), g1)   # <p^+ r^+ s q>
        return g1.T.copy(), dm2                                 # dm1[p,q] = <q^+ p>

    def make_rdm12(self, ci, norb, nelec):
        return self.trans_rdm12(ci, ci, norb, nelec)

    def transform_ci(self, ci, nelec, u):
        """``fci_small.transform_ci``: what ``FCI_EVCont_obj`` calls to bring a state solved in another orbital basis
        into the OAO basis."""
        return transform_ci(ci, nelec, u)

    def energy(self, h1, h2, ci, norb, nelec) -> float:
        dm1, dm2 = self.make_rdm12(ci, norb, nelec)
        return float(np.sum(np.asarray(h1) * dm1.T) + 0.5 * np.sum(np.asarray(h2).reshape(dm2.shape) * dm2))
