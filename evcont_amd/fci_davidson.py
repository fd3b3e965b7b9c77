"""Block Davidson for the lowest eigenpairs of the full-CI Hamiltonian, with the diagonal of H as preconditioner, written
once against a small set of vector operations (``DavidsonOps``): the CI-length vectors live wherever the operations keep
them, and the driver sees only the projected matrix, the Ritz coefficients and the residual norms.

``fci_device.DeviceFCI(eigensolver="davidson")`` runs it on ``fci_device._DeviceOps`` (csrc/fci_solve.hip and
``evc_fci_sigma`` on vectors that never leave the device).  ``NumpyOps`` states the same operations in numpy on
``SmallFCI.contract``: it exists so that the restart, deflation and convergence logic is tested without a GPU, and is not
a host route of ``DeviceFCI``.

Vector sets: ``"V"`` (the basis, ``max_space`` rows), ``"W"`` (``H V``, row by row) and ``"S"`` (``2 nroots`` rows of
scratch: the corrections, the collapsed basis at a restart, the Ritz vectors at the end).
"""
from __future__ import annotations

import warnings
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .fci_small import SmallFCI, _strings, resolve_spin_target, spin_constant

DEPENDENT = 1e-3     # a correction that keeps less than this of its norm through the projections is dropped
DENOM_FLOOR = 1e-8   # |hdiag - theta| is floored here, keeping its sign


# ---- the diagonal, in numpy ------------------------------------------------------------
def occupations(norb: int, nocc: int) -> np.ndarray:
    """``(n_strings, norb)`` 0/1 occupation numbers of the strings in their order (by integer value)."""
    strs = np.asarray(_strings(norb, nocc), dtype=np.int64)
    return ((strs[:, None] >> np.arange(norb)[None, :]) & 1).astype(np.float64)


def hdiag_numpy(h1, h2, norb: int, nelec: Tuple[int, int], spin_penalty: float = 0.0,
                spin_target: float = 0.0) -> np.ndarray:
    """``<I|H|I>`` of ``H = sum h'_pq E_pq + 1/2 sum (pq|rs) E_pq E_rs`` (``SmallFCI.contract``), ``(na, nb)``; no
    permutation symmetry of ``h2`` assumed:
    ``sum_p h'_pp n_p + 1/2 sum_pr (pp|rr) n_p n_r + 1/2 sum_{p != q} (pq|qp) sum_spin n_p,spin (1 - n_q,spin)``.
    A non-zero ``spin_penalty`` adds ``spin_penalty (<I|S^2|I> - spin_target)``, ``<I|S^2|I> = Sz (Sz + 1) + n_beta`` less
    the doubly occupied orbitals of ``I``: the diagonal of the operator ``SmallFCI(spin_penalty=...)`` contracts."""
    h1 = np.asarray(h1, dtype=np.float64).reshape(norb, norb)
    h2 = np.asarray(h2, dtype=np.float64).reshape(norb, norb, norb, norb)
    hp = np.diag(h1) - 0.5 * np.einsum("prrp->p", h2)
    J = np.einsum("pprr->pr", h2)
    K = np.einsum("pqqp->pq", h2)
    oa, ob = occupations(norb, int(nelec[0])), occupations(norb, int(nelec[1]))
    n = oa[:, None, :] + ob[None, :, :]
    out = n @ hp + 0.5 * np.einsum("abp,pr,abr->ab", n, J, n)
    ea = 0.5 * np.einsum("ap,pq,aq->a", oa, K, 1.0 - oa)
    eb = 0.5 * np.einsum("bp,pq,bq->b", ob, K, 1.0 - ob)
    out = out + ea[:, None] + eb[None, :]
    if spin_penalty != 0.0:
        out = out + spin_penalty * ((spin_constant(nelec) - spin_target) - oa @ ob.T)
    return out


# ---- vector operations -----------------------------------------------------------------
class DavidsonOps:
    """What the driver asks of a back-end.  ``name`` is ``"V"``, ``"W"`` or ``"S"``; rows are ``[first, first + count)``.
    Small matrices (coefficients, products, norms) are host numpy arrays."""

    dim: int
    nsigma: int = 0

    def prepare(self, nroots: int, max_space: int) -> None:
        """Storage for ``max_space`` rows of V and W and ``2 nroots`` rows of S; computes the diagonal."""
        raise NotImplementedError

    def lowest(self, n: int) -> List[int]:
        """Indices of the ``n`` lowest diagonal elements, ties to the lower index."""
        raise NotImplementedError

    def load(self, name: str, row: int, vec: np.ndarray) -> None:
        raise NotImplementedError

    def fetch(self, name: str, row: int) -> np.ndarray:
        raise NotImplementedError

    def copy(self, dst: str, d0: int, src: str, s0: int, count: int) -> None:
        raise NotImplementedError

    def sigma(self, row: int) -> None:
        """``W[row] = H V[row]``."""
        raise NotImplementedError

    def dots(self, x: str, x0: int, nx: int, y: str, y0: int, ny: int) -> np.ndarray:
        """``(nx, ny)`` products ``X_i . Y_j``."""
        raise NotImplementedError

    def combine(self, out: str, o0: int, src: str, s0: int, coef: np.ndarray, beta: float) -> None:
        """``Out_r = beta Out_r + sum_j coef[j, r] Src_j`` for the ``coef.shape[1]`` rows of ``out`` from ``o0``."""
        raise NotImplementedError

    def correction(self, m: int, y: np.ndarray, theta: np.ndarray) -> np.ndarray:
        """For the Ritz pairs ``(theta_r, V[:m]^T y[:, r])``: ``S[r] = r_r / (hdiag - theta_r)`` (floored denominator)
        and the squared residual norms ``|r_r|^2``."""
        raise NotImplementedError


class NumpyOps(DavidsonOps):
    """The operations in numpy, the sigma vector from ``SmallFCI.contract``."""

    def __init__(self, h1, h2, norb: int, nelec: Tuple[int, int], solver: Optional[SmallFCI] = None):
        self.h1, self.h2, self.norb, self.nelec = h1, h2, norb, (int(nelec[0]), int(nelec[1]))
        self.solver = solver if solver is not None else SmallFCI()
        _, _, self.na, self.nb = self.solver._ops(norb, self.nelec)
        self.dim = self.na * self.nb
        self.nsigma = 0
        self.sets = {}
        self.hdiag = None

    def prepare(self, nroots, max_space):
        self.sets = {"V": np.zeros((max_space, self.dim)), "W": np.zeros((max_space, self.dim)),
                     "S": np.zeros((2 * nroots, self.dim))}
        shift = self.solver.spin_penalty
        target = resolve_spin_target(self.solver.spin_target, self.nelec) if shift != 0.0 else 0.0
        self.hdiag = hdiag_numpy(self.h1, self.h2, self.norb, self.nelec, shift, target).reshape(-1)

    def lowest(self, n):
        return [int(i) for i in np.argsort(self.hdiag, kind="stable")[:n]]

    def load(self, name, row, vec):
        self.sets[name][row] = np.asarray(vec, dtype=np.float64).reshape(-1)

    def fetch(self, name, row):
        return self.sets[name][row].copy()

    def copy(self, dst, d0, src, s0, count):
        self.sets[dst][d0:d0 + count] = self.sets[src][s0:s0 + count]

    def sigma(self, row):
        self.nsigma += 1
        c = self.sets["V"][row].reshape(self.na, self.nb)
        self.sets["W"][row] = self.solver.contract(self.h1, self.h2, c, self.norb, self.nelec).reshape(-1)

    def dots(self, x, x0, nx, y, y0, ny):
        return self.sets[x][x0:x0 + nx] @ self.sets[y][y0:y0 + ny].T

    def combine(self, out, o0, src, s0, coef, beta):
        m, k = coef.shape
        o = self.sets[out][o0:o0 + k]
        new = coef.T @ self.sets[src][s0:s0 + m] if m else 0.0
        o[...] = new if beta == 0.0 else beta * o + new

    def correction(self, m, y, theta):
        k = y.shape[1]
        x = y.T @ self.sets["V"][:m]
        r = y.T @ self.sets["W"][:m] - theta[:, None] * x
        d = self.hdiag[None, :] - theta[:, None]
        d = np.where(np.abs(d) < DENOM_FLOOR, np.where(d < 0.0, -DENOM_FLOOR, DENOM_FLOOR), d)
        self.sets["S"][:k] = r / d
        return np.einsum("rk,rk->r", r, r)


# ---- the iteration ---------------------------------------------------------------------
def _orthonormal_coefficients(gram: np.ndarray, before: np.ndarray) -> np.ndarray:
    """Coefficients ``C`` (k, k') with ``C^T gram C = 1`` for the vectors whose Gram matrix is ``gram``: vectors whose
    squared norm fell below ``DEPENDENT^2`` of ``before`` are left out, and so are the directions in which the remaining,
    normalised, vectors are dependent on each other to the same degree."""
    k = gram.shape[0]
    diag = np.diag(gram)
    keep = [r for r in range(k) if before[r] > 0.0 and diag[r] > DEPENDENT ** 2 * before[r]]
    if not keep:
        return np.zeros((k, 0))
    scale = 1.0 / np.sqrt(diag[keep])
    g = gram[np.ix_(keep, keep)] * scale[:, None] * scale[None, :]
    w, u = np.linalg.eigh(0.5 * (g + g.T))
    good = w > DEPENDENT
    c = np.zeros((k, int(good.sum())))
    c[keep] = (scale[:, None] * u[:, good]) / np.sqrt(w[good])[None, :]
    return c


def _append(ops: DavidsonOps, m: int, k: int, room: int) -> int:
    """Orthogonalise S[0:k] against V[0:m] (two passes) and among themselves, append what is left (at most ``room``
    vectors) to V, their sigma vectors to W; returns how many were appended."""
    before = np.diag(ops.dots("S", 0, k, "S", 0, k)).copy()
    if m:
        for _ in range(2):
            ops.combine("S", 0, "V", 0, -ops.dots("V", 0, m, "S", 0, k), 1.0)
    c = _orthonormal_coefficients(ops.dots("S", 0, k, "S", 0, k), before)[:, :room]
    n = c.shape[1]
    if n:
        ops.combine("V", m, "S", 0, c, 0.0)
        for r in range(n):
            ops.sigma(m + r)
    return n


def _collapse_coefficients(y: np.ndarray, y_prev: Optional[np.ndarray], limit: int) -> np.ndarray:
    """Orthonormal columns spanning the current Ritz coefficients and, as far as ``limit`` allows, the previous ones."""
    cols = [y[:, r] for r in range(y.shape[1])]
    if y_prev is not None:
        cols += [y_prev[:, r] for r in range(y_prev.shape[1])]
    q = []
    for c in cols:
        if len(q) >= limit:
            break
        v = c.copy()
        for _ in range(2):
            for u in q:
                v -= (u @ v) * u
        nv = np.linalg.norm(v)
        if nv > DEPENDENT * np.linalg.norm(c):
            q.append(v / nv)
    return np.array(q).T


def davidson(ops: DavidsonOps, nroots: int = 1, conv_tol: float = 1e-10, max_space: Optional[int] = None,
             max_cycle: int = 300, ci0: Optional[Sequence[np.ndarray]] = None):
    """Lowest ``nroots`` eigenpairs.  Returns ``(energies (nroots,), vectors (nroots, dim) as the back-end delivers
    them -- unit norm up to rounding, sign not fixed --, converged, info)`` with ``info = dict(iterations, nsigma,
    restarts, residuals)``.

    A root is converged when its residual 2-norm is at most ``conv_tol``; the basis never exceeds
    ``min(dim, max_space)`` vectors (``max_space`` defaults to ``8 nroots + 12``) and is collapsed, when the next
    corrections do not fit, onto the current and the previous iteration's Ritz vectors, which costs no sigma vector."""
    dim = ops.dim
    if not 1 <= nroots <= dim:
        raise ValueError(f"davidson: nroots={nroots} for {dim} determinants")
    if max_space is None:
        max_space = 8 * nroots + 12
    mmax = min(dim, int(max_space))
    if mmax < min(dim, nroots + 1):
        raise ValueError(f"davidson: max_space={max_space} leaves no room beside {nroots} roots")
    ops.prepare(nroots, mmax)
    ops.nsigma = 0
    # start vectors: the lowest diagonal elements, each with a little of everything
    rng = np.random.default_rng(0)
    guess = []
    for i in ops.lowest(nroots):
        g = rng.standard_normal(dim)
        v = 1e-3 * g / np.linalg.norm(g)
        v[i] += 1.0
        guess.append(v)
    if ci0 is not None:
        given = [ci0] if isinstance(ci0, np.ndarray) and ci0.size == dim else list(ci0)
        for r, v in enumerate(given[:nroots]):
            v = np.asarray(v, dtype=np.float64).reshape(-1)
            if v.size != dim:
                raise ValueError(f"davidson: ci0[{r}] has {v.size} elements, expected {dim}")
            guess[r] = v
    for r, v in enumerate(guess):
        ops.load("S", r, v)
    m = _append(ops, 0, nroots, mmax)
    if m < nroots:
        raise ValueError("davidson: the start vectors are linearly dependent")
    H = np.zeros((mmax, mmax))
    H[:m, :m] = ops.dots("V", 0, m, "W", 0, m)
    y_prev = None
    converged, restarts, nact = False, 0, nroots
    res = np.full(nroots, np.inf)
    theta, y = None, None
    it = 0
    for it in range(1, max_cycle + 1):
        Hm = 0.5 * (H[:m, :m] + H[:m, :m].T)
        w, u = np.linalg.eigh(Hm)
        theta, y = w[:nroots].copy(), u[:, :nroots].copy()
        if m == dim:                    # the basis is complete: the Ritz pairs are exact
            res = np.zeros(nroots)
            converged = True
            break
        if mmax - m < nact and m > nroots:
            q = _collapse_coefficients(y, y_prev, min(2 * nroots, mmax - 1))
            if q.shape[1] < m:
                for name in ("V", "W"):
                    ops.combine("S", 0, name, 0, q, 0.0)
                    ops.copy(name, 0, "S", 0, q.shape[1])
                Hq = q.T @ Hm @ q
                y = q.T @ y
                m = q.shape[1]
                H[:m, :m] = Hq
                y_prev = None
                restarts += 1
        res = np.sqrt(np.maximum(ops.correction(m, y, theta), 0.0))
        done = res <= conv_tol
        if done.all():
            converged = True
            break
        if it == max_cycle:
            break
        active = [r for r in range(nroots) if not done[r]]
        nact = len(active)
        for slot, r in enumerate(active):          # the corrections of the unconverged roots, packed to the front
            if slot != r:
                ops.copy("S", slot, "S", r, 1)
        n = _append(ops, m, nact, mmax - m)
        if n == 0:
            break
        H[:m + n, m:m + n] = ops.dots("V", 0, m + n, "W", m, n)
        H[m:m + n, :m] = H[:m, m:m + n].T
        y_prev = np.vstack([y, np.zeros((n, nroots))])
        m += n
    ops.combine("S", 0, "V", 0, y, 0.0)
    vecs = np.array([ops.fetch("S", r) for r in range(nroots)])
    info = dict(iterations=it, nsigma=ops.nsigma, restarts=restarts, residuals=res)
    if not converged:
        warnings.warn(f"davidson: not converged after {it} iterations ({ops.nsigma} sigma vectors): residual norms "
                      f"{res}, conv_tol {conv_tol}", RuntimeWarning, stacklevel=2)
    return theta, vecs, converged, info
