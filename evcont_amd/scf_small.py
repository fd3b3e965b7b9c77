"""Restricted Hartree-Fock on AO arrays, for the canonical orbital basis of array-level molecules
(``electron_integral_utils.get_basis(mol, "canonical")``): host numpy, DIIS, core-Hamiltonian start.

The orbitals only choose the basis an FCI is solved in -- any orthonormal basis gives the same FCI state -- so the
convergence of the SCF changes the speed of the FCI solver and never its result.
"""
from __future__ import annotations

import warnings
from typing import Tuple

import numpy as np


def _nelec_pair(nelec) -> Tuple[int, int]:
    if isinstance(nelec, (int, np.integer)):
        return (int(nelec) + 1) // 2, int(nelec) // 2
    return int(nelec[0]), int(nelec[1])


def rhf(S, hcore, eri, nelec, conv_tol: float = 1e-10, max_cycle: int = 100, diis_space: int = 8):
    """``(mo_coeff, mo_energy, converged)``: ``mo_coeff`` (n, n) with ``C^T S C = 1``, columns by ascending orbital
    energy.  ``eri`` is ``(n, n, n, n)`` in chemists' order.  For ``n_alpha != n_beta`` the Fock matrix is built from the
    spin-averaged density (occupations 2 and 1).  Converged when the DIIS error ``F D S - S D F`` is below ``conv_tol``
    in the max norm; a run that is not warns and returns its last orbitals."""
    S = np.asarray(S, dtype=np.float64)
    h = np.asarray(hcore, dtype=np.float64)
    n = S.shape[0]
    eri = np.asarray(eri, dtype=np.float64).reshape(n, n, n, n)
    na, nb = _nelec_pair(nelec)
    if not (0 <= nb <= na <= n):
        raise ValueError(f"rhf: nelec=({na}, {nb}) for {n} orbitals (n_alpha >= n_beta)")
    occ = np.zeros(n)
    occ[:na] += 1.0
    occ[:nb] += 1.0
    w, V = np.linalg.eigh(S)
    X = V / np.sqrt(w) @ V.T                                       # S^(-1/2)

    def diagonalise(F):
        e, Cp = np.linalg.eigh(X.T @ F @ X)
        return e, X @ Cp

    e, Cm = diagonalise(h)
    fs, errs = [], []
    converged = False
    for _ in range(max_cycle):
        D = (Cm * occ) @ Cm.T
        F = h + np.einsum("pqrs,rs->pq", eri, D) - 0.5 * np.einsum("prqs,rs->pq", eri, D)
        err = X.T @ (F @ D @ S - S @ D @ F) @ X
        if np.abs(err).max() < conv_tol:
            converged = True
            e, Cm = diagonalise(F)
            break
        fs.append(F)
        errs.append(err)
        fs, errs = fs[-diis_space:], errs[-diis_space:]
        m = len(fs)
        if m > 1:
            B = -np.ones((m + 1, m + 1))
            B[m, m] = 0.0
            for i in range(m):
                for j in range(m):
                    B[i, j] = np.vdot(errs[i], errs[j])
            rhs = np.zeros(m + 1)
            rhs[m] = -1.0
            try:
                coef = np.linalg.solve(B, rhs)[:m]
                F = sum(c * f for c, f in zip(coef, fs))
            except np.linalg.LinAlgError:
                fs, errs = fs[-1:], errs[-1:]
        e, Cm = diagonalise(F)
    if not converged:
        warnings.warn(f"scf_small.rhf: not converged in {max_cycle} cycles; returning the last orbitals "
                      "(the FCI state does not depend on them, the solver's iteration count does)")
    return Cm, e, converged
