"""Observables of continuation states: the numpy statement of ``evc_properties_roots_batch`` (``csrc/properties.hip``).

The reference's workflow ends in them (``scripts/MD/H2O-H3O+/evaluate_dipole_moment_charges_continuation.py:72-90``, the
callback of ``04_Zundel_continuation_MD.py``): the eigenvector of the continuation gives the predicted 1-RDM in the OAO
basis, ``basis.dot(D).dot(basis.T)`` rotates it back to the AOs, and PySCF's ``dip_moment`` and a population analysis read
it.  Here the same for every pair of roots: slot (k, k) is state k, slot (k, l) the transition between k and l with the
symmetric weighting ``W = (c_k c_l^T + c_l c_k^T) / 2`` (the 1-RDM ``evc_outputs_roots.d_pred`` holds).

The population analysis is PLAIN Mulliken (PySCF's ``mulliken_pop``) and Loewdin.  The reference's script calls
``mulliken_meta``, which first orthogonalises against PySCF's tabulated atomic reference orbitals (meta-Loewdin); that
needs those tables and is not provided.

Everything here is host numpy: the device route is ``BatchedEvaluator.multistate_properties`` /
``ab_initio_eigenvector_continuation.get_multistate_properties``, and these functions are the oracle of its tests.
"""
from __future__ import annotations

import numpy as np

AU2DEBYE = 2.541746473   # e Bohr in Debye (PySCF's nist.AU2DEBYE)


def pair_weighting(c_k, c_l) -> np.ndarray:
    """``W = (c_k c_l^T + c_l c_k^T) / 2``; ``c_k c_k^T`` for one vector."""
    c_k, c_l = np.asarray(c_k, dtype=np.float64), np.asarray(c_l, dtype=np.float64)
    return 0.5 * (np.outer(c_k, c_l) + np.outer(c_l, c_k))


def predicted_one_rdm(one_RDM, c_k, c_l=None) -> np.ndarray:
    """OAO 1-RDM ``sum_ab W[a,b] one_RDM[a,b]`` of root k (or of the pair (k, l)); ``one_RDM`` (T,T,N,N)."""
    one = np.asarray(one_RDM, dtype=np.float64)
    return np.tensordot(pair_weighting(c_k, c_k if c_l is None else c_l), one, axes=2)


def predicted_one_rdm_ao(one_RDM, X, c_k, c_l=None) -> np.ndarray:
    """The same in the AO basis, ``X D X^T`` with ``X = S^-1/2`` (the script's ``basis.dot(D).dot(basis.T)``)."""
    X = np.asarray(X, dtype=np.float64)
    return X @ predicted_one_rdm(one_RDM, c_k, c_l) @ X.T


def dip_moment(charges, coords, dip_ao, dm_ao, origin=(0.0, 0.0, 0.0), unit="AU", transition=False) -> np.ndarray:
    """``sum_A Z_A (R_A - O) - tr(P r)`` (PySCF's ``dip_moment``: ``einsum('xij,ji->x', ao_dip, dm)``), ``dip_ao``
    (3,N,N) = <mu| r - O |nu> for the same origin.  ``transition``: the electronic part ``-tr(P r)`` alone (a transition
    density carries no nuclear term).  ``unit``: "AU" (e Bohr) or "Debye"."""
    el = np.einsum("xij,ji->x", np.asarray(dip_ao, dtype=np.float64), np.asarray(dm_ao, dtype=np.float64))
    mu = -el
    if not transition:
        Z = np.asarray(charges, dtype=np.float64)
        R = np.asarray(coords, dtype=np.float64).reshape(-1, 3) - np.asarray(origin, dtype=np.float64)
        mu = Z @ R - el
    if unit.upper() == "DEBYE":
        return mu * AU2DEBYE
    if unit.upper() != "AU":
        raise ValueError(f"unit={unit!r} (known: 'AU', 'Debye')")
    return mu


def _atom_sums(per_ao, aoslices) -> np.ndarray:
    return np.array([np.sum(per_ao[int(a): int(b)]) for a, b in np.asarray(aoslices).reshape(-1, 2)])


def mulliken_pop(dm_ao, S, aoslices) -> np.ndarray:
    """Plain Mulliken populations ``sum_{mu in A} (P S)_mu,mu`` (PySCF's ``mulliken_pop``: ``einsum('ij,ji->i', dm, s)``).
    Not ``mulliken_meta``."""
    return _atom_sums(np.einsum("ij,ji->i", np.asarray(dm_ao, dtype=np.float64), np.asarray(S, dtype=np.float64)),
                      aoslices)


def loewdin_pop(dm_oao, aoslices) -> np.ndarray:
    """Loewdin populations ``sum_{mu in A} D_mu,mu``: the OAO basis is the Loewdin basis, so they are the diagonal of
    the OAO 1-RDM (= ``(S^1/2 P S^1/2)_mu,mu``)."""
    return _atom_sums(np.diagonal(np.asarray(dm_oao, dtype=np.float64)), aoslices)


def oscillator_strength(E_k, E_l, mu_kl):
    """``f = 2/3 (E_l - E_k) |mu_kl|^2`` (length gauge, atomic units); ``mu_kl`` (..., 3)."""
    mu = np.asarray(mu_kl, dtype=np.float64)
    return 2.0 / 3.0 * (np.asarray(E_l, dtype=np.float64) - np.asarray(E_k, dtype=np.float64)) * np.sum(mu * mu, axis=-1)


def charges_from_populations(pops, charges, pairs) -> np.ndarray:
    """``Z - pop`` on the diagonal slots, ``-pop`` on the transition slots; ``pops`` (..., P, A)."""
    q = -np.array(pops, dtype=np.float64)
    for p, (k, l) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        if k == l:
            q[..., p, :] += np.asarray(charges, dtype=np.float64)
    return q


def properties_host(one_RDM, X, C, pairs, S, dip_ao, aoslices, charges, coords, origin=(0.0, 0.0, 0.0)) -> dict:
    """Every output of ``evc_properties_roots_batch`` for ONE geometry: ``C`` (nvec,T) coefficient rows, ``pairs``
    (P,2).  Returns ``d_oao``, ``d_ao`` (P,N,N), ``dipole`` (P,3), ``mulliken``, ``loewdin`` (P,A) populations."""
    out = {k: [] for k in ("d_oao", "d_ao", "dipole", "mulliken", "loewdin")}
    X = np.asarray(X, dtype=np.float64)
    for k, l in np.asarray(pairs).reshape(-1, 2):
        D = predicted_one_rdm(one_RDM, C[k], C[l])
        P = X @ D @ X.T
        out["d_oao"].append(D)
        out["d_ao"].append(P)
        out["dipole"].append(dip_moment(charges, coords, dip_ao, P, origin, transition=k != l))
        out["mulliken"].append(mulliken_pop(P, S, aoslices))
        out["loewdin"].append(loewdin_pop(D, aoslices))
    return {k: np.array(v) for k, v in out.items()}


def ir_intensities(apt, modes, masses) -> np.ndarray:
    """Infrared intensities ``|d mu / dQ_k|^2 = |sum_Ax P[A,x,:] L[Ax,k] / sqrt(m_A)|^2`` per normal mode, in atomic
    units (e^2 / m_e when ``masses`` are in electron masses).  ``apt`` (A,3,3) = ``P[A,x,c] = d mu_c / dR_Ax`` (the
    atomic polar tensor of ONE state, ``get_multistate_field_response``), ``modes`` (3A,K) the columns ``L[:,k]`` of the
    eigenvectors of the mass-weighted Hessian (rows ordered atom-major, x y z), ``masses`` (A,).  No unit conversion is
    applied (none is tabulated here); relative stick heights need none."""
    P = np.asarray(apt, dtype=np.float64)
    A = P.shape[0]
    L = np.asarray(modes, dtype=np.float64).reshape(3 * A, -1)
    m = np.repeat(np.asarray(masses, dtype=np.float64).reshape(A), 3)
    dmu = np.einsum("rc,rk->ck", P.reshape(3 * A, 3), L / np.sqrt(m)[:, None])
    return np.sum(dmu * dmu, axis=0)
