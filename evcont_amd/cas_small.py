"""CASCI training states and the transition RDMs between CAS states that live in *different* orbital sets: the host
statement (numpy) that ``fci_device.DeviceFCI.cas_trans_rdm12_rows`` is held to.

A CAS state is ``(U, ncore, ncas, nelecas, ci)``: ``U`` (N, N), orthogonal, holds the molecular orbitals as columns in the
OAO basis (``X S C``, the reference's ``trafo``, ``CASCI_EVCont.py:219``): ``ncore`` doubly occupied, ``ncas`` active,
then virtuals; ``ci`` is the ``(na, nb)`` vector over the active strings in the order of ``fci_small``.

For a bra ``(Ua, ca)`` and a ket ``(Uk, ck)`` of one shape, with ``m = ncore + ncas`` and ``s = Ua[:, :m]^T Uk[:, :m]`` in
blocks ``s_cc, s_ca, s_ac, s_aa``:

    s_eff = s_aa - s_ac s_cc^-1 s_ca,  fac = det(s_cc)^2
    A_c = Oa_c,  A_a = Oa_a - Oa_c (s_ac s_cc^-1)^T,  B_c = Ok_c s_cc^-1,  B_a = (Ok_a - Ok_c s_cc^-1 s_ca) s_eff^-1
    ck~ = fac transform_ci(ck, nelecas, s_eff^T),  S = <ca|ck~>,  (d1, d2) = trans_rdm12(ca, ck~)
    Qc = A_c B_c^T,  Qa = A_a d1^T B_a^T
    dm1 = (2 S Qc + Qa)^T
    dm2[p,q,r,s] = S (4 Qc[p,q] Qc[r,s] - 2 Qc[p,s] Qc[r,q]) + 2 Qc[p,q] Qa[r,s] + 2 Qa[p,q] Qc[r,s]
                 - Qc[p,s] Qa[r,q] - Qa[p,s] Qc[r,q] + sum_tuvw d2[t,u,v,w] A_a[p,t] B_a[q,u] A_a[r,v] B_a[s,w]

``A_a`` holds the bra's active orbitals made orthogonal to the *ket's* core, so it belongs to the pair, not to the bra.
Exact multilinear algebra (the biorthogonal orbitals satisfy ``[A_c A_a]^T [B_c B_a] = 1``); a pair whose ``s_cc`` or
``s_eff`` has a smallest singular value below ``COND_LIMIT`` of its largest is refused (the reference's extended Wick
theorem handles such pairs, this module does not).  The error grows with ``cond(s_eff)``: like ``eps cond`` when one active
orbital alone turns towards a virtual (1.9e-12 at 1e5, the sweep of tests/test_cas_host.py), faster for generic pairs,
where the minors of ``transform_ci`` compound it: unrelated random orbitals with ``cond(s_eff)`` above about 5e3 can miss
1e-10 inside the guard.

``casci(mol, ncas, nelecas, cisolver)`` is the ground-state CASCI on RHF orbitals (``scf_small.rhf``) that produces such
states for any molecule ``integrals.ao_arrays`` accepts; ``casci_roots(..., nroots)`` gives the lowest ``nroots`` states on
the same orbitals.  The intermediates above depend on the two orbital sets, not on the CI vectors, so for several bras of
one orbital set ``trans_rdm12_block(bras, kets)`` forms them once per group of kets that share their orbitals (DESIGN.md
8.1.6); it is the statement ``DeviceFCI.cas_trans_rdm12_block`` is held to.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import fci_small
from .fci_small import _nelec_pair

COND_LIMIT = 1.0e-5     # smallest / largest singular value of s_cc and of s_eff


@dataclass(eq=False)
class CASState:
    U: np.ndarray                 # (N, N) orbitals in the OAO basis, columns: core, active, virtual
    ncore: int
    ncas: int
    nelecas: Tuple[int, int]
    ci: np.ndarray                # (na, nb) over the active strings
    e_tot: float = 0.0


def casci(mol, ncas: int, nelecas, cisolver) -> CASState:
    """Ground-state CASCI of ``mol`` on its RHF orbitals; ``nelecas``: active electrons, a number or ``(alpha, beta)``."""
    return _casci_states(mol, ncas, nelecas, cisolver, None)[0]


def casci_roots(mol, ncas: int, nelecas, cisolver, nroots: int):
    """The ``nroots`` lowest CASCI states of ``mol`` on its RHF orbitals, ``e_tot`` ascending: one RHF, one set of
    active-space integrals and one ``cisolver.kernel(..., nroots=nroots)``; every state holds the same ``U`` array."""
    if int(nroots) < 1:
        raise ValueError(f"casci_roots: nroots={nroots}, at least 1")
    return _casci_states(mol, ncas, nelecas, cisolver, int(nroots))


def _casci_states(mol, ncas: int, nelecas, cisolver, nroots: Optional[int]):
    """The body of ``casci`` (``nroots=None``: the solver's plain ground-state call) and ``casci_roots``."""
    from .integrals import ao_arrays, energy_nuc
    from .scf_small import rhf
    ao = ao_arrays(mol, need_grad=False)
    S, h = np.asarray(ao.S, dtype=np.float64), np.asarray(ao.hcore, dtype=np.float64)
    n = S.shape[0]
    eri = np.asarray(ao.eri, dtype=np.float64).reshape(n, n, n, n)
    na_tot, nb_tot = _nelec_pair(mol.nelec)
    nact = int(nelecas) if isinstance(nelecas, (int, np.integer)) else int(nelecas[0]) + int(nelecas[1])
    ncore2 = na_tot + nb_tot - nact
    if ncore2 < 0 or ncore2 % 2:
        raise ValueError(f"casci: {nact} active electrons of {na_tot + nb_tot} leave {ncore2} core electrons "
                         "(an even number >= 0)")
    ncore = ncore2 // 2
    nel = (na_tot - ncore, nb_tot - ncore)
    if ncas < 1 or ncore + ncas > n or min(nel) < 0 or max(nel) > ncas:
        raise ValueError(f"casci: ncore={ncore}, ncas={ncas}, nelecas={nel} for {n} orbitals")
    if not isinstance(nelecas, (int, np.integer)) and _nelec_pair(nelecas) != nel:
        raise ValueError(f"casci: nelecas={tuple(nelecas)}, but {ncore} core orbitals leave {nel}")
    Cm, _, converged = rhf(S, h, eri, (na_tot, nb_tot))
    assert converged
    Cc, Ca = Cm[:, :ncore], Cm[:, ncore:ncore + ncas]
    Dc = 2.0 * Cc @ Cc.T
    Vc = np.einsum("pqrs,rs->pq", eri, Dc) - 0.5 * np.einsum("prqs,rs->pq", eri, Dc)
    ecore = float(energy_nuc(mol)) + float(np.sum(Dc * (h + 0.5 * Vc)))
    h1eff = Ca.T @ (h + Vc) @ Ca
    h2 = np.einsum("pqrs,pi,qj,rk,sl->ijkl", eri, Ca, Ca, Ca, Ca, optimize=True)
    if nroots is None:
        e, ci = cisolver.kernel(h1eff, h2, ncas, nel)
        es, cis = [e], [ci]
    else:
        es, cis = cisolver.kernel(h1eff, h2, ncas, nel, nroots=nroots)
        if nroots == 1 and np.ndim(es) == 0:        # (a solver that returns one root bare)
            es, cis = [es], [cis]
        order = np.argsort(np.asarray(es, dtype=np.float64), kind="stable")
        es, cis = [es[i] for i in order], [cis[i] for i in order]
    w, V = np.linalg.eigh(S)
    U = (V * np.sqrt(w)) @ V.T @ Cm                 # X S C with X = S^(-1/2)
    return [CASState(U=U, ncore=ncore, ncas=ncas, nelecas=nel, ci=np.asarray(ci, dtype=np.float64),
                     e_tot=float(e) + ecore) for e, ci in zip(es, cis)]


def _same_shape(bra: CASState, ket: CASState) -> None:
    if (bra.ncore, bra.ncas, tuple(bra.nelecas), bra.U.shape) != (ket.ncore, ket.ncas, tuple(ket.nelecas), ket.U.shape):
        raise ValueError("cas_small: bra and ket differ in ncore, ncas, nelecas or the number of orbitals")


def _guard(name: str, mat: np.ndarray, label: str) -> None:
    if mat.size == 0:
        return
    sv = np.linalg.svd(mat, compute_uv=False)
    # (a pair built exactly at the limit passes whichever way its singular values round)
    if not sv[-1] >= COND_LIMIT * sv[0] * (1.0 - 1.0e-9):
        raise ValueError(f"cas_small: {name} of the pair {label} is ill-conditioned (singular values {sv[-1]:.3e} ... "
                         f"{sv[0]:.3e}, limit {COND_LIMIT:g}): the core or active spaces of the two states have swapped "
                         "character, which this reduction does not handle")


def pair_intermediates(bra: CASState, ket: CASState, label: str = "(bra, ket)"):
    """``(fac, s_eff, A_a, B_a, Qc)`` of one pair; ``ValueError`` beyond the conditioning guard."""
    _same_shape(bra, ket)
    nc, m = bra.ncore, bra.ncore + bra.ncas
    Oa, Ok = np.asarray(bra.U, dtype=np.float64)[:, :m], np.asarray(ket.U, dtype=np.float64)[:, :m]
    s = Oa.T @ Ok
    s_cc, s_ca, s_ac, s_aa = s[:nc, :nc], s[:nc, nc:], s[nc:, :nc], s[nc:, nc:]
    _guard("s_cc", s_cc, label)
    inv_cc = np.linalg.inv(s_cc) if nc else np.zeros((0, 0))
    s_eff = s_aa - s_ac @ inv_cc @ s_ca
    _guard("s_eff", s_eff, label)
    fac = float(np.linalg.det(s_cc)) ** 2 if nc else 1.0
    A_a = Oa[:, nc:] - Oa[:, :nc] @ (s_ac @ inv_cc).T
    B_c = Ok[:, :nc] @ inv_cc
    B_a = (Ok[:, nc:] - Ok[:, :nc] @ inv_cc @ s_ca) @ np.linalg.inv(s_eff)
    Qc = Oa[:, :nc] @ B_c.T
    return fac, s_eff, np.ascontiguousarray(A_a), np.ascontiguousarray(B_a), np.ascontiguousarray(Qc)


def expand(S: float, d1, d2, A_a, B_a, Qc):
    """Step 5: ``(dm1 (N,N), dm2 (N,N,N,N))`` from the active-space quantities of one pair."""
    Qa = A_a @ np.asarray(d1).T @ B_a.T
    dm1 = (2.0 * S * Qc + Qa).T
    dm2 = np.einsum("tuvw,pt,qu,rv,sw->pqrs", d2, A_a, B_a, A_a, B_a, optimize=True)
    dm2 += S * (4.0 * np.einsum("pq,rs->pqrs", Qc, Qc) - 2.0 * np.einsum("ps,rq->pqrs", Qc, Qc))
    dm2 += 2.0 * np.einsum("pq,rs->pqrs", Qc, Qa) + 2.0 * np.einsum("pq,rs->pqrs", Qa, Qc)
    dm2 -= np.einsum("ps,rq->pqrs", Qc, Qa) + np.einsum("ps,rq->pqrs", Qa, Qc)
    return dm1, dm2


def trans_rdm12_rows(bra: CASState, kets: Sequence[CASState], cisolver: Optional[object] = None):
    """``(ovlp (T,), dm1 (T,N,N), dm2 (T,N,N,N,N))`` of one bra against ``kets`` in the OAO basis, conventions of
    ``fci_small`` (``dm1[p,q] = <q^+ p>``, ``dm2[p,q,r,s] = <p^+ r^+ s q>``).  ``cisolver``: whose ``transform_ci`` and
    ``trans_rdm12`` to use (``fci_small`` without one)."""
    kets = list(kets)
    rotate = getattr(cisolver, "transform_ci", None) or fci_small.transform_ci
    solver = cisolver if hasattr(cisolver, "trans_rdm12") else fci_small.SmallFCI()
    n, T = bra.U.shape[0], len(kets)
    ovlp, dm1, dm2 = np.empty(T), np.empty((T, n, n)), np.empty((T, n, n, n, n))
    ca = np.asarray(bra.ci, dtype=np.float64)
    for i, ket in enumerate(kets):
        fac, s_eff, A_a, B_a, Qc = pair_intermediates(bra, ket, f"(bra, ket {i})")
        ck = fac * np.asarray(rotate(ket.ci, tuple(bra.nelecas), np.ascontiguousarray(s_eff.T)))
        ovlp[i] = float(np.dot(ca.reshape(-1), ck.reshape(-1)))
        d1, d2 = solver.trans_rdm12(ca, ck.reshape(ca.shape), bra.ncas, tuple(bra.nelecas))
        dm1[i], dm2[i] = expand(ovlp[i], d1, d2, A_a, B_a, Qc)
    return ovlp, dm1, dm2


def same_orbitals(a: CASState, b: CASState) -> bool:
    return a.U is b.U or (a.U.shape == b.U.shape and np.array_equal(a.U, b.U))


def ket_groups(kets: Sequence[CASState]):
    """``[(first, count)]``: the runs of consecutive kets that share their orbitals (one geometry's roots)."""
    groups, i = [], 0
    while i < len(kets):
        j = i + 1
        while j < len(kets) and same_orbitals(kets[i], kets[j]) and (kets[i].ncore, kets[i].ncas, tuple(
                kets[i].nelecas)) == (kets[j].ncore, kets[j].ncas, tuple(kets[j].nelecas)):
            j += 1
        groups.append((i, j - i))
        i = j
    return groups


def check_block(who: str, bras: Sequence[CASState], kets: Sequence[CASState]) -> None:
    if not bras or not kets:
        raise ValueError(f"{who}: no bras or no kets")
    for r, bra in enumerate(bras[1:], 1):
        _same_shape(bras[0], bra)
        if not same_orbitals(bras[0], bra):
            raise ValueError(f"{who}: bra {r} differs from bra 0 in its orbitals U (the bras of a block are the roots of "
                             "one geometry)")


def trans_rdm12_block(bras: Sequence[CASState], kets: Sequence[CASState], cisolver: Optional[object] = None):
    """``(ovlp (R,K), dm1 (R,K,N,N), dm2 (R,K,N,N,N,N))``: the stack of ``trans_rdm12_rows(bra_r, kets)`` for bras that
    share their orbitals (``ValueError`` otherwise).  The pair intermediates depend on the two orbital sets alone, so
    they are formed once per group of consecutive kets that share a ``U``, and each ket is rotated once.  Kets in the
    bras' own orbitals take the same route (``s_eff = 1`` to rounding)."""
    bras, kets = list(bras), list(kets)
    check_block("cas_small.trans_rdm12_block", bras, kets)
    rotate = getattr(cisolver, "transform_ci", None) or fci_small.transform_ci
    solver = cisolver if hasattr(cisolver, "trans_rdm12") else fci_small.SmallFCI()
    bra0 = bras[0]
    n, R, K = bra0.U.shape[0], len(bras), len(kets)
    nelec = tuple(bra0.nelecas)
    ovlp, dm1, dm2 = np.empty((R, K)), np.empty((R, K, n, n)), np.empty((R, K, n, n, n, n))
    for first, count in ket_groups(kets):
        fac, s_eff, A_a, B_a, Qc = pair_intermediates(bra0, kets[first], f"(bras, ket {first})")
        u = np.ascontiguousarray(s_eff.T)
        for i in range(first, first + count):
            _same_shape(bra0, kets[i])
            ck = fac * np.asarray(rotate(kets[i].ci, nelec, u))
            for r, bra in enumerate(bras):
                ca = np.asarray(bra.ci, dtype=np.float64)
                ovlp[r, i] = float(np.dot(ca.reshape(-1), ck.reshape(-1)))
                d1, d2 = solver.trans_rdm12(ca, ck.reshape(ca.shape), bra0.ncas, nelec)
                dm1[r, i], dm2[r, i] = expand(ovlp[r, i], d1, d2, A_a, B_a, Qc)
    return ovlp, dm1, dm2
