"""CPU tests of ``evcont_amd.cas_small``: the reduction of a CAS pair in two orbital sets to a non-orthogonal
``transform_ci`` and an active-space t-RDM, against the full-space embedding oracle of tests/cas_reference.py, its
conditioning guard, and the CASCI driver and container built on it."""
import copy
import functools

import numpy as np
import pytest

from evcont_amd import cas_small
from evcont_amd.cas_small import CASState
from evcont_amd.fci_small import SmallFCI, transform_ci
from cas_reference import (near_rotation, oracle_rows, random_ci, random_orthogonal, random_state, sweep_pair)

_HOST = SmallFCI()
# (N, ncore, ncas, nelecas)
SHAPES = [(6, 1, 3, (2, 1)), (6, 2, 3, (1, 1)), (7, 0, 4, (2, 2)), (8, 2, 4, (2, 2)), (6, 1, 5, (2, 2)),   # no virtuals
          (6, 2, 4, (2, 1))]                                                                               # Uk = Ua
IDS = ["-".join(map(str, (n, c, a) + e)) for n, c, a, e in SHAPES]


def worst(got, want):
    return max(float(np.abs(np.asarray(g) - np.asarray(w)).max()) for g, w in zip(got, want))


def pair_conditions(bra, ket):
    """cond(s_cc) and cond(s_eff) of a pair, from the orbitals alone."""
    nc, m = bra.ncore, bra.ncore + bra.ncas
    s = bra.U[:, :m].T @ ket.U[:, :m]
    schur = s[nc:, nc:] - (s[nc:, :nc] @ np.linalg.solve(s[:nc, :nc], s[:nc, nc:]) if nc else 0.0)
    return (float(np.linalg.cond(s[:nc, :nc])) if nc else 1.0), float(np.linalg.cond(schur))


def unrelated_ket(bra, rng, limit=30.0):
    """A ket with fully random orbitals, unrelated to the bra's.  The parity bound of 1e-13 is one for pairs of ordinary
    conditioning: the error of the reduction grows with cond(s_eff) (test_conditioning_sweep holds it along that axis),
    and one random draw in a few dozen has cond(s_eff) of several hundred.  Such draws are passed over: the condition is
    one of the input orbitals and is computed here, not by the code under test.

    Why 30: for generic pairs the error grows faster than eps cond -- the rotated ket vector is made of minors of s_eff
    up to the order of the electron count, so roughly like a power of cond between 2 and 3.  Surveyed draws at the shapes
    of this file: up to cond 27 the worst difference was 7e-15; (6,1,5,(2,2)) with cond 1.9e2 gave 6.8e-13, already
    over the bound of 1e-13, while other shapes hold it up to a few hundred.  30 is the round figure that leaves a decade
    between the surveyed errors and the bound at every shape; most draws pass it."""
    while True:
        ket = random_state(bra.U.shape[0], bra.ncore, bra.ncas, bra.nelecas, rng)
        if max(pair_conditions(bra, ket)) <= limit:
            return ket


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_parity_with_the_embedding_oracle(shape):
    n, ncore, ncas, nelecas = shape
    rng = np.random.default_rng(100 + 7 * n + ncore)
    bra = random_state(n, ncore, ncas, nelecas, rng)
    same = shape == SHAPES[-1]
    kets = [random_state(n, ncore, ncas, nelecas, rng, U=bra.U) if same else unrelated_ket(bra, rng), bra]
    got = cas_small.trans_rdm12_rows(bra, kets)
    err = worst(got, oracle_rows(bra, kets))
    print(f"cas host parity {shape}: worst |d| = {err:.2e}")
    assert err <= 1e-13


def embedded_cas_rdms(bra, ket):
    """Uk = Ua: the ordinary active-space t-RDMs, rotated with the active orbitals, plus the core terms."""
    nc, m, n = bra.ncore, bra.ncore + bra.ncas, bra.U.shape[0]
    S = float(np.vdot(bra.ci, ket.ci))
    d1, d2 = _HOST.trans_rdm12(bra.ci, ket.ci, bra.ncas, bra.nelecas)
    Ca, Cc = bra.U[:, nc:m], bra.U[:, :nc]
    P = Cc @ Cc.T
    Qa = Ca @ d1.T @ Ca.T
    dm1 = (2 * S * P + Qa).T
    dm2 = np.einsum("tuvw,pt,qu,rv,sw->pqrs", d2, Ca, Ca, Ca, Ca, optimize=True)
    dm2 += S * (4 * np.einsum("pq,rs->pqrs", P, P) - 2 * np.einsum("ps,rq->pqrs", P, P))
    dm2 += 2 * np.einsum("pq,rs->pqrs", P, Qa) + 2 * np.einsum("pq,rs->pqrs", Qa, P)
    dm2 -= np.einsum("ps,rq->pqrs", P, Qa) + np.einsum("ps,rq->pqrs", Qa, P)
    return S, dm1, dm2


def test_orbital_relations():
    n, ncore, ncas, nelecas = 7, 2, 3, (2, 1)
    rng = np.random.default_rng(5)
    bra = random_state(n, ncore, ncas, nelecas, rng)
    unrelated = unrelated_ket(bra, rng)
    near = random_state(n, ncore, ncas, nelecas, rng, U=near_rotation(bra.U, rng))
    same = random_state(n, ncore, ncas, nelecas, rng, U=bra.U)
    kets = [unrelated, near, same]
    got = cas_small.trans_rdm12_rows(bra, kets)
    assert worst(got, oracle_rows(bra, kets)) <= 1e-13
    S, dm1, dm2 = embedded_cas_rdms(bra, same)
    assert abs(got[0][2] - S) <= 1e-14
    assert worst((got[1][2], got[2][2]), (dm1, dm2)) <= 1e-13


def test_identities():
    # no core and no virtuals: the plain t-RDMs after transform_ci into the OAO basis
    n, nelecas = 5, (3, 2)
    rng = np.random.default_rng(11)
    bra, ket = random_state(n, 0, n, nelecas, rng), random_state(n, 0, n, nelecas, rng)
    ov, dm1, dm2 = cas_small.trans_rdm12_rows(bra, [ket])
    cb, ck = transform_ci(bra.ci, nelecas, bra.U.T), transform_ci(ket.ci, nelecas, ket.U.T)
    d1, d2 = _HOST.trans_rdm12(cb, ck, n, nelecas)
    assert abs(ov[0] - np.vdot(cb, ck)) <= 1e-13 and worst((dm1[0], dm2[0]), (d1, d2)) <= 1e-13
    # bra = ket: S = 1, tr dm1 = n_electrons, dm2 contracts to dm1
    n, ncore, ncas, nelecas = 7, 2, 3, (2, 1)
    st = random_state(n, ncore, ncas, nelecas, rng)
    ov, dm1, dm2 = cas_small.trans_rdm12_rows(st, [st])
    nel = 2 * ncore + sum(nelecas)
    assert abs(ov[0] - 1.0) <= 1e-13 and abs(np.trace(dm1[0]) - nel) <= 1e-12
    assert np.abs(np.einsum("pqrr->pq", dm2[0]) - (nel - 1) * dm1[0]).max() <= 1e-12


@functools.lru_cache(maxsize=None)
def sweep_error(decade):
    bra, ket = sweep_pair(10.0 ** decade, np.random.default_rng(40 + decade))
    _, s_eff, _, _, _ = cas_small.pair_intermediates(bra, ket)
    sv = np.linalg.svd(s_eff, compute_uv=False)
    return float(sv[0] / sv[-1]), worst(cas_small.trans_rdm12_rows(bra, [ket]), oracle_rows(bra, [ket]))


def test_conditioning_sweep():
    """(7,2,3,(2,1)), Uk = Ua R with one active ket orbital rotated towards a virtual: cond(s_eff) = 1e1 ... 1e5.  The
    error grows like eps cond(s_eff); at 1e5 it must be <= 1e-11."""
    for decade in range(1, 6):
        cond, err = sweep_error(decade)
        print(f"cas conditioning sweep: cond(s_eff) = {cond:.3e}  worst |d| = {err:.2e}")
        assert 0.5 * 10.0 ** decade <= cond <= 2.0 * 10.0 ** decade
    assert sweep_error(5)[1] <= 1e-11


def test_pairs_beyond_the_guard_are_refused():
    rng = np.random.default_rng(46)
    bra, ket = sweep_pair(1.0e6, rng)
    with pytest.raises(ValueError, match=r"s_eff.*ket 0"):
        cas_small.trans_rdm12_rows(bra, [ket])
    # a core orbital exchanged with a virtual: s_cc exactly singular
    n, ncore, ncas, nelecas = 7, 2, 3, (2, 1)
    bra = random_state(n, ncore, ncas, nelecas, rng)
    perm = list(range(n))
    perm[1], perm[6] = perm[6], perm[1]
    ket = random_state(n, ncore, ncas, nelecas, rng, U=bra.U[:, perm])
    with pytest.raises(ValueError, match="s_cc"):
        cas_small.pair_intermediates(bra, ket)
    with pytest.raises(ValueError, match="differ"):
        cas_small.pair_intermediates(bra, random_state(n, 1, ncas, (3, 2), rng))


# ---- the CASCI driver ---------------------------------------------------------------------------------------------
def chain(d, natm=6):
    from evcont_amd.hchain import hydrogen_chain
    return hydrogen_chain(natm, d, need_grad=False)


def oao_integrals(mol):
    from oracle.evcont_oracle import integrals_oao
    return integrals_oao(mol)


def test_casci_with_every_orbital_active_is_fci():
    from evcont_amd.electron_integral_utils import get_basis
    mol = chain(1.8)
    st = cas_small.casci(mol, 6, 6, _HOST)
    assert (st.ncore, st.ncas, st.nelecas) == (0, 6, (3, 3))
    assert np.abs(st.U.T @ st.U - np.eye(6)).max() <= 1e-12
    h1, h2 = oao_integrals(mol)
    e, _ = _HOST.kernel(h1, h2, 6, (3, 3))
    assert abs(st.e_tot - (e + mol.enuc)) <= 1e-10


@pytest.mark.parametrize("ncas,nact", [(2, 2), (4, 4)])
def test_casci_energy_from_the_diagonal_pair(ncas, nact):
    mol = chain(1.8)
    st = cas_small.casci(mol, ncas, nact, _HOST)
    assert st.ncore == (6 - nact) // 2
    ov, dm1, dm2 = cas_small.trans_rdm12_rows(st, [st])
    h1, h2 = oao_integrals(mol)
    e = float(np.sum(h1 * dm1[0].T) + 0.5 * np.sum(h2 * dm2[0]) + mol.enuc)
    assert abs(ov[0] - 1.0) <= 1e-12 and abs(e - st.e_tot) <= 1e-10


def test_casci_refuses_impossible_active_spaces():
    mol = chain(1.8)
    for ncas, nact in ((4, 3), (4, 8), (7, 6), (1, 4)):
        with pytest.raises(ValueError, match="casci"):
            cas_small.casci(mol, ncas, nact, _HOST)


@functools.lru_cache(maxsize=None)
def host_container():
    from evcont_amd.CASCI_EVCont import CAS_EVCont_obj
    cont = CAS_EVCont_obj(4, 4, cisolver=SmallFCI())
    mols = [chain(d) for d in (1.6, 1.8, 2.1)]
    for m in mols:
        cont.append_to_rdms(m)
    return cont, mols


def test_container_with_the_host_solver():
    cont, mols = host_container()
    assert cont.ntrain == 3 and len(cont.cascis) == 3 and len(cont.ens) == 3
    assert all(isinstance(s, CASState) for s in cont.cascis)
    assert np.array_equal(cont.overlap, cont.overlap.T) and np.abs(np.diag(cont.overlap) - 1.0).max() <= 1e-12
    assert cont.one_rdm.shape == (3, 3, 6, 6) and cont.two_rdm.shape == (3, 3, 6, 6, 6, 6)
    want = oracle_rows(cont.cascis[2], cont.cascis)
    assert worst((cont.overlap[2], cont.one_rdm[2], cont.two_rdm[2]), want) <= 1e-12
    pruned = copy.deepcopy(cont)
    pruned.prune_datapoints([0, 2])
    assert pruned.ntrain == 2 and [s.e_tot for s in pruned.cascis] == [cont.ens[0], cont.ens[2]]
    assert pruned.ens == [cont.ens[0], cont.ens[2]] and cont.ntrain == 3


def test_a_refused_pair_leaves_the_container_as_it_was(monkeypatch):
    from evcont_amd.CASCI_EVCont import CAS_EVCont_obj
    cont = CAS_EVCont_obj(4, 4, cisolver=SmallFCI())
    cont.append_to_rdms(chain(1.8))

    def refuse(*a, **k):
        raise ValueError("cas_small: s_eff of the pair (bra, ket 0) is ill-conditioned")

    monkeypatch.setattr(cas_small, "trans_rdm12_rows", refuse)
    with pytest.raises(ValueError, match="s_eff"):
        cont.append_to_rdms(chain(1.9))
    assert cont.ntrain == 1 and len(cont.cascis) == 1 and len(cont.ens) == 1
    monkeypatch.undo()
    cont.append_to_rdms(chain(1.9))
    assert cont.ntrain == 2 and len(cont.cascis) == 2 and len(cont.ens) == 2


def test_container_without_a_solver_is_unchanged():
    from evcont_amd.CASCI_EVCont import CAS_EVCont_obj
    with pytest.raises(ImportError):
        CAS_EVCont_obj(4, 4).append_to_rdms(chain(1.8))
    with pytest.raises(ImportError, match="pair_rdm_fun"):
        CAS_EVCont_obj(4, 4, casci_solver=object).append_to_rdms(chain(1.8))


def test_continuation_energy_at_the_training_geometries():
    from oracle.evcont_oracle import approximate_ground_state
    cont, mols = host_container()
    for i, mol in enumerate(mols):
        h1, h2 = oao_integrals(mol)
        e, _ = approximate_ground_state(h1, h2, cont.one_rdm, cont.two_rdm, cont.overlap)
        print(f"cas continuation at geometry {i}: E = {e + mol.enuc:.12f}  CASCI = {cont.ens[i]:.12f}")
        assert e + mol.enuc <= cont.ens[i] + 1e-10
    h1, h2 = oao_integrals(mols[0])
    e, _ = approximate_ground_state(h1, h2, cont.one_rdm[:1, :1], cont.two_rdm[:1, :1], cont.overlap[:1, :1])
    assert abs(e + mols[0].enuc - cont.ens[0]) <= 1e-10
