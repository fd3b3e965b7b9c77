"""CPU tests of several CASCI roots per geometry: ``cas_small.casci_roots``, the block statement
``cas_small.trans_rdm12_block`` against the embedding oracle of tests/cas_reference.py, and ``CAS_EVCont_obj`` with
``nroots`` / ``roots_train``."""
import copy
import functools

import numpy as np
import pytest

from evcont_amd import cas_small
from evcont_amd.CASCI_EVCont import CAS_EVCont_obj
from evcont_amd.fci_small import SmallFCI
from cas_reference import oracle_rows, random_state


def chain(d, natm=6):
    from evcont_amd.hchain import hydrogen_chain
    return hydrogen_chain(natm, d, need_grad=False)


def oao_integrals(mol):
    from oracle.evcont_oracle import integrals_oao
    return integrals_oao(mol)


def worst(got, want):
    return max(float(np.abs(np.asarray(g) - np.asarray(w)).max()) for g, w in zip(got, want))


def oracle_block(bras, kets):
    rows = [oracle_rows(b, kets) for b in bras]
    return tuple(np.stack([r[i] for r in rows]) for i in range(3))


@functools.lru_cache(maxsize=None)
def h6_roots(d, nroots=3):
    return tuple(cas_small.casci_roots(chain(d), 4, 4, SmallFCI(spin_penalty=0.2), nroots))


def test_casci_roots_share_orbitals_and_are_spin_pure():
    roots = h6_roots(1.8)
    assert len(roots) == 3 and all(s.U is roots[0].U for s in roots)
    assert all((s.ncore, s.ncas, s.nelecas) == (1, 4, (2, 2)) for s in roots)
    c = np.stack([s.ci.reshape(-1) for s in roots])
    assert np.abs(c @ c.T - np.eye(3)).max() <= 1e-12
    e = [s.e_tot for s in roots]
    assert e == sorted(e)
    ground = cas_small.casci(chain(1.8), 4, 4, SmallFCI(spin_penalty=0.2))
    assert abs(ground.e_tot - e[0]) <= 1e-10
    assert min(np.abs(ground.ci - roots[0].ci).max(), np.abs(ground.ci + roots[0].ci).max()) <= 1e-10
    assert np.array_equal(ground.U, roots[0].U)
    solver = SmallFCI()
    ss = [solver.spin_square(s.ci, 4, (2, 2))[0] for s in roots]
    print(f"H6 CAS(4,4) roots at 1.8: E = {e}, <S^2> = {ss}, gaps {e[1] - e[0]:.3f} {e[2] - e[1]:.3f}")
    assert max(abs(x) for x in ss) <= 1e-8


def test_casci_is_the_first_of_one_root():
    mol = chain(1.7)
    one, = cas_small.casci_roots(mol, 4, 4, SmallFCI(), 1)
    ground = cas_small.casci(mol, 4, 4, SmallFCI())
    assert one.e_tot == ground.e_tot and np.array_equal(one.ci, ground.ci) and np.array_equal(one.U, ground.U)
    with pytest.raises(ValueError, match="nroots"):
        cas_small.casci_roots(mol, 4, 4, SmallFCI(), 0)


def test_block_against_the_embedding_oracle_h6():
    states = [s for d in (1.6, 1.8, 2.0) for s in h6_roots(d)]
    assert len(states) == 9
    for g in range(3):
        bras = states[3 * g:3 * g + 3]
        got = cas_small.trans_rdm12_block(bras, states)
        assert got[0].shape == (3, 9) and got[1].shape == (3, 9, 6, 6) and got[2].shape == (3, 9) + (6,) * 4
        err = worst(got, oracle_block(bras, states))
        print(f"cas block H6 geometry {g}: worst |d| = {err:.2e}")
        assert err <= 1e-13
        # ... and it is the stack of the single-bra statement
        for r, bra in enumerate(bras):
            rows = cas_small.trans_rdm12_rows(bra, states)
            assert worst([x[r] for x in got], rows) <= 1e-13


def random_geometries(seed=21, n=7, ncore=2, ncas=3, nelecas=(2, 1), core=True):
    """Two "geometries" of two roots each: random orbitals near each other, shared per geometry."""
    from cas_reference import near_rotation, random_orthogonal
    rng = np.random.default_rng(seed)
    nc = ncore if core else 0
    U0 = random_orthogonal(n, rng)
    U1 = near_rotation(U0, rng)
    return [random_state(n, nc, ncas, nelecas, rng, U=U) for U in (U0, U0, U1, U1)]


@pytest.mark.parametrize("core", [True, False])
def test_block_on_a_shape_with_core_and_virtuals(core):
    states = random_geometries(core=core)
    for bras in (states[:2], states[2:]):
        got = cas_small.trans_rdm12_block(bras, states)
        err = worst(got, oracle_block(bras, states))
        print(f"cas block random shape core={core}: worst |d| = {err:.2e}")
        assert err <= 1e-13
    # an equal array counts as shared orbitals, the same object or not
    twin = copy.copy(states[1])
    twin.U = states[0].U.copy()
    assert worst(cas_small.trans_rdm12_block([states[0], twin], states),
                 cas_small.trans_rdm12_block(states[:2], states)) == 0.0
    with pytest.raises(ValueError, match="orbitals"):
        cas_small.trans_rdm12_block([states[0], states[2]], states)


def test_block_forms_the_intermediates_once_per_geometry(monkeypatch):
    states = [s for d in (1.6, 1.8) for s in h6_roots(d)]
    calls = []
    real = cas_small.pair_intermediates

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(cas_small, "pair_intermediates", counted)
    rotations = []

    class Counting(SmallFCI):
        def transform_ci(self, ci, nelec, u):
            rotations.append(1)
            return cas_small.fci_small.transform_ci(ci, nelec, u)

    cas_small.trans_rdm12_block(states[3:], states, Counting())
    assert len(calls) == 2 and len(rotations) == 6


# ---- the container -------------------------------------------------------------------------------------------------
def subspace(cont, mol):
    """Eigenvalues of the continuation Hamiltonian of the container's arrays at ``mol``, with the nuclear repulsion."""
    from scipy.linalg import eigh
    h1, h2 = oao_integrals(mol)
    H = np.tensordot(cont.one_rdm, h1, axes=2) + 0.5 * np.tensordot(cont.two_rdm, h2, axes=4)
    H = 0.5 * (H + H.T)
    return eigh(H, cont.overlap, eigvals_only=True) + mol.enuc


def test_one_geometry_three_roots_known_answer():
    mol = chain(1.8)
    cont = CAS_EVCont_obj(4, 4, cisolver=SmallFCI(spin_penalty=0.2), nroots=3)
    cont.append_to_rdms(mol)
    assert cont.ntrain == 3 and cont.mol_index == [0, 0, 0] and len(cont.cascis) == 3
    assert np.abs(cont.overlap - np.eye(3)).max() <= 1e-12
    # a frozen core shared by the three states: <a|H|b> = delta_ab E_a, core terms of the S = 0 pairs included
    h1, h2 = oao_integrals(mol)
    H = np.tensordot(cont.one_rdm, h1, axes=2) + 0.5 * np.tensordot(cont.two_rdm, h2, axes=4) + mol.enuc * cont.overlap
    assert np.abs(H - np.diag(cont.ens)).max() <= 1e-10
    assert np.abs(subspace(cont, mol) - np.asarray(cont.ens)).max() <= 1e-10


def test_invariance_against_the_fci_container():
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    from evcont_amd.hchain import hydrogen_chain
    cas = CAS_EVCont_obj(4, 4, cisolver=SmallFCI(), nroots=2)
    fci = FCI_EVCont_obj(cisolver=SmallFCI(), cibasis="canonical", nroots=2)
    for d in (1.6, 1.8, 2.0):
        mol = hydrogen_chain(4, d, need_grad=False)
        cas.append_to_rdms(mol)
        # FCI_EVCont_obj.append_to_rdms transforms its integrals on the device; without one, its two roots are solved
        # here in the OAO basis (the same span as the canonical solve rotated there) and appended root by root as it
        # does.  tests/test_gpu_cas_roots.py repeats this test through append_to_rdms itself.
        h1, h2 = oao_integrals(mol)
        es, vecs = SmallFCI().kernel(h1, h2, 4, mol.nelec, nroots=2)
        mindex = 0 if not fci.mol_index else max(fci.mol_index) + 1
        for e, v in zip(es, vecs):
            fci._append_root(v, e + mol.enuc, mindex, 4, mol.nelec)
    assert cas.cascis[0].ncore == 0 and cas.ntrain == fci.ntrain == 6 and cas.mol_index == fci.mol_index
    for d in (1.7, 1.9):
        mol = hydrogen_chain(4, d, need_grad=False)
        a, b = subspace(cas, mol)[:2], subspace(fci, mol)[:2]
        print(f"H4 at {d}: CAS container {a}, FCI container {b}")
        assert np.abs(a - b).max() <= 1e-10


def test_one_root_is_todays_container_bit_for_bit():
    mols = [chain(d) for d in (1.6, 1.8, 2.1)]
    cont = CAS_EVCont_obj(4, 4, cisolver=SmallFCI(), nroots=1)
    for m in mols:
        cont.append_to_rdms(m)
    from evcont_amd.containers import grow_trdms
    states, arrays = [], (None, None, None)
    for m in mols:
        states.append(cas_small.casci(m, 4, 4, SmallFCI()))
        arrays = grow_trdms(*arrays, *cas_small.trans_rdm12_rows(states[-1], states, SmallFCI()))
    assert np.array_equal(cont.overlap, arrays[0]) and np.array_equal(cont.one_rdm, arrays[1])
    assert np.array_equal(cont.two_rdm, arrays[2])
    assert cont.ens == [s.e_tot for s in states] and cont.mol_index == [0, 1, 2]


def test_roots_train_keeps_the_listed_roots():
    cont = CAS_EVCont_obj(4, 4, cisolver=SmallFCI(spin_penalty=0.2), nroots=3, roots_train=[0, 2])
    for d in (1.6, 1.8):
        cont.append_to_rdms(chain(d))
    assert cont.ntrain == 4 and cont.mol_index == [0, 0, 1, 1]
    want = [h6_roots(d)[k].e_tot for d in (1.6, 1.8) for k in (0, 2)]
    assert np.abs(np.asarray(cont.ens) - want).max() <= 1e-10
    assert np.array_equal(cont.overlap, cont.overlap.T)
    assert worst((cont.overlap[3], cont.one_rdm[3], cont.two_rdm[3]), oracle_rows(cont.cascis[3], cont.cascis)) <= 1e-12
    cont.prune_datapoints([0, 1, 3])
    assert cont.ntrain == 3 and cont.mol_index == [0, 0, 1] and len(cont.cascis) == 3 and len(cont.ens) == 3


def test_a_refused_block_leaves_the_container_as_it_was(monkeypatch):
    cont = CAS_EVCont_obj(4, 4, cisolver=SmallFCI(), nroots=2)
    cont.append_to_rdms(chain(1.8))

    def refuse(*a, **k):
        raise ValueError("cas_small: s_eff of the pair (bras, ket 0) is ill-conditioned")

    monkeypatch.setattr(cas_small, "trans_rdm12_block", refuse)
    with pytest.raises(ValueError, match="s_eff"):
        cont.append_to_rdms(chain(1.9))
    assert cont.ntrain == 2 and len(cont.cascis) == 2 and len(cont.ens) == 2 and cont.mol_index == [0, 0]


def test_the_third_party_route_is_ground_state_only():
    with pytest.raises(NotImplementedError):
        CAS_EVCont_obj(4, 4, casci_solver=object, pair_rdm_fun=lambda a, b: None, nroots=2).append_to_rdms(chain(1.8))
