"""Oracle for transition RDMs between CAS states in different orbital sets, built from ``fci_small`` alone: embed each CAS
vector in the full CI space of all N orbitals (full string = core bits | active string << ncore, sign +1: the core
orbitals come first, so no operator crosses another), rotate it into the OAO basis with ``transform_ci(full, nelec, U^T)``
and take ``SmallFCI.trans_rdm12`` there.  Shares no code with ``cas_small.pair_intermediates``.  Cost grows like the full
CI space, so N <= 8 or so."""
import numpy as np
from scipy.linalg import expm

from evcont_amd.cas_small import CASState
from evcont_amd.fci_small import SmallFCI, _strings, transform_ci

_HOST = SmallFCI()


def embed(state):
    """The state as an (na_full, nb_full) vector over the strings of all N orbitals, still in its own orbitals."""
    n, nc, ncas = state.U.shape[0], state.ncore, state.ncas
    nelec = (state.nelecas[0] + nc, state.nelecas[1] + nc)
    core = (1 << nc) - 1
    full = np.zeros((len(_strings(n, nelec[0])), len(_strings(n, nelec[1]))))
    ia = [_strings(n, nelec[0]).index(core | (s << nc)) for s in _strings(ncas, state.nelecas[0])]
    ib = [_strings(n, nelec[1]).index(core | (s << nc)) for s in _strings(ncas, state.nelecas[1])]
    full[np.ix_(ia, ib)] = np.asarray(state.ci).reshape(len(ia), len(ib))
    return full, nelec


def in_oao(state):
    full, nelec = embed(state)
    return transform_ci(full, nelec, np.asarray(state.U).T), nelec


def oracle_rows(bra, kets):
    """(ovlp (T,), dm1 (T,N,N), dm2 (T,N,N,N,N)) of one bra against the kets."""
    n = bra.U.shape[0]
    cb, nelec = in_oao(bra)
    T = len(kets)
    ovlp, dm1, dm2 = np.empty(T), np.empty((T, n, n)), np.empty((T, n, n, n, n))
    for i, ket in enumerate(kets):
        ck, _ = in_oao(ket)
        ovlp[i] = float(np.vdot(cb, ck))
        dm1[i], dm2[i] = _HOST.trans_rdm12(cb, ck, n, nelec)
    return ovlp, dm1, dm2


def random_orthogonal(n, rng):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def random_ci(ncas, nelecas, rng):
    c = rng.standard_normal((len(_strings(ncas, nelecas[0])), len(_strings(ncas, nelecas[1]))))
    return c / np.linalg.norm(c)


def random_state(n, ncore, ncas, nelecas, rng, U=None):
    return CASState(U=random_orthogonal(n, rng) if U is None else U, ncore=ncore, ncas=ncas, nelecas=tuple(nelecas),
                    ci=random_ci(ncas, nelecas, rng))


def near_rotation(U, rng, scale=0.1):
    """U expm(scale K), K a random antisymmetric matrix."""
    k = rng.standard_normal(U.shape)
    return U @ expm(scale * (k - k.T))


def sweep_pair(cond, rng, n=7, ncore=2, ncas=3, nelecas=(2, 1), core=False):
    """The conditioning sweep of DESIGN.md 8.1.5: Uk = Ua R with R a 2 x 2 rotation of one ket orbital (the last active
    one, or the last core one with ``core``) towards the first virtual, by the angle whose cosine is 1 / cond: the
    overlap block concerned then has singular values 1 ... 1 / cond."""
    Ua = random_orthogonal(n, rng)
    i, v = (ncore - 1 if core else ncore + ncas - 1), ncore + ncas
    c = 1.0 / cond
    s = np.sqrt(1.0 - c * c)
    R = np.eye(n)
    R[i, i], R[v, v], R[i, v], R[v, i] = c, c, -s, s
    bra = random_state(n, ncore, ncas, nelecas, rng, U=Ua)
    ket = random_state(n, ncore, ncas, nelecas, rng, U=Ua @ R)
    return bra, ket
