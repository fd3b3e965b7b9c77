"""The batched subspace solve (``evc_subspace_solve_batch`` behind ``active_learning.subspace_energies`` /
``subset_energies``) on every route the active-learning loop takes: both kernels and the LDS / global-memory forms of the
large one inside a batch, the few-roots boundary, shared against per-problem overlap matrices, one problem and more
problems than compute units, the workspace chunking of the wrapper, the eigenvectors, the loop's own leave-one-out
shapes and a training set whose overlap matrix approaches singularity.

Reference: ``scipy.linalg.eigh(H[g], S[g], lower=True)`` in FP64 on the host, per problem; every problem of every call is
compared.  Problems are built as in tests/test_gpu_eigensolvers.py (``H = L C L^T``, ``S = L L^T``, ``C`` with a chosen
spectrum), the upper triangles of what is uploaded are NaN (the entry point reads lower triangles, as scipy does with
``lower=True``: a kernel that consumes an upper-triangle element returns NaN and fails).

Tolerances (those of ``test_subspace_spectra``): eigenvalues ``1e-10 max(1, max|w|)``, ``c S c^T = 1`` to 1e-10, residual
``max|H c - E S c| < 1e-9 max(1, max|H|)``, the lowest vector of a non-degenerate problem equal to scipy's up to sign to
1e-8; "bit for bit" is ``torch.equal``.  The k = 6 tier of ``test_converging_training_set`` replaces the factor 1e-10 by
``cond(S) 2^-52`` (the first-order bound of a Cholesky reduction to standard form, constant 1) and scales the vector
tolerances by the same ratio.  Each test prints its largest error / tolerance ratio; a failing assertion carries its own."""
import functools
import os

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from evcont_amd import _lib
from test_gpu_eigensolvers import spectrum, with_spectrum

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ("random", "degenerate", "triple", "cluster1e-6", "cluster1e-10")
SENTINEL = -3.0e200
EIG_TOL, ORTH_TOL, RES_TOL, VEC_TOL = 1e-10, 1e-10, 1e-9, 1e-8


# ------------------------------------------------------------------------------------------------ problems
class Problems:
    """count problems of one size with their scipy solutions.  S is (count,T,T) or, shared, (T,T)."""

    def __init__(self, H, S, shift, kinds):
        self.H, self.S, self.shift, self.kinds = H, S, shift, kinds
        self.count, self.T = H.shape[0], H.shape[1]
        self.shared = S.ndim == 2
        self.w = np.empty((self.count, self.T))
        self.v = np.empty((self.count, self.T, self.T))        # v[g][:, k]: scipy's k-th vector
        for g in range(self.count):
            self.w[g], self.v[g] = sla.eigh(H[g], self.Sg(g), lower=True)

    def Sg(self, g):
        return self.S if self.shared else self.S[g]

    def head(self, count):
        p = object.__new__(Problems)
        p.H, p.S, p.shift, p.kinds = self.H[:count], self.S if self.shared else self.S[:count], self.shift[:count], \
            self.kinds[:count]
        p.count, p.T, p.shared, p.w, p.v = count, self.T, self.shared, self.w[:count], self.v[:count]
        return p

    def one(self, g):
        p = object.__new__(Problems)
        p.H, p.S, p.shift, p.kinds = self.H[g:g + 1], self.S if self.shared else self.S[g:g + 1], \
            self.shift[g:g + 1], self.kinds[g:g + 1]
        p.count, p.T, p.shared, p.w, p.v = 1, self.T, self.shared, self.w[g:g + 1], self.v[g:g + 1]
        return p


def overlap_well_conditioned(T, rng):
    A = rng.standard_normal((T, T))
    return A @ A.T / T + np.eye(T)


def build(T, count, seed, shared=False, kinds=KINDS, overlap=overlap_well_conditioned):
    """Problem g has the spectrum kinds[g % len(kinds)] - 2 (indefinite, like an energy spectrum)."""
    rng = np.random.default_rng(seed)
    S_shared = overlap(T, rng) if shared else None
    H, S, names = [], [], []
    for g in range(count):
        kind = kinds[g % len(kinds)]
        Sg = S_shared if shared else overlap(T, rng)
        L = np.linalg.cholesky(Sg)
        vals = spectrum(kind, T, rng) - 2.0
        while kind == "random" and T > 1 and vals[1] - vals[0] < 1e-3:    # "non-degenerate" below: lowest gap >= 1e-3
            vals = spectrum(kind, T, rng) - 2.0
        Hg = L @ with_spectrum(vals, rng) @ L.T
        H.append(0.5 * (Hg + Hg.T))
        S.append(Sg)
        names.append(kind)
    return Problems(np.stack(H), S_shared if shared else np.stack(S), rng.standard_normal(count), names)


@functools.lru_cache(maxsize=None)
def grid_problems(T):
    return build(T, 5, 3000 + T)


@functools.lru_cache(maxsize=None)
def many_problems(T):
    return build(T, 257, 4000 + T)


def upload(a):
    """Device copy with the strict upper triangle(s) NaN."""
    a = np.array(a, dtype=np.float64, copy=True)
    iu = np.triu_indices(a.shape[-1], 1)
    a[..., iu[0], iu[1]] = np.nan
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_inputs(P):
    return upload(P.H), upload(P.S), torch.from_numpy(np.ascontiguousarray(P.shift)).to(DEV)


# ------------------------------------------------------------------------------------------------ checks (host)
def check_values(e, P, nroots, shifted, what, factor=EIG_TOL):
    """e (count, nroots) against scipy; returns the largest error / tolerance."""
    assert e.shape == (P.count, nroots), (what, e.shape)
    worst = 0.0
    for g in range(P.count):
        ref = P.w[g, :nroots] + (P.shift[g] if shifted else 0.0)
        tol = factor * max(1.0, np.abs(P.w[g]).max())
        err = np.abs(e[g] - ref).max()
        worst = max(worst, err / tol)
        assert err <= tol, (what, g, P.kinds[g], err, tol)     # (NaN: fails)
    return worst


def check_vectors(vec, e, P, nroots, shifted, what, scale=1.0, lowest=True):
    """vec (count, nroots, T): S-orthonormal, each row an eigenvector of its eigenvalue, the lowest one scipy's where the
    problem is non-degenerate.  Returns the largest error / tolerance of (orthonormality, residual, lowest vector)."""
    assert vec.shape == (P.count, nroots, P.T), (what, vec.shape)
    worst = [0.0, 0.0, 0.0]
    for g in range(P.count):
        il = np.tril_indices(P.T, -1)
        H, S = np.array(P.H[g]), np.array(P.Sg(g))
        H[il[1], il[0]] = H[il]            # symmetrised from the lower triangles
        S[il[1], il[0]] = S[il]
        c = vec[g]
        E = e[g] - (P.shift[g] if shifted else 0.0)
        orth = np.abs(c @ S @ c.T - np.eye(nroots)).max()
        res = np.abs(c @ H - E[:, None] * (c @ S)).max()
        res_tol = RES_TOL * scale * max(1.0, np.abs(H).max())
        worst[0] = max(worst[0], orth / (ORTH_TOL * scale))
        worst[1] = max(worst[1], res / res_tol)
        assert orth < ORTH_TOL * scale, (what, g, P.kinds[g], "orthonormality", orth)
        assert res < res_tol, (what, g, P.kinds[g], "residual", res, res_tol)
        if lowest and (P.kinds[g] == "random" or P.T == 1):
            v0 = P.v[g][:, 0]
            dv = min(np.abs(c[0] - v0).max(), np.abs(c[0] + v0).max())
            worst[2] = max(worst[2], dv / VEC_TOL)
            assert dv < VEC_TOL, (what, g, "lowest vector", dv)
    return worst


def report(tag, **worst):
    print(f"[subspace-batch] {tag}: largest error / tolerance " + ", ".join(f"{k}={v:.3g}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ routes
def ws_bytes(T, count=1):
    return int(_lib.load().evc_subspace_solve_ws_bytes(T, count))


def fits_lds(T):
    """Whether the large kernel keeps its matrix in LDS: its scratch then holds three Tp x Tp matrices and nothing else
    (``subspace_big_scratch_doubles``)."""
    Tp = (T + 15) & ~15
    return ws_bytes(T) == 3 * Tp * Tp * 8


def expected_route(T, nroots):
    few_on = int(os.environ.get("EVC_SUBSPACE_FEW", "1")) != 0
    fast = int(os.environ.get("EVC_EIGH_F32", "2")) != 0       # (the small kernel's few-roots route needs the fast base)
    if T <= 32:
        return "subspace_kernel few=%d" % int(few_on and fast and nroots <= 4 and T >= 2)
    if fits_lds(T):
        return "subspace_big_kernel<1> few=%d" % int(few_on and nroots <= 4)
    return "subspace_big_kernel<0> few=0"


def route():
    return _lib.load().evc_profile_kernel(_lib.PROF_STAGES["subspace"]).decode()


def solve(Hd, Sd, shift_d, nroots, **kw):
    from evcont_amd.active_learning import subspace_energies
    e, vec = subspace_energies(Hd, Sd, shift_d, nroots=nroots, return_vectors=True, **kw)
    return e, vec


def solve_direct(Hd, Sd, shift_d, nroots, chunk=None):
    """The entry point itself on sentinel-filled outputs (the wrapper allocates its own): (evals (count,T),
    evecs (count,T,T)), every element the call did not write still SENTINEL."""
    from evcont_amd.evaluator import _stream_ptr
    lib = _lib.load()
    count, T = int(Hd.shape[0]), int(Hd.shape[1])
    shared = Sd.dim() == 2
    evals = torch.full((count, T), SENTINEL, dtype=torch.float64, device=Hd.device)
    evecs = torch.full((count, T, T), SENTINEL, dtype=torch.float64, device=Hd.device)
    per = ws_bytes(T)
    chunk = count if chunk is None else chunk
    ws = torch.empty(per * chunk, dtype=torch.uint8, device=Hd.device) if per else None
    for c0 in range(0, count, chunk):
        c1 = min(count, c0 + chunk)
        _lib.check(lib.evc_subspace_solve_batch(
            Hd[c0:c1].data_ptr(), Sd.data_ptr() if shared else Sd[c0:c1].data_ptr(), 0 if shared else T * T, T, c1 - c0,
            nroots, shift_d[c0:c1].data_ptr() if shift_d is not None else None, evals[c0:c1].data_ptr(),
            evecs[c0:c1].data_ptr(), ws.data_ptr() if ws is not None else None, per * (c1 - c0),
            _stream_ptr(Hd.device)), "evc_subspace_solve_batch")
    torch.cuda.synchronize()
    return evals, evecs


def assert_untouched_beyond(evals, evecs, nroots, what):
    assert bool((evals[:, :nroots] != SENTINEL).all()) and bool((evecs[:, :nroots] != SENTINEL).all()), what
    assert bool((evals[:, nroots:] == SENTINEL).all()), (what, "evals past nroots written")
    assert bool((evecs[:, nroots:] == SENTINEL).all()), (what, "evecs rows past nroots written")


# ------------------------------------------------------------------------------------------------ (a) + (e)
GRID_T = [1, 2, 3, 8, 9, 16, 17, 24, 25, 31, 32, 33, 34, 47, 64, 65, 100, 128, 129, 160]


def test_grid_straddles_the_lds_boundary():
    """T = 128 | 129 of the grid is the switch of the large kernel from LDS to global memory (``big_fits_lds``)."""
    switch = [T for T in range(33, 513) if fits_lds(T) != fits_lds(T - 1) and T > 33]
    assert switch == [129], switch
    assert 128 in GRID_T and 129 in GRID_T


@pytest.mark.parametrize("T", GRID_T)
def test_size_and_route_grid(T):
    """(a), (e): five problems of mixed spectra per call, per-problem S, with and without e_shift, nroots in
    {1, 4, 5, T}: the route the library reports, every eigenvalue, every vector."""
    P = grid_problems(T)
    Hd, Sd, shd = device_inputs(P)
    wv, wo, wr, wl = 0.0, 0.0, 0.0, 0.0
    for nroots in sorted({min(n, T) for n in (1, 4, 5, T)}):
        for shifted in (True, False):
            what = (T, nroots, shifted)
            e, vec = solve(Hd, Sd, shd if shifted else None, nroots)
            rec = route()
            e, vec = e.cpu().numpy(), vec.cpu().numpy()
            assert rec == expected_route(T, nroots), (what, rec, expected_route(T, nroots))
            wv = max(wv, check_values(e, P, nroots, shifted, what))
            o, r, l = check_vectors(vec, e, P, nroots, shifted, what)
            wo, wr, wl = max(wo, o), max(wr, r), max(wl, l)
    report(f"(a)/(e) T={T}", eigenvalues=wv, orthonormality=wo, residual=wr, lowest_vector=wl)


@pytest.mark.parametrize("T", [8, 33])
def test_rows_past_nroots_are_left_alone(T):
    """(e): the call writes the first nroots entries of each evals row and the first nroots rows of each evecs block
    (include/evcont_hip.h) and nothing else -- not the rest of the block, not the next problem's."""
    P = grid_problems(T)
    Hd, Sd, shd = device_inputs(P)
    evals, evecs = solve_direct(Hd, Sd, shd, 2)
    assert_untouched_beyond(evals, evecs, 2, T)
    e, vec = solve(Hd, Sd, shd, 2)
    assert torch.equal(evals[:, :2], e) and torch.equal(evecs[:, :2], vec)
    check_values(evals[:, :2].cpu().numpy(), P, 2, True, T)


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("T", [19, 33, 129])
def test_shared_overlap_equals_expanded(T):
    """(b): one S (T,T) with s_stride = 0 against the same S repeated per problem: bit for bit, and both scipy's."""
    P = build(T, 5, 5000 + T, shared=True)
    Hd, Sd, shd = device_inputs(P)
    Sx = Sd.unsqueeze(0).expand(P.count, T, T).contiguous()
    wv, wo, wr = 0.0, 0.0, 0.0
    for nroots in (1, 5):
        e0, v0 = solve(Hd, Sd, shd, nroots)
        e1, v1 = solve(Hd, Sx, shd, nroots)
        assert torch.equal(e0, e1) and torch.equal(v0, v1), (T, nroots)
        e, vec = e0.cpu().numpy(), v0.cpu().numpy()
        wv = max(wv, check_values(e, P, nroots, True, (T, nroots)))
        o, r, _ = check_vectors(vec, e, P, nroots, True, (T, nroots))
        wo, wr = max(wo, o), max(wr, r)
    report(f"(b) T={T}", eigenvalues=wv, orthonormality=wo, residual=wr)


# ------------------------------------------------------------------------------------------------ (c)
COUNTS = (1, 2, 17, 257)


@pytest.mark.parametrize("T", [5, 32, 33])
def test_count_edges(T):
    """(c): one problem, two, 17 (more workgroups than the card has XCDs: blocks 0, 8 and 16 share an L2) and 257 (more
    than it has compute units), per-problem S and shift; in the largest call problem g is bit for bit what it is when
    solved alone: no dependence on the block index or the neighbours."""
    full = many_problems(T)
    wv, wo, wr = 0.0, 0.0, 0.0
    for count in COUNTS:
        P = full.head(count)
        Hd, Sd, shd = device_inputs(P)
        for nroots in (1, 5):
            what = (T, count, nroots)
            e_d, vec_d = solve(Hd, Sd, shd, nroots)
            assert route() == expected_route(T, nroots), what
            e, vec = e_d.cpu().numpy(), vec_d.cpu().numpy()
            wv = max(wv, check_values(e, P, nroots, True, what))
            o, r, _ = check_vectors(vec, e, P, nroots, True, what)
            wo, wr = max(wo, o), max(wr, r)
            if count == 257:
                for g in (0, 1, 128, 255, 256):
                    e1, v1 = solve(Hd[g:g + 1], Sd[g:g + 1], shd[g:g + 1], nroots)
                    assert torch.equal(e1[0], e_d[g]) and torch.equal(v1[0], vec_d[g]), (what, g)
    report(f"(c) T={T}", eigenvalues=wv, orthonormality=wo, residual=wr)


@pytest.mark.parametrize("T", [33, 129])
def test_scratch_is_per_problem(T):
    """24 problems on the large kernel, in LDS (T = 33) and in global memory (T = 129).  Blocks b and b + 8 run on the same
    XCD and share its L2; up to eight blocks each have an L2 to themselves and never see one another's global stores
    within a launch, so a call of five or seven problems passes even when every block uses the SAME scratch (measured:
    ``a.scratch += g * a.sscratch`` removed changes no figure of the other tests of this file below count = 9)."""
    P = build(T, 24, 4500 + T)
    Hd, Sd, shd = device_inputs(P)
    wv, wo, wr = 0.0, 0.0, 0.0
    for nroots in (1, 5):
        e, vec = solve(Hd, Sd, shd, nroots)
        assert route() == expected_route(T, nroots), (T, nroots)
        e, vec = e.cpu().numpy(), vec.cpu().numpy()
        wv = max(wv, check_values(e, P, nroots, True, (T, nroots)))
        o, r, _ = check_vectors(vec, e, P, nroots, True, (T, nroots))
        wo, wr = max(wo, o), max(wr, r)
    report(f"(c) scratch T={T}", eigenvalues=wv, orthonormality=wo, residual=wr)


# ------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("T", [33, 65, 129])
def test_workspace_chunking(T):
    """(d): seven problems in chunks of 3 + 3 + 1 and of one (``max_ws_bytes``; also below one problem's workspace, which
    still solves one problem per launch), per-problem and shared S, with and without e_shift: bit for bit the unchunked
    call, scipy's values, and every output slot written by exactly the launch that owns it."""
    per = ws_bytes(T)
    assert per > 0
    nroots = 3
    wv, wo, wr = 0.0, 0.0, 0.0
    for shared in (False, True):
        P = build(T, 7, 6000 + T + (500 if shared else 0), shared=shared)
        Hd, Sd, shd = device_inputs(P)
        for shifted in (True, False):
            what = (T, shared, shifted)
            sh = shd if shifted else None
            e0, v0 = solve(Hd, Sd, sh, nroots)
            e, vec = e0.cpu().numpy(), v0.cpu().numpy()
            wv = max(wv, check_values(e, P, nroots, shifted, what))
            o, r, _ = check_vectors(vec, e, P, nroots, shifted, what)
            wo, wr = max(wo, o), max(wr, r)
            for max_ws in (3 * per, per, per // 2):
                e1, v1 = solve(Hd, Sd, sh, nroots, max_ws_bytes=max_ws)
                assert torch.equal(e0, e1) and torch.equal(v0, v1), (what, max_ws // per)
            for chunk in (3, 1):
                evals, evecs = solve_direct(Hd, Sd, sh, nroots, chunk=chunk)
                assert_untouched_beyond(evals, evecs, nroots, (what, chunk))
                assert torch.equal(evals[:, :nroots], e0) and torch.equal(evecs[:, :nroots], v0), (what, chunk)
    report(f"(d) T={T}", eigenvalues=wv, orthonormality=wo, residual=wr)


# ------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("T", [9, 33, 34])
def test_loop_subsets(T):
    """(f): ``subset_energies`` on the subsets the loop asks for -- the full set, every leave-one-out set, drop-last, a
    pair and a single state -- of one H (3,T,T) and one S (T,T).  T = 33: the full set on the large kernel, the 33
    leave-one-out sets on the small one; T = 34: both on the large one.  (Ascending ids: a sub-matrix's lower triangle
    comes from the lower triangle of H.)"""
    from evcont_amd.active_learning import subset_energies
    P = build(T, 3, 7000 + T, shared=True, kinds=("random", "degenerate", "cluster1e-6"))
    enuc = P.shift
    subsets = [list(range(T))] + [[i for i in range(T) if i != j] for j in range(T)] + [list(range(T - 1))] + \
        [[1, T - 2], [T // 2]]
    got = subset_energies(upload(P.H), upload(P.S), torch.from_numpy(enuc).to(DEV), subsets).cpu().numpy()
    assert got.shape == (3, len(subsets))
    worst = 0.0
    for k, ids in enumerate(subsets):
        ix = np.ix_(ids, ids)
        for b in range(3):
            w = sla.eigh(P.H[b][ix], P.S[ix])[0]
            tol = EIG_TOL * max(1.0, np.abs(w).max())
            err = abs(got[b, k] - (w[0] + enuc[b]))
            worst = max(worst, err / tol)
            assert err <= tol, (T, k, b, err, tol)
    report(f"(f) T={T}", eigenvalues=worst)


# ------------------------------------------------------------------------------------------------ (g)
@pytest.mark.parametrize("k", [4, 6])
@pytest.mark.parametrize("T", [8, 19, 32, 33, 65])
def test_converging_training_set(T, k):
    """(g): overlap matrices with eigenvalues logspace(-k, 0, T) -- a training set that converges.  k = 4: the tolerances
    of every other test.  k = 6: eigenvalues within cond(S) 2^-52 max(1, max|w|) of scipy's (first-order bound of the
    Cholesky reduction to standard form; scipy itself stays 50 to 100 times inside it on these inputs), the vector
    tolerances scaled by the same ratio cond(S) 2^-52 / 1e-10."""
    def graded(T, rng):
        return with_spectrum(np.logspace(-k, 0, T), rng)
    P = build(T, 5, 8000 + 10 * T + k, kinds=("random",), overlap=graded)
    Hd, Sd, shd = device_inputs(P)
    wv, wo, wr = 0.0, 0.0, 0.0
    for nroots in (1, min(5, T)):
        e, vec = solve(Hd, Sd, shd, nroots)
        assert route() == expected_route(T, nroots), (T, k, nroots)
        e, vec = e.cpu().numpy(), vec.cpu().numpy()
        for g in range(P.count):
            one = P.one(g)
            factor = EIG_TOL
            if k == 6:
                s = np.linalg.eigvalsh(P.S[g])
                factor = s[-1] / s[0] * 2.0 ** -52
            what = (T, k, nroots, g)
            wv = max(wv, check_values(e[g:g + 1], one, nroots, True, what, factor=factor))
            o, r, _ = check_vectors(vec[g:g + 1], e[g:g + 1], one, nroots, True, what, scale=factor / EIG_TOL,
                                    lowest=False)
            wo, wr = max(wo, o), max(wr, r)
    report(f"(g) T={T} k={k}", eigenvalues=wv, orthonormality=wo, residual=wr)
