"""GPU tests of the device eigensolver of ``DeviceFCI(eigensolver="davidson")``: the vector entry points of
csrc/fci_solve.hip called directly on poisoned, fenced buffers, then the solver against the host.

Bounds of the random-data comparisons are derived, not chosen.  The references are formed in extended precision
(np.longdouble), so that the whole allowance belongs to the device:

* dots.  A sum of ``dim`` products in any order obeys |err| <= dim * u * sum |x_k y_k| <= dim * u * ||x|| ||y||, u = 2^-53.
* combine.  Out[e] = beta Out[e] + sum_j c_j V_j[e] is a sum of m + 1 terms, each product rounded once or fused:
  |err| <= (m + 2) * u * (|beta Out[e]| + sum_j |c_j V_j[e]|), element by element.
* correction.  x = sum_j y_j V_j and s = sum_j y_j W_j are m-term sums, r = s - theta x one more fused step:
  |err r[e]| <= E[e] = (m + 2) * u * (sum_j |y_j W_j[e]| + |theta| sum_j |y_j V_j[e]|); t = r / d with d = hdiag - theta
  rounded once and the quotient once: |err t[e]| <= (E[e] + 3 u |r[e]|) / |d[e]|; |r|^2 is a dim-term sum of squares of
  values off by E: |err| <= sum_e (2 |r[e]| E[e] + E[e]^2) + dim * u * sum_e r[e]^2 (terms of second order in u included).

With integer data of small entries every intermediate is an integer (or one correctly rounded division), so the results
are held to numpy bit for bit."""
import re

import numpy as np
import pytest
import torch

from evcont_amd.fci_davidson import DENOM_FLOOR, hdiag_numpy
from evcont_amd.fci_small import SmallFCI
from evcont_amd.fci_tables import packed_table
from evcont_amd.hchain import hydrogen_chain, s_gaussian_mol
from test_fci_davidson_host import RESTART_CASE, integer_integrals, oao_integrals
from test_fci_solve_closure import SOLVE_RECORDS
from test_gpu_fci_abi import Fenced, library
from test_hchain_physics import bent_chain

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
_HOST = SmallFCI()
DIMS = [4, 300, 4900, 63504]
COUNTS = [1, 3, 8, 11]


def solve_record():
    mod, lib, _ = library()
    return lib.evc_profile_kernel(mod.FCI_PROF_SOLVE).decode()


class VectorSet:
    """``count`` vectors of ``dim`` doubles at pitch ``ld`` in a fenced device buffer; the gaps between the rows hold the
    NaN poison.  The last row ends with its ``dim``-th element."""

    def __init__(self, dim, ld, count, dev, data=None):
        self.dim, self.ld, self.count = dim, ld, count
        self.n = (count - 1) * ld + dim
        self.f = Fenced(8 * self.n, dev)
        if data is not None:
            flat = np.full(self.n, np.nan)
            for i in range(count):
                flat[i * ld:i * ld + dim] = data[i]
            self.f.buf[self.f.off:self.f.off + 8 * self.n] = torch.from_numpy(flat.view(np.uint8)).to(dev)

    @property
    def ptr(self):
        return self.f.ptr

    def rows(self):
        """``(count, dim)`` values; asserts the fences and the gaps."""
        assert self.f.fences_intact()
        flat = self.f.doubles()
        pad = np.concatenate([flat, np.full(self.count * self.ld - self.n, np.nan)]).reshape(self.count, self.ld)
        assert np.isnan(pad[:, self.dim:]).all()
        return pad[:, :self.dim].copy()


class Vectors:
    """The entry points on fenced buffers for one ``dim``."""

    def __init__(self, dim):
        self.mod, self.lib, self.check = library()
        self.dev = torch.device("cuda:0")
        self.dim, self.ld = dim, dim + 5
        rows = max(256, (-(-dim // 256) + 63) // 64 * 64)
        self.nblk = -(-dim // rows)

    def up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)

    def dots(self, x, y):
        nx, ny = len(x), len(y)
        X, Y = VectorSet(self.dim, self.ld, nx, self.dev, x), VectorSet(self.dim, self.ld + 3, ny, self.dev, y)
        wsb = 8 * self.nblk * nx * ny                      # exactly what the call needs
        ws, out = Fenced(wsb, self.dev, front=False), Fenced(8 * nx * ny, self.dev)
        self.check(self.lib.evc_fci_dots(self.dim, X.ptr, X.ld, nx, Y.ptr, Y.ld, ny, out.ptr, ws.ptr, wsb, None),
                   "evc_fci_dots")
        torch.cuda.synchronize()
        assert ws.fences_intact() and out.fences_intact()
        rec = solve_record()
        assert re.fullmatch(SOLVE_RECORDS["evc_fci_dots"], rec), rec
        assert f"nx={nx} ny={ny} groups={-(-nx // 8)} blocks={self.nblk} " in rec, rec
        return out.doubles().reshape(nx, ny)

    def combine(self, v, coef, beta, out0):
        m, k = coef.shape
        V = VectorSet(self.dim, self.ld, max(m, 1), self.dev, v if m else None)
        O = VectorSet(self.dim, self.ld + 1, k, self.dev, out0)
        dcoef = self.up(np.pad(coef, ((0, 0), (0, 2)), constant_values=np.nan)) if m else None   # ldc = k + 2
        self.check(self.lib.evc_fci_combine(self.dim, V.ptr, V.ld, m, dcoef.data_ptr() if m else None, k + 2, k, beta,
                                            O.ptr, O.ld, None), "evc_fci_combine")
        torch.cuda.synchronize()
        rec = solve_record()
        assert re.fullmatch(SOLVE_RECORDS["evc_fci_combine"], rec), rec
        assert rec.endswith(f"m={m} k={k} groups={-(-k // 8)}"), rec
        V.rows()
        return O.rows()

    def correction(self, v, w, y, theta, hd):
        m, k = y.shape
        V, W = VectorSet(self.dim, self.ld, m, self.dev, v), VectorSet(self.dim, self.ld + 2, m, self.dev, w)
        T = VectorSet(self.dim, self.ld + 1, k, self.dev)
        wsb = 8 * self.nblk * k
        ws, rn = Fenced(wsb, self.dev, front=False), Fenced(8 * k, self.dev)
        dy, dth, dhd = self.up(y), self.up(theta), self.up(hd)
        self.check(self.lib.evc_fci_davidson_correction(self.dim, V.ptr, V.ld, W.ptr, W.ld, m, dy.data_ptr(), k,
                                                        dth.data_ptr(), k, dhd.data_ptr(), T.ptr, T.ld, rn.ptr, ws.ptr, wsb,
                                                        None), "evc_fci_davidson_correction")
        torch.cuda.synchronize()
        assert ws.fences_intact() and rn.fences_intact()
        rec = solve_record()
        assert re.fullmatch(SOLVE_RECORDS["evc_fci_davidson_correction"], rec), rec
        assert f"m={m} k={k} groups={-(-k // 8)} blocks={self.nblk} " in rec, rec
        return T.rows(), rn.doubles()


def integer_rows(rng, count, dim, top=3):
    return rng.integers(-top, top + 1, size=(count, dim)).astype(np.float64)


# ---- hdiag ---------------------------------------------------------------------------------------------------------
def device_hdiag(norb, nelec, h1, h2):
    mod, lib, check = library()
    dev = torch.device("cuda:0")
    ta, tb = packed_table(norb, nelec[0]), packed_table(norb, nelec[1])
    na, nb = ta.shape[0], tb.shape[0]
    dta, dtb = torch.from_numpy(ta).to(dev), torch.from_numpy(tb).to(dev)
    dh1 = torch.from_numpy(np.ascontiguousarray(h1, dtype=np.float64)).to(dev)
    dh2 = torch.from_numpy(np.ascontiguousarray(h2, dtype=np.float64).reshape(-1)).to(dev)
    wsb = lib.evc_fci_solve_workspace_bytes(norb, na, nb, 1)
    assert wsb > 0
    ws, out = Fenced(wsb, dev, front=False), Fenced(8 * na * nb, dev)
    check(lib.evc_fci_hdiag(norb, na, nb, dta.data_ptr(), dtb.data_ptr(), dh1.data_ptr(), dh2.data_ptr(), out.ptr, ws.ptr,
                            wsb, None), "evc_fci_hdiag")
    torch.cuda.synchronize()
    assert ws.fences_intact() and out.fences_intact()
    rec = solve_record()
    assert re.fullmatch(SOLVE_RECORDS["evc_fci_hdiag"], rec) and f"strings={na + nb} " in rec, rec
    return out.doubles().reshape(na, nb)


@pytest.mark.parametrize("norb,nelec", [(3, (2, 1)), (6, (3, 2)), (9, (4, 4))])
def test_hdiag_integer_inputs_bit_for_bit(norb, nelec):
    h1, h2 = integer_integrals(norb, seed=20 + norb)
    want = hdiag_numpy(h1, h2, norb, nelec)
    assert np.array_equal(want, np.rint(want)) and np.abs(want).max() < 2.0 ** 40
    got = device_hdiag(norb, nelec, h1, h2)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(got, device_hdiag(norb, nelec, h1, h2))


def test_hdiag_random_inputs():
    norb, nelec = 6, (3, 3)
    rng = np.random.default_rng(6)
    h1, h2 = rng.standard_normal((norb, norb)), rng.standard_normal((norb,) * 4)       # no symmetry at all
    got, want = device_hdiag(norb, nelec, h1, h2), hdiag_numpy(h1, h2, norb, nelec)
    _, _, na, nb = _HOST._ops(norb, nelec)
    k = 123
    e = np.zeros(na * nb)
    e[k] = 1.0
    assert abs(_HOST.contract(h1, h2, e.reshape(na, nb), norb, nelec).reshape(-1)[k] - want.reshape(-1)[k]) < 1e-12
    print(f"hdiag random (6,(3,3)): max|d|={np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() < 1e-12


# ---- dots ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_dots_against_numpy(dim):
    p = Vectors(dim)
    rng = np.random.default_rng(dim)
    worst = 0.0
    for n in COUNTS:
        ny = COUNTS[(COUNTS.index(n) + 1) % len(COUNTS)]             # 1 x 3, 3 x 8, 8 x 11, 11 x 1
        x, y = integer_rows(rng, n, dim), integer_rows(rng, ny, dim)
        assert np.array_equal(p.dots(x, y), x @ y.T)
        x, y = rng.standard_normal((n, dim)), rng.standard_normal((ny, dim))
        got = p.dots(x, y)
        ref = (x.astype(LD) @ y.astype(LD).T).astype(np.float64)
        bound = dim * U * np.linalg.norm(x, axis=1)[:, None] * np.linalg.norm(y, axis=1)[None, :]
        worst = max(worst, (np.abs(got - ref) / bound).max())
        assert (np.abs(got - ref) <= bound).all()
        assert np.array_equal(got, p.dots(x, y))                     # run to run
        if n == 11:                                                  # 11 rows = 8 + 3, bit for bit
            assert np.array_equal(got[:8], p.dots(x[:8], y)) and np.array_equal(got[8:], p.dots(x[8:], y))
        if n == 8:                                                   # and column by column
            assert np.array_equal(got[:, 4:5], p.dots(x, y[4:5]))
    x = rng.standard_normal((11, dim))
    g = p.dots(x, x)                                                 # a set against itself
    assert np.array_equal(g, g.T)
    print(f"dots dim={dim}: worst error / bound = {worst:.3f}")


# ---- combine -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_combine_against_numpy(dim):
    p = Vectors(dim)
    rng = np.random.default_rng(dim + 1)
    worst = 0.0
    for m in COUNTS:
        k = COUNTS[(COUNTS.index(m) + 2) % len(COUNTS)]              # 1 -> 8, 3 -> 11, 8 -> 1, 11 -> 3
        v, c, o = integer_rows(rng, m, dim), integer_rows(rng, m, k, top=4), integer_rows(rng, k, dim)
        assert np.array_equal(p.combine(v, c, 2.0, o), 2.0 * o + c.T @ v)
        assert np.array_equal(p.combine(v, c, 0.0, None), c.T @ v)   # beta = 0: the NaN in Out is not read
        v, c, o = rng.standard_normal((m, dim)), rng.standard_normal((m, k)), rng.standard_normal((k, dim))
        beta = -0.75
        got = p.combine(v, c, beta, o)
        ref = (beta * o.astype(LD) + c.astype(LD).T @ v.astype(LD)).astype(np.float64)
        bound = (m + 2) * U * (np.abs(beta * o) + np.abs(c).T @ np.abs(v))
        worst = max(worst, (np.abs(got - ref) / bound).max())
        assert (np.abs(got - ref) <= bound).all()
        assert np.array_equal(got, p.combine(v, c, beta, o))
    o = integer_rows(rng, 3, dim)
    assert np.array_equal(p.combine(None, np.zeros((0, 3)), 4.0, o), 4.0 * o)       # m = 0 scales
    print(f"combine dim={dim}: worst error / bound = {worst:.3f}")


def test_combine_refuses_aliasing_without_a_launch():
    p = Vectors(300)
    rng = np.random.default_rng(3)
    v = rng.standard_normal((4, 300))
    V = VectorSet(300, p.ld, 4, p.dev, v)
    dcoef = p.up(np.ones((3, 2)))
    p.dots(v, v)
    before = solve_record()
    rc = p.lib.evc_fci_combine(300, V.ptr, V.ld, 3, dcoef.data_ptr(), 2, 2, 0.0, V.ptr + 8 * 2 * V.ld, V.ld, None)
    assert rc != 0 and b"alias" in p.lib.evc_last_error()
    rc = p.lib.evc_fci_combine(300, V.ptr + 8 * V.ld, V.ld, 3, dcoef.data_ptr(), 2, 2, 0.0, V.ptr, V.ld, None)
    assert rc != 0 and b"alias" in p.lib.evc_last_error()            # Out before V, its second row inside V
    torch.cuda.synchronize()
    assert solve_record() == before                                  # nothing was launched, nothing recorded
    assert np.array_equal(V.rows(), v)
    O = VectorSet(300, p.ld, 2, p.dev)
    T = VectorSet(300, p.ld, 2, p.dev)
    rc = p.lib.evc_fci_davidson_correction(300, V.ptr, V.ld, V.ptr, V.ld, 4, dcoef.data_ptr(), 2, dcoef.data_ptr(), 2,
                                           O.ptr, V.ptr + 8 * 3 * V.ld, V.ld, T.ptr, T.ptr, 1 << 16, None)
    assert rc != 0 and b"alias" in p.lib.evc_last_error()
    assert p.lib.evc_fci_dots(300, V.ptr, 299, 1, V.ptr, 300, 1, O.ptr, T.ptr, 1 << 16, None) != 0     # ld < dim
    assert solve_record() == before


# ---- correction ----------------------------------------------------------------------------------------------------
def correction_reference(v, w, y, theta, hd):
    """(r, t, |r|^2) in extended precision, the denominator as the device forms it (one float64 subtraction)."""
    x = y.astype(LD).T @ v.astype(LD)
    r = y.astype(LD).T @ w.astype(LD) - theta.astype(LD)[:, None] * x
    d = hd[None, :] - theta[:, None]
    d = np.where(np.abs(d) < DENOM_FLOOR, np.where(d < 0.0, -DENOM_FLOOR, DENOM_FLOOR), d)
    return r, r / d.astype(LD), d


@pytest.mark.parametrize("dim", DIMS)
def test_correction_against_numpy(dim):
    p = Vectors(dim)
    rng = np.random.default_rng(dim + 2)
    worst_t = worst_n = 0.0
    for m in COUNTS:
        k = COUNTS[(COUNTS.index(m) + 1) % len(COUNTS)]
        v, w, y = integer_rows(rng, m, dim), integer_rows(rng, m, dim), integer_rows(rng, m, k, top=2)
        theta = rng.integers(-5, 6, size=k).astype(np.float64)
        hd = rng.integers(-7, 8, size=dim).astype(np.float64)
        hd[0] = theta[0]                                             # d = 0 counts as +1e-8
        hd[1] = theta[0] - 1e-9                                      # floored, sign kept
        hd[dim - 1] = theta[k - 1] + 1e-9
        r = y.T @ w - theta[:, None] * (y.T @ v)
        d = hd[None, :] - theta[:, None]
        d = np.where(np.abs(d) < DENOM_FLOOR, np.where(d < 0.0, -DENOM_FLOOR, DENOM_FLOOR), d)
        assert d[0, 0] == DENOM_FLOOR and d[0, 1] == -DENOM_FLOOR and d[k - 1, dim - 1] == DENOM_FLOOR
        t, rn = p.correction(v, w, y, theta, hd)
        assert np.array_equal(t, r / d) and np.array_equal(rn, np.einsum("re,re->r", r, r))
        v, w, y = rng.standard_normal((m, dim)), rng.standard_normal((m, dim)), rng.standard_normal((m, k))
        theta, hd = np.sort(rng.standard_normal(k)), rng.standard_normal(dim) + 2.0
        t, rn = p.correction(v, w, y, theta, hd)
        r, tref, d = correction_reference(v, w, y, theta, hd)
        E = (m + 2) * U * (np.abs(y).T @ np.abs(w) + np.abs(theta)[:, None] * (np.abs(y).T @ np.abs(v)))
        ra = np.abs(r).astype(np.float64)
        bt = (E + 3 * U * ra) / np.abs(d)
        bn = (2 * ra * E + E * E).sum(axis=1) + dim * U * (ra * ra).sum(axis=1)
        nref = (r * r).sum(axis=1).astype(np.float64)
        worst_t = max(worst_t, (np.abs(t - tref.astype(np.float64)) / bt).max())
        worst_n = max(worst_n, (np.abs(rn - nref) / bn).max())
        assert (np.abs(t - tref.astype(np.float64)) <= bt).all() and (np.abs(rn - nref) <= bn).all()
        t2, rn2 = p.correction(v, w, y, theta, hd)
        assert np.array_equal(t, t2) and np.array_equal(rn, rn2)
        if k == 11:                                                  # the roots in any grouping: the same bits
            t3, rn3 = p.correction(v, w, y[:, 8:], theta[8:], hd)
            assert np.array_equal(t[8:], t3) and np.array_equal(rn[8:], rn3)
    print(f"correction dim={dim}: worst error / bound: t {worst_t:.3f}, |r|^2 {worst_n:.3f}")


# ---- the solver ----------------------------------------------------------------------------------------------------
def davidson_solver(**kw):
    from evcont_amd.fci_device import DeviceFCI
    return DeviceFCI(eigensolver="davidson", **kw)


def compare(e_d, v_d, e_h, v_h, nroots):
    if nroots == 1:
        assert isinstance(e_d, float) and v_d.ndim == 2
        e_d, v_d, e_h, v_h = [e_d], [v_d], [e_h], [v_h]
    assert len(e_d) == len(v_d) == nroots
    for v in v_d:
        assert v.flat[np.argmax(np.abs(v))] > 0.0 and abs(np.linalg.norm(v) - 1.0) < 1e-12
    de = max(abs(a - b) for a, b in zip(e_d, e_h))
    dv = max(min(np.abs(a - b).max(), np.abs(a + b).max()) for a, b in zip(v_d, v_h))
    return de, dv


@pytest.mark.parametrize("norb,nelec", [(4, (2, 2)), (6, (3, 2)), (8, (4, 4))])
@pytest.mark.parametrize("nroots", [1, 3])
def test_davidson_kernel_against_host(norb, nelec, nroots):
    h1, h2 = oao_integrals(norb)
    s = davidson_solver()
    e_d, v_d = s.kernel(h1, h2, norb, nelec, nroots=nroots)
    rec = solve_record()
    info = s.davidson_info
    assert s.converged is True and (info["residuals"] <= 1e-10).all()
    assert re.fullmatch(SOLVE_RECORDS["evc_fci_combine"], rec), rec        # the Ritz vectors are the last thing formed
    assert rec.endswith(f" k={nroots} groups=1")
    e_h, v_h = _HOST.kernel(h1, h2, norb, nelec, nroots=nroots)
    de, dv = compare(e_d, v_d, e_h, v_h, nroots)
    print(f"davidson norb={norb} nelec={nelec} nroots={nroots}: {info['iterations']} iterations, {info['nsigma']} sigma "
          f"vectors, {info['restarts']} restarts, |dE|={de:.2e} |dv|={dv:.2e}")
    assert de < 1e-10 and dv < 1e-7
    e_2, v_2 = davidson_solver().kernel(h1, h2, norb, nelec, nroots=nroots)
    assert np.array_equal(np.asarray(e_d), np.asarray(e_2)) and np.array_equal(np.asarray(v_d), np.asarray(v_2))


def test_davidson_kernel_h10_against_the_default_route():
    from evcont_amd.fci_device import DeviceFCI
    norb, nelec = 10, (5, 5)
    h1, h2 = oao_integrals(norb)
    s = davidson_solver()
    e_d, v_d = s.kernel(h1, h2, norb, nelec)
    info = s.davidson_info
    e_h, v_h = DeviceFCI().kernel(h1, h2, norb, nelec)
    de, dv = compare(e_d, v_d, e_h, v_h, 1)
    print(f"davidson H10: {info['iterations']} iterations, {info['nsigma']} sigma vectors, {info['restarts']} restarts, "
          f"|dE|={de:.2e} |dv|={dv:.2e}")
    assert s.converged is True and de < 1e-10 and dv < 1e-7
    # warm start from a vector converged to 1e-10, asked for 1e-9 (a margin far above what reloading the vector changes
    # of its residual): one sigma vector
    warm = davidson_solver(conv_tol=1e-9)
    e_w, v_w = warm.kernel(h1, h2, norb, nelec, ci0=v_d)
    assert warm.converged is True and warm.davidson_info["nsigma"] == 1 and abs(e_w - e_d) < 1e-10
    e_2, v_2 = davidson_solver().kernel(h1, h2, norb, nelec)
    assert e_2 == e_d and np.array_equal(v_2, v_d)


def test_davidson_kernel_with_restarts_and_the_iteration_cap():
    norb, nelec, nroots, max_space = RESTART_CASE
    h1, h2 = oao_integrals(norb)
    s = davidson_solver(max_space=max_space)
    e_d, v_d = s.kernel(h1, h2, norb, nelec, nroots=nroots)
    e_h, v_h = _HOST.kernel(h1, h2, norb, nelec, nroots=nroots)
    de, dv = compare(e_d, v_d, e_h, v_h, nroots)
    print(f"davidson max_space={max_space}: {s.davidson_info['nsigma']} sigma vectors, {s.davidson_info['restarts']} "
          f"restarts, |dE|={de:.2e} |dv|={dv:.2e}")
    assert s.converged is True and s.davidson_info["restarts"] >= 3 and de < 1e-10 and dv < 1e-7
    capped = davidson_solver(max_cycle=2)
    with pytest.warns(RuntimeWarning, match="not converged"):
        e_c, v_c = capped.kernel(h1, h2, norb, nelec)
    assert capped.converged is False and v_c.shape == v_d.shape and e_c > e_d


def test_container_grown_with_the_davidson_solver_h6():
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    from evcont_amd.ab_initio_gradients_loewdin import get_energy_with_grad
    cd = FCI_EVCont_obj(cisolver=davidson_solver(), cibasis="OAO")
    ch = FCI_EVCont_obj(cisolver=SmallFCI(), cibasis="OAO")
    for d in (1.5, 2.0, 2.8):
        cd.append_to_rdms(hydrogen_chain(6, d, need_grad=False))
        ch.append_to_rdms(hydrogen_chain(6, d, need_grad=False))
    assert cd.cisolver.converged is True
    m = s_gaussian_mol(bent_chain(6, d=1.9, seed=11, amp=0.15))
    Ed, gd = get_energy_with_grad(m, cd.one_rdm, cd.two_rdm, cd.overlap)
    Eh, gh = get_energy_with_grad(m, ch.one_rdm, ch.two_rdm, ch.overlap)
    print(f"H6 container, Davidson against SmallFCI: |dE|={abs(Ed - Eh):.2e} |dg|={np.abs(gd - gh).max():.2e}")
    assert abs(Ed - Eh) < 1e-9 and np.abs(gd - gh).max() < 1e-8
