"""Reference statements for the s-Gaussian AO integrals (evcont_amd/hchain.py, csrc/sgto.hip), shared by
tests/test_sgto_reference_host.py, tests/test_sgto_truth_host.py, tests/test_gpu_sgto.py, tests/test_gpu_sgto_limits.py
and tests/golden/make_sgto_truth.py -- a helper, no test.

``loop_reference``: plain Python loops over contracted and primitive indices (at most four centres), for each of the
eight outputs the value and the sum of the absolute values of its primitive-level addends.  ``abs_sums``: the same
sums for any number of centres, vectorised.  ``allowed``: the per-element bound the tests hold every route to,

    2^-53 (n_terms + 432) sum|terms|

with n_terms the length of the sum (K^4 for eri / eri_ip1, K^2 (A + 1) for hcore / dhcore, K^2 for S / ipovlp, A for enuc /
gnuc) and 432 = 32 roundings within a term + 4 / 1e-2 for the cancellation in F1 = (F0 - exp(-t)) / 2t just above the
switch of ``boys01`` at t = 1e-2.  In the derivative arrays the F0 part and the F1 part of a primitive addend count as
separate terms.

That bound compares two float64 routes of one algorithm.  Against the exact values (tests/golden/sgto_truth.npz, mpmath,
made by tests/golden/make_sgto_truth.py) a route is held to ``allowed_truth``,

    2^-53 [ (n_terms + 32) sum|terms| + c cancel + cond ]

with ``cancel`` a second absolute sum per element: over the primitive F1 addends with t >= 1e-2, the absolute coefficient
of F1 times (F0(t) + exp(-t)) / 2t, which is what one relative rounding of erf and of exp each leaves in
F1 = (F0 - exp(-t)) / 2t.  It is large only where the cancellation is (4 / t units of F1 just above the switch, nothing
below it) and zero for the arrays without F1.  An addend counts from t >= 1e-2 (1 - 2^-40): t as a float64 route
computes it is a few ulp from the exact one, and a route may send such an addend down the erf branch.

``cond`` is a third sum, for what no float64 route of these formulas can avoid: the coordinates are exact inputs, and
rounding the intermediates that are differences or exponents of them is amplified by their condition.  (Measured with
``s_gaussian_mol`` against the truth before ``cond`` existed: 92 units of sum|terms| in S for centres 40 Bohr apart,
where F1 plays no part; 258 in dhcore of ``4c_K1`` at an element whose (P - C)_z is 0.002 between coordinates of 0.8,
far from the switch.)  Two weights per addend, worked out from the operations both routes perform:
  * Kab = exp(-x), x = mu |AB|^2 computed with EXP_ROUNDINGS = 9 roundings (a b, a + b, the quotient; AB_x and its square,
    two additions; the product): a relative error of 9 x in Kab.  Every addend weighs EXP_ROUNDINGS (x_ab + x_cd) times
    its absolute value.
  * P_x = (a A_x + b B_x) / p: a product, the sum and the quotient round, P_ROUNDINGS = 3 relative to
    (a |A_x| + b |B_x|) / p, so (P - Q)_x, a factor of every F1 addend, carries s_ab,x + s_cd,x with
    s_ab,x = 3 (a |A_x| + b |B_x|) / p whatever its own size (nothing for a nucleus, and nothing where A_x = B_x: both
    routes take P_x = A_x there).  Every F1 addend weighs that times |addend / (P - Q)_x|.
The same rounding of P reaches F0 and F1 through t, at most by (t F1 / F0) dt / t <= dt / 2t of the addend; the
geometries of the fixture keep that below the 32 roundings of a term, and ``cond`` leaves it out.  ``cond`` is negligible
beside 32 sum|terms| for compact molecules near the origin and is what the bound consists of at 40 Bohr.  Elements all of
whose addends vanish exactly (sum|terms| = 0: underflown Kab, every primitive on one centre) must be exactly 0 on every
route, whatever ``cond`` is: P_x = A_x where A_x = B_x makes P - Q and P - C vanish exactly there.  (Before this bound
existed both routes rounded (a A + b A) / p, and int2e_ip1[x, i, i, i, i], exactly 0, came out as 1e-17.)

``c`` is measured, not derived: the largest value ``s_gaussian_mol`` needs against the truth over all cases of the
fixture is C_MEASURED (tests/test_sgto_truth_host.py prints it; ``boys01`` alone needs 2.2), and the bound for a device
route takes
C_CANCEL = ceil(2 C_MEASURED), the margin for a second correct erf / exp of 1-2 ulp.  ``s_gaussian_mol`` itself is held
to C_CANCEL / 2, and two float64 routes against each other where no truth exists (more than a handful of centres) to
2 C_CANCEL without ``cond`` (``allowed_pair``).

``one_electron`` and ``eri_rows``: value, sum|terms|, cancel and cond of the one-electron arrays and of chosen bra rows of eri /
eri_ip1 for any number of centres, vectorised over one set of term formulas, so that 96 centres do not need the full
two-electron pass of ``s_gaussian_mol``."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from evcont_amd.hchain import boys01

NAMES = ("enuc", "S", "hcore", "eri", "ipovlp", "dhcore", "eri_ip1", "gnuc")
ROUNDINGS = 432
T_SWITCH = 1e-2                           # the switch of boys01
T_CANCEL = T_SWITCH * (1.0 - 2.0 ** -40)  # F1 addends from here on count in ``cancel``
TERM_ROUNDINGS = 32                       # roundings within one primitive term
C_MEASURED = 1.92                         # largest c s_gaussian_mol needs against sgto_truth.npz
C_CANCEL = 4                              # ceil(2 C_MEASURED): the c of a device route against the truth
CANCEL_FIELDS = ("dhcore", "eri_ip1")     # the arrays with F1 addends
EXP_ROUNDINGS = 9                         # roundings in mu |AB|^2 as both routes compute it: each is x in exp(-x)
P_ROUNDINGS = 3                           # roundings in P_x = (a A_x + b B_x) / p relative to (a |A_x| + b |B_x|) / p


def n_terms(name, A, K):
    return {"eri": K ** 4, "eri_ip1": K ** 4, "hcore": K * K * (A + 1), "dhcore": K * K * (A + 1), "S": K * K,
            "ipovlp": K * K, "enuc": A, "gnuc": A}[name]


def allowed(name, A, K, abs_sum):
    return 2.0 ** -53 * (n_terms(name, A, K) + ROUNDINGS) * np.asarray(abs_sum)


def allowed_truth(name, A, K, abs_sum, cancel, cond, c=None):
    """The bound against the exact value: 2^-53 [(n_terms + 32) sum|terms| + c cancel + cond], c = C_CANCEL unless
    given."""
    c = C_CANCEL if c is None else c
    return 2.0 ** -53 * ((n_terms(name, A, K) + TERM_ROUNDINGS) * np.asarray(abs_sum) + c * np.asarray(cancel) +
                         np.asarray(cond))


def allowed_pair(name, A, K, abs_sum, cancel):
    """The bound for two float64 routes of the one statement against each other, where no truth exists: the expression of
    ``allowed_truth`` with 2 C_CANCEL and without ``cond`` (both routes round Kab's exponent and P alike), plus the
    smallest normal number: below it a result is a sum of subnormal products, which carry no relative accuracy (a chain
    of 64 centres has elements from 1 down to exact 0 through that range)."""
    return allowed_truth(name, A, K, abs_sum, cancel, 0.0, c=2 * C_CANCEL) + 2.0 ** -1022


def needed_c(name, A, K, err, abs_sum, cancel, cond):
    """Smallest c with err <= allowed_truth(..., c) on every element (inf where no c does)."""
    err, s, k, d = (np.asarray(v, dtype=np.float64) for v in (err, abs_sum, cancel, cond))
    over = err / 2.0 ** -53 - (n_terms(name, A, K) + TERM_ROUNDINGS) * s - d
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.where(over <= 0.0, 0.0, np.where(k > 0.0, over / k, np.inf))
    return float(np.max(need)) if need.size else 0.0


def truth_ratio(name, A, K, got, hi, lo, abs_sum, cancel, cond, c=None):
    """Largest |got - (hi + lo)| in units of ``allowed_truth``; inf if an element whose addends all vanish
    (sum|terms| = 0) is not exactly 0."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == np.shape(hi), (name, got.shape, np.shape(hi))
    err = np.abs((got - hi) - lo)                    # got - hi is exact for got within a factor 2 of hi
    bound = allowed_truth(name, A, K, abs_sum, cancel, cond, c)
    if np.any(got[np.asarray(abs_sum) == 0.0] != 0.0):
        return np.inf
    nz = bound > 0.0
    return float(np.max(err[nz] / bound[nz])) if np.any(nz) else 0.0


def worst_ratio(name, A, K, got, want, abs_sum):
    """Largest |got - want| in units of 2^-53 sum|terms| (elements whose terms all vanish must agree exactly)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    s = np.asarray(abs_sum, dtype=np.float64)
    assert err.shape == s.shape, (name, err.shape, s.shape)
    if np.any(err[s == 0.0] != 0.0):
        return np.inf
    nz = s > 0.0
    return float(np.max(err[nz] / (2.0 ** -53 * s[nz]))) if np.any(nz) else 0.0


def _boys(t):
    if t < 1e-2:
        f0 = f1 = 0.0
        term = 1.0
        for k in range(9):
            f0 += term / (2 * k + 1)
            f1 += term / (2 * k + 3)
            term = term * (-t) / (k + 1)
        return f0, f1
    rt = math.sqrt(t)
    f0 = 0.5 * math.sqrt(math.pi) / rt * math.erf(rt)
    return f0, (f0 - math.exp(-t)) / (2.0 * t)


def loop_reference(R, Z, ex, co, with_cancel=False):
    """{name: (value, sum|terms|)} by plain loops; R (A,3) Bohr with A <= 4, Z (A), ex / co (K).  ``with_cancel``: that,
    {name: cancel} for the CANCEL_FIELDS and {name: cond}."""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3)
    A, K = R.shape[0], len(ex)
    assert A <= 4
    Z = [float(z) for z in Z]
    ex = [float(x) for x in ex]
    cn = [float(c) * (2.0 * a / math.pi) ** 0.75 for a, c in zip(ex, co)]
    X = [[float(v) for v in r] for r in R]
    n = A
    val = {"enuc": np.zeros(()), "S": np.zeros((n, n)), "hcore": np.zeros((n, n)), "eri": np.zeros((n, n, n, n)),
           "ipovlp": np.zeros((3, n, n)), "dhcore": np.zeros((A, 3, n, n)), "eri_ip1": np.zeros((3, n, n, n, n)),
           "gnuc": np.zeros((A, 3))}
    ab = {k: np.zeros_like(v) for k, v in val.items()}
    dH1, adH1, cdH1, kdH1 = np.zeros((3, n, n)), np.zeros((3, n, n)), np.zeros((3, n, n)), np.zeros((3, n, n))
    cn_ = {k: np.zeros_like(val[k]) for k in CANCEL_FIELDS}
    kd = {k: np.zeros_like(v) for k, v in val.items()}         # cond

    def amp(t, f0):                                # what one rounding of erf and of exp each leaves in F1
        return (f0 + math.exp(-t)) / (2.0 * t) if t >= T_CANCEL else 0.0

    def pair(i, j, a, b):
        p = a + b
        mu = a * b / p
        AB = [X[i][x] - X[j][x] for x in range(3)]
        r2 = sum(d * d for d in AB)
        P = [X[i][x] if AB[x] == 0.0 else (a * X[i][x] + b * X[j][x]) / p for x in range(3)]
        # ... and what the roundings of the exponent and of P weigh
        return (p, mu, AB, r2, math.exp(-mu * r2), P, EXP_ROUNDINGS * mu * r2,
                [0.0 if AB[x] == 0.0 else P_ROUNDINGS * (a * abs(X[i][x]) + b * abs(X[j][x])) / p for x in range(3)])

    # one-electron part
    for i in range(n):
        for j in range(n):
            for ia in range(K):
                for ib in range(K):
                    a, b, w = ex[ia], ex[ib], cn[ia] * cn[ib]
                    p, mu, AB, r2, kab, P, kx, sP = pair(i, j, a, b)
                    sp = (math.pi / p) ** 1.5 * kab
                    tp = mu * (3.0 - 2.0 * mu * r2) * sp
                    val["S"][i, j] += w * sp
                    ab["S"][i, j] += abs(w * sp)
                    kd["S"][i, j] += abs(w * sp) * kx
                    val["hcore"][i, j] += w * tp
                    ab["hcore"][i, j] += abs(w * tp)
                    kd["hcore"][i, j] += abs(w * tp) * kx
                    for x in range(3):
                        dsp = -2.0 * mu * AB[x] * sp
                        dtp = mu * (-4.0 * mu * AB[x] * sp + (3.0 - 2.0 * mu * r2) * dsp)
                        val["ipovlp"][x, i, j] += -w * dsp
                        ab["ipovlp"][x, i, j] += abs(w * dsp)
                        kd["ipovlp"][x, i, j] += abs(w * dsp) * kx
                        dH1[x, i, j] += w * dtp
                        adH1[x, i, j] += abs(w * dtp)
                        kdH1[x, i, j] += abs(w * dtp) * kx
                    for c in range(A):
                        PC = [P[x] - X[c][x] for x in range(3)]
                        t = p * sum(d * d for d in PC)
                        f0, f1 = _boys(t)
                        pref = -Z[c] * (2.0 * math.pi / p) * kab * w
                        val["hcore"][i, j] += pref * f0
                        ab["hcore"][i, j] += abs(pref * f0)
                        kd["hcore"][i, j] += abs(pref * f0) * kx
                        for x in range(3):
                            t0, t1 = pref * (-2.0 * mu * AB[x] * f0), pref * (-2.0 * a * PC[x] * f1)
                            dH1[x, i, j] += t0 + t1
                            adH1[x, i, j] += abs(t0) + abs(t1)
                            cdH1[x, i, j] += abs(pref * 2.0 * a * PC[x]) * amp(t, f0)
                            kdH1[x, i, j] += (abs(t0) + abs(t1)) * kx + abs(pref * 2.0 * a * f1) * sP[x]
                            o = pref * (-f1) * 2.0 * p * (-PC[x])
                            val["dhcore"][c, x, i, j] += o
                            ab["dhcore"][c, x, i, j] += abs(o)
                            cn_["dhcore"][c, x, i, j] += abs(pref * 2.0 * p * PC[x]) * amp(t, f0)
                            kd["dhcore"][c, x, i, j] += abs(o) * kx + abs(pref * 2.0 * p * f1) * sP[x]
    for at in range(A):
        for arr, d in ((val["dhcore"], dH1), (ab["dhcore"], adH1), (cn_["dhcore"], cdH1), (kd["dhcore"], kdH1)):
            arr[at, :, at, :] += d[:, at, :]
            arr[at, :, :, at] += d[:, at, :]
    # nuclear repulsion
    for i in range(A):
        for j in range(A):
            if i == j:
                continue
            d = [X[i][x] - X[j][x] for x in range(3)]
            r = math.sqrt(sum(v * v for v in d))
            if j > i:
                val["enuc"] += Z[i] * Z[j] / r
                ab["enuc"] += abs(Z[i] * Z[j] / r)
            for x in range(3):
                val["gnuc"][i, x] -= Z[i] * Z[j] * d[x] / r ** 3
                ab["gnuc"][i, x] += abs(Z[i] * Z[j] * d[x] / r ** 3)
    # two-electron part
    prim = [(i, ia) for i in range(n) for ia in range(K)]
    pairs = {}
    for i, ia in prim:
        for j, ib in prim:
            pairs[(i, ia, j, ib)] = pair(i, j, ex[ia], ex[ib])
    for (i, ia, j, ib), (p, mu, AB, r2, kab, P, kx, sP) in pairs.items():
        wb = cn[ia] * cn[ib] * kab
        for (k, ic, l, id_), (q, _, _, _, kcd, Q, kxq, sQ) in pairs.items():
            rho = p * q / (p + q)
            PQ = [P[x] - Q[x] for x in range(3)]
            t = rho * sum(d * d for d in PQ)
            f0, f1 = _boys(t)
            w = 2.0 * math.pi ** 2.5 / (p * q * math.sqrt(p + q)) * wb * cn[ic] * cn[id_] * kcd
            val["eri"][i, j, k, l] += w * f0
            ab["eri"][i, j, k, l] += abs(w * f0)
            kd["eri"][i, j, k, l] += abs(w * f0) * (kx + kxq)
            for x in range(3):
                t0, t1 = w * (-2.0 * mu * AB[x] * f0), w * (-2.0 * rho * (ex[ia] / p) * PQ[x] * f1)
                val["eri_ip1"][x, i, j, k, l] -= t0 + t1
                ab["eri_ip1"][x, i, j, k, l] += abs(t0) + abs(t1)
                cn_["eri_ip1"][x, i, j, k, l] += abs(w * 2.0 * rho * (ex[ia] / p) * PQ[x]) * amp(t, f0)
                kd["eri_ip1"][x, i, j, k, l] += ((abs(t0) + abs(t1)) * (kx + kxq) +
                                                 abs(w * 2.0 * rho * (ex[ia] / p) * f1) * (sP[x] + sQ[x]))
    out = {k: (val[k], ab[k]) for k in NAMES}
    return (out, cn_, kd) if with_cancel else out


def _amp(t, f0):
    """(F0 + exp(-t)) / 2t where t >= T_CANCEL, else 0."""
    big = t >= T_CANCEL
    ts = np.where(big, t, 1.0)
    return np.where(big, (f0 + np.exp(-ts)) / (2.0 * ts), 0.0)


def abs_sums(R, Z, ex, co, with_cancel=False):
    """{name: sum|terms|} as ``loop_reference`` counts them, for any number of centres (numpy, primitives^4 doubles).
    ``with_cancel``: that, {name: cancel} for the CANCEL_FIELDS and {name: cond}."""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3)
    A, K = R.shape[0], len(ex)
    Z = np.asarray(Z, dtype=np.float64)
    a = np.tile(np.asarray(ex, dtype=np.float64), A)
    owner = np.repeat(np.arange(A), K)
    Rp = R[owner]
    cn = np.abs(np.tile(np.asarray(co, dtype=np.float64), A) * (2.0 * a / np.pi) ** 0.75)
    Np = A * K
    O = np.zeros((Np, A))
    O[np.arange(Np), owner] = cn                         # |weights|: contracting with O sums absolute addends
    c2 = lambda M: np.einsum("pi,...pq,qj->...ij", O, M, O)
    pp = a[:, None] + a[None, :]
    mu = a[:, None] * a[None, :] / pp
    AB = np.moveaxis(Rp[:, None, :] - Rp[None, :, :], -1, 0)         # (3,Np,Np)
    R2 = np.sum(AB * AB, axis=0)
    Kab = np.exp(-mu * R2)
    wide = lambda X: (a[:, None, None] * X[:, None, :] + a[None, :, None] * X[None, :, :]) / pp[:, :, None]
    P = np.where(np.moveaxis(AB, 0, -1) == 0.0, Rp[:, None, :], wide(Rp))
    Sp = (np.pi / pp) ** 1.5 * Kab
    kin = 3.0 - 2.0 * mu * R2
    dSp = -2.0 * mu[None] * AB * Sp[None]
    dTp = mu[None] * (-4.0 * mu[None] * AB * Sp[None] + kin[None] * dSp)
    out = {"S": c2(np.abs(Sp)), "ipovlp": c2(np.abs(dSp))}
    hc = c2(np.abs(mu * kin * Sp))
    adH1 = c2(np.abs(dTp))
    aop = np.zeros((A, 3, A, A))
    cdH1, cop = np.zeros((3, A, A)), np.zeros((A, 3, A, A))
    kx = EXP_ROUNDINGS * mu * R2
    sP = np.where(AB == 0.0, 0.0, P_ROUNDINGS * np.moveaxis(wide(np.abs(Rp)), -1, 0))              # (3,Np,Np)
    cond = {"S": c2(np.abs(Sp) * kx), "ipovlp": c2(np.abs(dSp) * kx[None]), "enuc": np.zeros(()), "gnuc": np.zeros((A, 3))}
    khc, kdH1, kop = c2(np.abs(mu * kin * Sp) * kx), c2(np.abs(dTp) * kx[None]), np.zeros((A, 3, A, A))
    for c in range(A):
        PC = np.moveaxis(P - R[c][None, None, :], -1, 0)
        t = pp * np.sum(PC * PC, axis=0)
        f0, f1 = boys01(t)
        pref = -Z[c] * (2.0 * np.pi / pp) * Kab
        if with_cancel:
            am = _amp(t, f0)
            cdH1 += c2(np.abs(pref[None] * 2.0 * a[None, :, None] * PC) * am[None])
            cop[c] = c2(np.abs(pref[None] * 2.0 * pp[None] * PC) * am[None])
            khc += c2(np.abs(pref * f0) * kx)
            kdH1 += c2((np.abs(pref[None] * 2.0 * mu[None] * AB * f0[None]) +
                        np.abs(pref[None] * 2.0 * a[None, :, None] * PC * f1[None])) * kx[None] +
                       np.abs(pref * f1)[None] * 2.0 * a[None, :, None] * sP)
            kop[c] = c2(np.abs(pref[None] * f1[None] * 2.0 * pp[None] * PC) * kx[None] + np.abs(pref * f1 * 2.0 * pp)[None] * sP)
        hc += c2(np.abs(pref * f0))
        adH1 += c2(np.abs(pref[None] * 2.0 * mu[None] * AB * f0[None]) +
                   np.abs(pref[None] * 2.0 * a[None, :, None] * PC * f1[None]))
        aop[c] = c2(np.abs(pref[None] * f1[None] * 2.0 * pp[None] * PC))
    for at in range(A):
        aop[at, :, at, :] += adH1[:, at, :]
        aop[at, :, :, at] += adH1[:, at, :]
        cop[at, :, at, :] += cdH1[:, at, :]
        cop[at, :, :, at] += cdH1[:, at, :]
        kop[at, :, at, :] += kdH1[:, at, :]
        kop[at, :, :, at] += kdH1[:, at, :]
    out["hcore"], out["dhcore"] = hc, aop
    en, gn = 0.0, np.zeros((A, 3))
    for i in range(A):
        for j in range(A):
            if i != j:
                d = R[i] - R[j]
                r = np.linalg.norm(d)
                en += abs(Z[i] * Z[j] / r) if j > i else 0.0
                gn[i] += np.abs(Z[i] * Z[j] * d / r ** 3)
    out["enuc"], out["gnuc"] = np.asarray(en), gn
    q, Q, Kq = pp.reshape(-1), P.reshape(-1, 3), Kab.reshape(-1)
    pI = pp.reshape(-1)[:, None]
    PQ = np.moveaxis(P.reshape(-1, 1, 3) - Q[None, :, :], -1, 0)     # (3,Np^2,Np^2)
    rho = pI * q[None, :] / (pI + q[None, :])
    t = rho * np.sum(PQ * PQ, axis=0)
    f0, f1 = boys01(t)
    w = 2.0 * np.pi ** 2.5 / (pI * q[None, :] * np.sqrt(pI + q[None, :])) * Kq[:, None] * Kq[None, :]
    c4 = lambda M: np.einsum("pi,qj,...pqrs,rk,sl->...ijkl", O, O, M.reshape(M.shape[:-2] + (Np,) * 4), O, O,
                             optimize=True)
    out["eri"] = c4(np.abs(w * f0))
    mab = (mu[None] * AB).reshape(3, -1, 1)
    apb = (a[:, None] / pp).reshape(-1, 1)
    out["eri_ip1"] = c4(np.abs(w[None] * 2.0 * mab * f0[None]) + np.abs(w[None] * 2.0 * rho[None] * apb[None] * PQ * f1[None]))
    out = {k: out[k] for k in NAMES}
    if not with_cancel:
        return out
    kq = kx.reshape(-1, 1) + kx.reshape(1, -1)
    sq = sP.reshape(3, -1, 1) + sP.reshape(3, 1, -1)
    cond.update(hcore=khc, dhcore=kop, eri=c4(np.abs(w * f0) * kq))
    cond["eri_ip1"] = c4((np.abs(w[None] * 2.0 * mab * f0[None]) + np.abs(w[None] * 2.0 * rho[None] * apb[None] * PQ * f1[None])) *
                         kq[None] + np.abs(w * 2.0 * rho * apb * f1)[None] * sq)
    return (out, {"dhcore": cop, "eri_ip1": c4(np.abs(w[None] * 2.0 * rho[None] * apb[None] * PQ) * _amp(t, f0)[None])},
            {k: cond[k] for k in NAMES})


# ---- any number of centres: the one-electron arrays, and chosen bra rows of the two-electron ones ----------------
def _primitives(R, ex, co):
    R = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(-1, 3))
    A, K = R.shape[0], len(ex)
    a = np.tile(np.asarray(ex, dtype=np.float64), A)
    owner = np.repeat(np.arange(A), K)
    cn = np.tile(np.asarray(co, dtype=np.float64), A) * (2.0 * a / np.pi) ** 0.75
    Cm = np.zeros((A * K, A))
    Cm[np.arange(A * K), owner] = cn
    return R, A, K, a, owner, R[owner], Cm


def _pairs(a, Ra, b, Rb):
    """p, mu, AB (3,..), |AB|^2, Kab, P (3,..) of the primitive pairs a (rows) x b (columns), and the weights of cond:
    EXP_ROUNDINGS mu |AB|^2 and P_ROUNDINGS (a |A_x| + b |B_x|) / p (0 where A_x = B_x)."""
    p = a[:, None] + b[None, :]
    mu = a[:, None] * b[None, :] / p
    AB = np.moveaxis(Ra[:, None, :] - Rb[None, :, :], -1, 0)
    r2 = np.sum(AB * AB, axis=0)
    wide = lambda X, Y: np.moveaxis((a[:, None, None] * X[:, None, :] + b[None, :, None] * Y[None, :, :]) / p[:, :, None], -1, 0)
    P = np.where(AB == 0.0, np.moveaxis(Ra, -1, 0)[:, :, None], wide(Ra, Rb))
    return (p, mu, AB, r2, np.exp(-mu * r2), P, EXP_ROUNDINGS * mu * r2,
            np.where(AB == 0.0, 0.0, P_ROUNDINGS * wide(np.abs(Ra), np.abs(Rb))))


def one_electron(R, Z, ex, co):
    """{name: (value, sum|terms|, cancel, cond)} of enuc, S, hcore, ipovlp, dhcore, gnuc for any number of centres."""
    R, A, K, a, owner, Rp, Cm = _primitives(R, ex, co)
    Z = np.asarray(Z, dtype=np.float64)
    Ca = np.abs(Cm)
    c2 = lambda M: np.einsum("pi,...pq,qj->...ij", Cm, M, Cm, optimize=True)
    c2a = lambda M: np.einsum("pi,...pq,qj->...ij", Ca, M, Ca, optimize=True)
    p, mu, AB, r2, Kab, P, kx, sP = _pairs(a, Rp, a, Rp)
    Sp = (np.pi / p) ** 1.5 * Kab
    kin = 3.0 - 2.0 * mu * r2
    dSp = -2.0 * mu[None] * AB * Sp[None]
    dTp = mu[None] * (-4.0 * mu[None] * AB * Sp[None] + kin[None] * dSp)
    S, aS, kS = c2(Sp), c2a(np.abs(Sp)), c2a(np.abs(Sp) * kx)
    dS, adS, kdS = c2(dSp), c2a(np.abs(dSp)), c2a(np.abs(dSp) * kx[None])
    Tp = mu * kin * Sp
    hc, ahc, khc = c2(Tp), c2a(np.abs(Tp)), c2a(np.abs(Tp) * kx)
    dH1, adH1, kdH1 = c2(dTp), c2a(np.abs(dTp)), c2a(np.abs(dTp) * kx[None])
    cdH1 = np.zeros((3, A, A))
    op, aop, cop, kop = (np.zeros((A, 3, A, A)) for _ in range(4))
    for c in range(A):
        PC = P - R[c][:, None, None]
        t = p * np.sum(PC * PC, axis=0)
        f0, f1 = boys01(t)
        am = _amp(t, f0)
        pref = -Z[c] * (2.0 * np.pi / p) * Kab
        v0 = pref * f0
        hc, ahc, khc = hc + c2(v0), ahc + c2a(np.abs(v0)), khc + c2a(np.abs(v0) * kx)
        t0, t1 = pref[None] * (-2.0 * mu[None] * AB * f0[None]), pref[None] * (-2.0 * a[None, :, None] * PC * f1[None])
        dH1 += c2(t0 + t1)
        adH1 += c2a(np.abs(t0) + np.abs(t1))
        cdH1 += c2a(np.abs(pref[None] * 2.0 * a[None, :, None] * PC) * am[None])
        kdH1 += c2a((np.abs(t0) + np.abs(t1)) * kx[None] + np.abs(pref * f1)[None] * 2.0 * a[None, :, None] * sP)
        o = pref[None] * f1[None] * 2.0 * p[None] * PC
        op[c], aop[c] = c2(o), c2a(np.abs(o))
        cop[c] = c2a(np.abs(pref[None] * 2.0 * p[None] * PC) * am[None])
        kop[c] = c2a(np.abs(o) * kx[None] + np.abs(pref * f1 * 2.0 * p)[None] * sP)
    for at in range(A):
        for arr, d in ((op, dH1), (aop, adH1), (cop, cdH1), (kop, kdH1)):
            arr[at, :, at, :] += d[:, at, :]
            arr[at, :, :, at] += d[:, at, :]
    D = R[:, None, :] - R[None, :, :]
    r = np.sqrt(np.sum(D * D, axis=-1))
    np.fill_diagonal(r, 1.0)
    zz = Z[:, None] * Z[None, :]
    np.fill_diagonal(zz, 0.0)
    en = np.triu(zz / r, 1)
    gn = -zz[:, :, None] * D / r[:, :, None] ** 3
    zero = np.zeros
    return {"enuc": (np.asarray(np.sum(en)), np.asarray(np.sum(np.abs(en))), zero(()), zero(())),
            "S": (0.5 * (S + S.T), aS, zero((A, A)), kS), "hcore": (0.5 * (hc + hc.T), ahc, zero((A, A)), khc),
            "ipovlp": (-dS, adS, zero((3, A, A)), kdS), "dhcore": (op, aop, cop, kop),
            "gnuc": (np.sum(gn, axis=1), np.sum(np.abs(gn), axis=1), zero((A, 3)), zero((A, 3)))}


def eri_rows(R, ex, co, bra_pairs, chunk=64, threads=8):
    """{"eri": (value (B,n,n), sum|terms|, cancel, cond), "eri_ip1": (value (B,3,n,n), ...)}: the rows [i, j, :, :] and
    [:, i, j, :, :] of the ordered bra pairs ``bra_pairs`` = [(i, j), ...] over all kets, ``chunk`` pairs at a time on ``threads`` threads (numpy's loops release the interpreter)."""
    R, A, K, a, owner, Rp, Cm = _primitives(R, ex, co)
    Ca = np.abs(Cm)
    q, _, _, _, Kq, Q, kxq, sQ = _pairs(a, Rp, a, Rp)
    q, Kq, Q, kxq, sQ = q.reshape(-1), Kq.reshape(-1), Q.reshape(3, -1), kxq.reshape(1, -1), sQ.reshape(3, 1, -1)
    Np, K2 = A * K, K * K
    e, cn = a[:K], Cm[np.arange(K), 0]                        # the contraction, the same on every centre
    pairs = np.asarray(bra_pairs, dtype=np.int64).reshape(-1, 2)

    def some(lo):
        bi, bj = pairs[lo:lo + chunk, 0], pairs[lo:lo + chunk, 1]
        B = len(bi)
        # primitive pairs (pair, a on i, b on j), flattened to rows of B K^2
        rows = lambda X: np.ascontiguousarray(X).reshape(X.shape[:-3] + (B * K2, 1))
        ea, eb = np.broadcast_to(e[None, :, None], (B, K, K)), np.broadcast_to(e[None, None, :], (B, K, K))
        p, mu = ea + eb, ea * eb / (ea + eb)
        AB = np.moveaxis(R[bi] - R[bj], -1, 0)[:, :, None, None]                   # (3,B,1,1)
        r2 = np.sum(AB * AB, axis=0)
        Ri, Rj = (np.moveaxis(R[b], -1, 0)[:, :, None, None] for b in (bi, bj))        # (3,B,1,1)
        P = np.where(AB == 0.0, Ri, (ea[None] * Ri + eb[None] * Rj) / p[None])
        wb = rows(cn[None, :, None] * cn[None, None, :] * np.exp(-mu * r2))
        kx = rows(EXP_ROUNDINGS * mu * r2)
        sP = rows(np.where(AB == 0.0, 0.0, P_ROUNDINGS * (ea[None] * np.abs(Ri) + eb[None] * np.abs(Rj)) / p[None]))
        AB, P, apb, p, mu = rows(np.broadcast_to(AB, P.shape)), rows(P), rows(ea / p), rows(p), rows(mu)
        PQ = P - Q[:, None, :]                                                     # (3,B K^2,Np^2)
        rho = p * q[None, :] / (p + q[None, :])
        t = rho * np.sum(PQ * PQ, axis=0)
        f0, f1 = boys01(t)
        w = 2.0 * np.pi ** 2.5 / (p * q[None, :] * np.sqrt(p + q[None, :])) * wb * Kq[None, :]
        kq = kx + kxq
        # the bra weights are in w already: sum the primitive pairs of each bra pair, contract the ket ones
        bra = lambda M: np.sum(M.reshape(M.shape[:-2] + (B, K2, Np, Np)), axis=-3)
        fold = lambda M: np.moveaxis(np.einsum("...rs,rk,sl->...kl", bra(M), Cm, Cm, optimize=True), -3, 0)
        folda = lambda M: np.moveaxis(np.einsum("...rs,rk,sl->...kl", bra(M), Ca, Ca, optimize=True), -3, 0)
        v = w * f0
        t0, t1 = w[None] * (2.0 * mu[None] * AB * f0[None]), w[None] * (2.0 * rho[None] * apb[None] * PQ * f1[None])
        at = np.abs(t0) + np.abs(t1)
        fours = {"eri": (fold(v), folda(np.abs(v)), None, folda(np.abs(v) * kq)),
                 "eri_ip1": (fold(t0 + t1), folda(at),
                             folda(np.abs(w[None] * 2.0 * rho[None] * apb[None] * PQ) * _amp(t, f0)[None]),
                             folda(at * kq[None] + np.abs(w * 2.0 * rho * apb * f1)[None] * (sP + sQ)))}
        return {k: tuple(np.zeros_like(four[0]) if x is None else x for x in four) for k, four in fours.items()}

    starts = range(0, len(pairs), chunk)
    if threads > 1 and len(starts) > 1:
        with ThreadPoolExecutor(threads) as pool:
            parts = list(pool.map(some, starts))
    else:
        parts = [some(lo) for lo in starts]
    return {k: tuple(np.concatenate([part[k][f] for part in parts]) for f in range(4)) for k in ("eri", "eri_ip1")}


# ---- geometries of the tests ----------------------------------------------------------------------
def host_cases():
    """The four (R, Z, exponents, coefficients) cases of tests/test_sgto_reference_host.py."""
    from evcont_amd.hchain import (STO3G_H_COEFFICIENTS, STO3G_H_EXPONENTS, STO6G_H_COEFFICIENTS,
                                   STO6G_H_EXPONENTS)
    rng = np.random.default_rng(11)
    return {
        "3c_spread1.5_K3": (1.5 * rng.standard_normal((3, 3)), [1.0, 2.0, 0.5], STO3G_H_EXPONENTS, STO3G_H_COEFFICIENTS),
        "3c_spread0.08_K3": (0.08 * rng.standard_normal((3, 3)), [1.0, 1.0, 1.0], STO3G_H_EXPONENTS,
                             STO3G_H_COEFFICIENTS),
        "2c_STO6G": (np.array([[0.0, 0.1, -0.2], [1.3, -0.4, 0.6]]), [1.0, 1.0], STO6G_H_EXPONENTS, STO6G_H_COEFFICIENTS),
        "4c_K1": (1.2 * rng.standard_normal((4, 3)), [1.0, 1.0, 2.0, 1.0], (0.4,), (1.0,)),
    }


def _perturbed_chain(A, G, seed):
    """G perturbed chains of A centres: neighbours 1.7 Bohr apart along x, every coordinate moved by up to 0.3."""
    rng = np.random.default_rng(seed)
    R = np.zeros((G, A, 3))
    R[:, :, 0] = 1.7 * np.arange(A)
    return R + 0.3 * rng.uniform(-1.0, 1.0, (G, A, 3))


def truth_cases():
    """The cases of tests/golden/sgto_truth.npz: name -> (R (G,A,3), Z, exponents, coefficients)."""
    from evcont_amd.hchain import STO3G_H_COEFFICIENTS, STO3G_H_EXPONENTS
    sto3g = (STO3G_H_EXPONENTS, STO3G_H_COEFFICIENTS)
    host = host_cases()
    cases = {k: (np.asarray(host[k][0])[None],) + tuple(host[k][1:]) for k in ("3c_spread1.5_K3", "4c_K1")}
    # two centres d apart along an oblique direction, exponent 0.4: t = 0.4 d^2 in (00|11), t / 4, 2 t and t / 2 in the
    # other integral classes.  t = 1e-2 (1 +- s), s = 0 and 64 values from 1e-16 to 0.5; the doubles next to 1e-2; 125
    # values of t from 1e-4 to 1.
    s = np.geomspace(1e-16, 0.5, 64)
    t = np.concatenate([T_SWITCH * (1.0 - s), T_SWITCH * (1.0 + s),
                        [T_SWITCH, np.nextafter(T_SWITCH, 0.0), np.nextafter(T_SWITCH, 1.0)], np.geomspace(1e-4, 1.0, 125)])
    u = np.array([0.3, -0.5, 0.8])
    u = u / np.linalg.norm(u)
    R = np.zeros((t.size, 2, 3))                   # one centre at the origin: no cancellation among the coordinates
    R[:, 1] = np.sqrt(t / 0.4)[:, None] * u
    cases["switch_K1"] = (R, [1.0, 2.0], (0.4,), (1.0,))
    # clusters 0.03 ... 0.2 Bohr across: sums of 81 quartets on both sides of the switch
    rng = np.random.default_rng(12)
    R = rng.uniform(-0.5, 0.5, (8, 3, 3)) * np.geomspace(0.03, 0.2, 8)[:, None, None]
    cases["switch_K3"] = (R, [1.0, 2.0, 0.5], *sto3g)
    # a pair 1.4 Bohr apart and a centre 40 Bohr away: exp(-mu |AB|^2) of the tight cross pairs is exactly 0, t up to 1e4
    far = np.array([[[0.0, 0.0, 0.0], [0.9, -0.7, 0.8], [24.0, 20.0, -25.0]]])
    far[0, 1] *= 1.4 / np.linalg.norm(far[0, 1])
    cases["far"] = (far, [1.0, 2.0, 0.5], *sto3g)
    # ... and every cross pair exactly 0: one tight primitive, centres 8 and 40 Bohr apart
    cases["far_K1"] = (np.array([[[0.0, 0.0, 0.0], [5.0, -4.0, 4.8], [24.0, 20.0, -25.0]]]), [1.0, 2.0, 0.5], (35.5,), (1.0,))
    # the largest contraction: eight even-tempered primitives, coefficients of both signs
    cases["K8"] = (_perturbed_chain(2, 2, 13), [1.0, 2.0], tuple(0.05 * 3.0 ** k for k in range(8)),
                   (0.21, -0.34, 0.48, 0.39, -0.17, 0.12, 0.06, -0.02))
    return cases
