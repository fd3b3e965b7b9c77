"""Reference statements for the s-Gaussian AO integrals (evcont_amd/hchain.py, csrc/sgto.hip), shared by
tests/test_sgto_reference_host.py and tests/test_gpu_sgto.py -- a helper, no test.

``loop_reference``: plain Python loops over contracted and primitive indices (at most four centres), for each of the
eight outputs the value and the sum of the absolute values of its primitive-level addends.  ``abs_sums``: the same
sums for any number of centres, vectorised.  ``allowed``: the per-element bound the tests hold every route to,

    2^-53 (n_terms + 432) sum|terms|

with n_terms the length of the sum (K^4 for eri / eri_ip1, K^2 (A + 1) for hcore / dhcore, K^2 for S / ipovlp, A for enuc /
gnuc) and 432 = 32 roundings within a term + 4 / 1e-2 for the cancellation in F1 = (F0 - exp(-t)) / 2t just above the
switch of ``boys01`` at t = 1e-2.  In the derivative arrays the F0 part and the F1 part of a primitive addend count as
separate terms."""
import math

import numpy as np

from evcont_amd.hchain import boys01

NAMES = ("enuc", "S", "hcore", "eri", "ipovlp", "dhcore", "eri_ip1", "gnuc")
ROUNDINGS = 432


def n_terms(name, A, K):
    return {"eri": K ** 4, "eri_ip1": K ** 4, "hcore": K * K * (A + 1), "dhcore": K * K * (A + 1), "S": K * K,
            "ipovlp": K * K, "enuc": A, "gnuc": A}[name]


def allowed(name, A, K, abs_sum):
    return 2.0 ** -53 * (n_terms(name, A, K) + ROUNDINGS) * np.asarray(abs_sum)


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


def loop_reference(R, Z, ex, co):
    """{name: (value, sum|terms|)} by plain loops; R (A,3) Bohr with A <= 4, Z (A), ex / co (K)."""
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
    dH1, adH1 = np.zeros((3, n, n)), np.zeros((3, n, n))

    def pair(i, j, a, b):
        p = a + b
        mu = a * b / p
        AB = [X[i][x] - X[j][x] for x in range(3)]
        r2 = sum(d * d for d in AB)
        return p, mu, AB, r2, math.exp(-mu * r2), [(a * X[i][x] + b * X[j][x]) / p for x in range(3)]

    # one-electron part
    for i in range(n):
        for j in range(n):
            for ia in range(K):
                for ib in range(K):
                    a, b, w = ex[ia], ex[ib], cn[ia] * cn[ib]
                    p, mu, AB, r2, kab, P = pair(i, j, a, b)
                    sp = (math.pi / p) ** 1.5 * kab
                    tp = mu * (3.0 - 2.0 * mu * r2) * sp
                    val["S"][i, j] += w * sp
                    ab["S"][i, j] += abs(w * sp)
                    val["hcore"][i, j] += w * tp
                    ab["hcore"][i, j] += abs(w * tp)
                    for x in range(3):
                        dsp = -2.0 * mu * AB[x] * sp
                        dtp = mu * (-4.0 * mu * AB[x] * sp + (3.0 - 2.0 * mu * r2) * dsp)
                        val["ipovlp"][x, i, j] += -w * dsp
                        ab["ipovlp"][x, i, j] += abs(w * dsp)
                        dH1[x, i, j] += w * dtp
                        adH1[x, i, j] += abs(w * dtp)
                    for c in range(A):
                        PC = [P[x] - X[c][x] for x in range(3)]
                        f0, f1 = _boys(p * sum(d * d for d in PC))
                        pref = -Z[c] * (2.0 * math.pi / p) * kab * w
                        val["hcore"][i, j] += pref * f0
                        ab["hcore"][i, j] += abs(pref * f0)
                        for x in range(3):
                            t0, t1 = pref * (-2.0 * mu * AB[x] * f0), pref * (-2.0 * a * PC[x] * f1)
                            dH1[x, i, j] += t0 + t1
                            adH1[x, i, j] += abs(t0) + abs(t1)
                            o = pref * (-f1) * 2.0 * p * (-PC[x])
                            val["dhcore"][c, x, i, j] += o
                            ab["dhcore"][c, x, i, j] += abs(o)
    for at in range(A):
        for arr, d in ((val["dhcore"], dH1), (ab["dhcore"], adH1)):
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
    for (i, ia, j, ib), (p, mu, AB, r2, kab, P) in pairs.items():
        wb = cn[ia] * cn[ib] * kab
        for (k, ic, l, id_), (q, _, _, _, kcd, Q) in pairs.items():
            rho = p * q / (p + q)
            PQ = [P[x] - Q[x] for x in range(3)]
            f0, f1 = _boys(rho * sum(d * d for d in PQ))
            w = 2.0 * math.pi ** 2.5 / (p * q * math.sqrt(p + q)) * wb * cn[ic] * cn[id_] * kcd
            val["eri"][i, j, k, l] += w * f0
            ab["eri"][i, j, k, l] += abs(w * f0)
            for x in range(3):
                t0, t1 = w * (-2.0 * mu * AB[x] * f0), w * (-2.0 * rho * (ex[ia] / p) * PQ[x] * f1)
                val["eri_ip1"][x, i, j, k, l] -= t0 + t1
                ab["eri_ip1"][x, i, j, k, l] += abs(t0) + abs(t1)
    return {k: (val[k], ab[k]) for k in NAMES}


def abs_sums(R, Z, ex, co):
    """{name: sum|terms|} as ``loop_reference`` counts them, for any number of centres (numpy, primitives^4 doubles)."""
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
    P = (a[:, None, None] * Rp[:, None, :] + a[None, :, None] * Rp[None, :, :]) / pp[:, :, None]
    Sp = (np.pi / pp) ** 1.5 * Kab
    kin = 3.0 - 2.0 * mu * R2
    dSp = -2.0 * mu[None] * AB * Sp[None]
    dTp = mu[None] * (-4.0 * mu[None] * AB * Sp[None] + kin[None] * dSp)
    out = {"S": c2(np.abs(Sp)), "ipovlp": c2(np.abs(dSp))}
    hc = c2(np.abs(mu * kin * Sp))
    adH1 = c2(np.abs(dTp))
    aop = np.zeros((A, 3, A, A))
    for c in range(A):
        PC = np.moveaxis(P - R[c][None, None, :], -1, 0)
        f0, f1 = boys01(pp * np.sum(PC * PC, axis=0))
        pref = -Z[c] * (2.0 * np.pi / pp) * Kab
        hc += c2(np.abs(pref * f0))
        adH1 += c2(np.abs(pref[None] * 2.0 * mu[None] * AB * f0[None]) +
                   np.abs(pref[None] * 2.0 * a[None, :, None] * PC * f1[None]))
        aop[c] = c2(np.abs(pref[None] * f1[None] * 2.0 * pp[None] * PC))
    for at in range(A):
        aop[at, :, at, :] += adH1[:, at, :]
        aop[at, :, :, at] += adH1[:, at, :]
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
    f0, f1 = boys01(rho * np.sum(PQ * PQ, axis=0))
    w = 2.0 * np.pi ** 2.5 / (pI * q[None, :] * np.sqrt(pI + q[None, :])) * Kq[:, None] * Kq[None, :]
    c4 = lambda M: np.einsum("pi,qj,...pqrs,rk,sl->...ijkl", O, O, M.reshape(M.shape[:-2] + (Np,) * 4), O, O,
                             optimize=True)
    out["eri"] = c4(np.abs(w * f0))
    mab = (mu[None] * AB).reshape(3, -1, 1)
    apb = (a[:, None] / pp).reshape(-1, 1)
    out["eri_ip1"] = c4(np.abs(w[None] * 2.0 * mab * f0[None]) + np.abs(w[None] * 2.0 * rho[None] * apb[None] * PQ * f1[None]))
    return {k: out[k] for k in NAMES}


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
