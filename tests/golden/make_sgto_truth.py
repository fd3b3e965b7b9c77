"""Generates tests/golden/sgto_truth.npz: the eight arrays of ``hchain.s_gaussian_mol`` / ``evc_sgto_integrals_batch``
stated with mpmath at 60 digits, for the cases of ``tests/sgto_reference.truth_cases()``.  Plain loops over contracted and
primitive indices; F_n(t) = gammainc(n + 1/2, 0, t) / (2 t^(n + 1/2)), F_n(0) = 1 / (2n + 1); the float64 inputs are taken
as exact.  Per case ``<case>/R, Z, ex, co`` and per array

    <case>/<name>_hi, _lo   the value as a double-double: hi = float(x), lo = float(x - hi) (lo kept as float32: the pair
                            is good to 2^-77 of the value)
    <case>/<name>_abs       sum of the absolute primitive-level addends, as ``sgto_reference.loop_reference`` counts them
    <case>/<name>_cancel    (dhcore, eri_ip1) the cancellation sum of ``sgto_reference``: over the F1 addends with
                            t >= T_CANCEL, |coefficient of F1| (F0(t) + exp(-t)) / 2t
    <case>/<name>_cond      (all but enuc, gnuc) its conditioning sum: |addend| EXP_ROUNDINGS (mu_ab |AB|^2 + mu_cd |CD|^2)
                            over all addends, plus |addend / (P - Q)_x| (s_ab,x + s_cd,x) over the F1 addends, with
                            s_ab,x = P_ROUNDINGS (a |A_x| + b |B_x|) / p, 0 where A_x = B_x

The sums only scale a bound: they are rounded UP to 24 significant bits (and kept as float64 for their range), which
keeps the file small.  A nonzero sum below 1e-290 would make an element's bound a denormal; the cases have none, and
the generator refuses one.  About 1 minute on 16 processes.

    python tests/golden/make_sgto_truth.py [case ...]      # no argument: all cases, writes the file
                                                           # with arguments: recomputes those and compares with the file
"""
import os
import sys
from multiprocessing import Pool

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import sgto_reference as ref          # noqa: E402

mp.dps = 60
OUT = os.path.join(HERE, "sgto_truth.npz")
T_CANCEL = mpf(ref.T_CANCEL)


def boys(n, t):
    if t == 0:
        return mpf(1) / (2 * n + 1)
    return mp.gammainc(n + mpf(1) / 2, 0, t) / (2 * t ** (n + mpf(1) / 2))


def amp(t, f0):
    return (f0 + mp.exp(-t)) / (2 * t) if t >= T_CANCEL else mpf(0)


def geometry(args):
    """One geometry: {name: (value, sum|terms|, cancel)} as nested lists of mpf, flattened in C order."""
    R, Z, ex, co = args
    A, K = len(R), len(ex)
    X = [[mpf(float(v)) for v in r] for r in R]
    Z = [mpf(float(z)) for z in Z]
    ex = [mpf(float(x)) for x in ex]
    cn = [mpf(float(c)) * (2 * a / mp.pi) ** (mpf(3) / 4) for a, c in zip(ex, co)]
    n = A
    shapes = {"enuc": (), "S": (n, n), "hcore": (n, n), "eri": (n, n, n, n), "ipovlp": (3, n, n), "dhcore": (A, 3, n, n),
              "eri_ip1": (3, n, n, n, n), "gnuc": (A, 3)}
    new = lambda: {k: np.full(s, mpf(0), dtype=object) for k, s in shapes.items()}
    val, ab, cc, kd = new(), new(), new(), new()
    dH1, adH1, cdH1, kdH1 = (np.full((3, n, n), mpf(0), dtype=object) for _ in range(4))

    def pair(i, j, a, b):
        p = a + b
        mu = a * b / p
        AB = [X[i][x] - X[j][x] for x in range(3)]
        r2 = sum(d * d for d in AB)
        P = [(a * X[i][x] + b * X[j][x]) / p for x in range(3)]
        return (p, mu, AB, r2, mp.exp(-mu * r2), P, ref.EXP_ROUNDINGS * mu * r2,
                [mpf(0) if AB[x] == 0 else ref.P_ROUNDINGS * (a * abs(X[i][x]) + b * abs(X[j][x])) / p for x in range(3)])

    for i in range(n):
        for j in range(n):
            for ia in range(K):
                for ib in range(K):
                    a, b, w = ex[ia], ex[ib], cn[ia] * cn[ib]
                    p, mu, AB, r2, kab, P, kx, sP = pair(i, j, a, b)
                    sp = (mp.pi / p) ** (mpf(3) / 2) * kab
                    tp = mu * (3 - 2 * mu * r2) * sp
                    val["S"][i, j] += w * sp
                    ab["S"][i, j] += abs(w * sp)
                    kd["S"][i, j] += abs(w * sp) * kx
                    val["hcore"][i, j] += w * tp
                    ab["hcore"][i, j] += abs(w * tp)
                    kd["hcore"][i, j] += abs(w * tp) * kx
                    for x in range(3):
                        dsp = -2 * mu * AB[x] * sp
                        dtp = mu * (-4 * mu * AB[x] * sp + (3 - 2 * mu * r2) * dsp)
                        val["ipovlp"][x, i, j] += -w * dsp
                        ab["ipovlp"][x, i, j] += abs(w * dsp)
                        kd["ipovlp"][x, i, j] += abs(w * dsp) * kx
                        dH1[x, i, j] += w * dtp
                        adH1[x, i, j] += abs(w * dtp)
                        kdH1[x, i, j] += abs(w * dtp) * kx
                    for c in range(A):
                        PC = [P[x] - X[c][x] for x in range(3)]
                        t = p * sum(d * d for d in PC)
                        f0, f1 = boys(0, t), boys(1, t)
                        am = amp(t, f0)
                        pref = -Z[c] * (2 * mp.pi / p) * kab * w
                        val["hcore"][i, j] += pref * f0
                        ab["hcore"][i, j] += abs(pref * f0)
                        kd["hcore"][i, j] += abs(pref * f0) * kx
                        for x in range(3):
                            t0, t1 = pref * (-2 * mu * AB[x] * f0), pref * (-2 * a * PC[x] * f1)
                            dH1[x, i, j] += t0 + t1
                            adH1[x, i, j] += abs(t0) + abs(t1)
                            cdH1[x, i, j] += abs(pref * 2 * a * PC[x]) * am
                            kdH1[x, i, j] += (abs(t0) + abs(t1)) * kx + abs(pref * 2 * a * f1) * sP[x]
                            o = pref * f1 * 2 * p * PC[x]
                            val["dhcore"][c, x, i, j] += o
                            ab["dhcore"][c, x, i, j] += abs(o)
                            cc["dhcore"][c, x, i, j] += abs(pref * 2 * p * PC[x]) * am
                            kd["dhcore"][c, x, i, j] += abs(o) * kx + abs(pref * 2 * p * f1) * sP[x]
    for at in range(A):
        for arr, d in ((val["dhcore"], dH1), (ab["dhcore"], adH1), (cc["dhcore"], cdH1), (kd["dhcore"], kdH1)):
            arr[at, :, at, :] += d[:, at, :]
            arr[at, :, :, at] += d[:, at, :]
    for i in range(A):
        for j in range(A):
            if i == j:
                continue
            d = [X[i][x] - X[j][x] for x in range(3)]
            r = mp.sqrt(sum(v * v for v in d))
            if j > i:
                val["enuc"][()] += Z[i] * Z[j] / r
                ab["enuc"][()] += abs(Z[i] * Z[j] / r)
            for x in range(3):
                val["gnuc"][i, x] -= Z[i] * Z[j] * d[x] / r ** 3
                ab["gnuc"][i, x] += abs(Z[i] * Z[j] * d[x] / r ** 3)
    prim = [(i, ia) for i in range(n) for ia in range(K)]
    pairs = {(i, ia, j, ib): pair(i, j, ex[ia], ex[ib]) for i, ia in prim for j, ib in prim}
    two_pi_52 = 2 * mp.pi ** (mpf(5) / 2)
    for (i, ia, j, ib), (p, mu, AB, r2, kab, P, kx, sP) in pairs.items():
        wb = cn[ia] * cn[ib] * kab
        for (k, ic, l, id_), (q, _, _, _, kcd, Q, kxq, sQ) in pairs.items():
            rho = p * q / (p + q)
            PQ = [P[x] - Q[x] for x in range(3)]
            t = rho * sum(d * d for d in PQ)
            f0, f1 = boys(0, t), boys(1, t)
            am = amp(t, f0)
            w = two_pi_52 / (p * q * mp.sqrt(p + q)) * wb * cn[ic] * cn[id_] * kcd
            val["eri"][i, j, k, l] += w * f0
            ab["eri"][i, j, k, l] += abs(w * f0)
            kd["eri"][i, j, k, l] += abs(w * f0) * (kx + kxq)
            for x in range(3):
                c1 = w * 2 * rho * (ex[ia] / p) * PQ[x]
                t0, t1 = w * (-2 * mu * AB[x] * f0), -c1 * f1
                val["eri_ip1"][x, i, j, k, l] -= t0 + t1
                ab["eri_ip1"][x, i, j, k, l] += abs(t0) + abs(t1)
                cc["eri_ip1"][x, i, j, k, l] += abs(c1) * am
                kd["eri_ip1"][x, i, j, k, l] += (abs(t0) + abs(t1)) * (kx + kxq) + abs(w * 2 * rho * (ex[ia] / p) * f1) * (sP[x] + sQ[x])
    return {k: (val[k], ab[k], cc[k], kd[k]) for k in ref.NAMES}


def round_up24(x):
    """x >= 0 rounded up to 24 significant bits."""
    m, e = np.frexp(x)
    return np.ldexp(np.ceil(m * 2.0 ** 24) / 2.0 ** 24, e)


def pack(results):
    """Per-geometry results -> the arrays of one case."""
    out = {}
    for name in ref.NAMES:
        hi = np.array([np.vectorize(float, otypes=[np.float64])(r[name][0]) for r in results])
        lo = np.array([np.vectorize(lambda x: float(x - mpf(float(x))), otypes=[np.float64])(r[name][0]) for r in results])
        out[name + "_hi"], out[name + "_lo"] = hi, lo.astype(np.float32)
        sums = ([(1, "_abs")] + ([(2, "_cancel")] if name in ref.CANCEL_FIELDS else []) +
                ([(3, "_cond")] if name not in ("enuc", "gnuc") else []))
        for idx, tag in sums:
            exact = np.array([np.vectorize(float, otypes=[np.float64])(r[name][idx]) for r in results])
            assert not np.any((exact > 0.0) & (exact < 1e-290)), (name, tag, "a sum in the denormal range")
            out[name + tag] = round_up24(exact)
    return out


def main(argv):
    cases = ref.truth_cases()
    chosen = argv or sorted(cases)
    jobs = [(name, g) for name in chosen for g in range(len(cases[name][0]))]
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        res = pool.map(geometry, [(cases[n][0][g],) + tuple(cases[n][1:]) for n, g in jobs], chunksize=1)
    made = {}
    for name in chosen:
        R, Z, ex, co = cases[name]
        arrays = pack([r for (n, _), r in zip(jobs, res) if n == name])
        arrays.update(R=np.asarray(R, dtype=np.float64), Z=np.asarray(Z, dtype=np.float64),
                      ex=np.asarray(ex, dtype=np.float64), co=np.asarray(co, dtype=np.float64))
        made.update({f"{name}/{k}": v for k, v in arrays.items()})
    if not argv:
        np.savez_compressed(OUT, **made)
        print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(made)} arrays")
        return 0
    with np.load(OUT) as old:
        same = all(np.array_equal(old[k], v) and old[k].dtype == v.dtype for k, v in made.items())
    print(f"{', '.join(chosen)}: {'reproduces' if same else 'DIFFERS FROM'} {OUT}")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
