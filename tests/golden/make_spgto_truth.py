"""Generates tests/golden/spgto_truth.npz: the eight arrays of ``gto_small.sp_gaussian_mol`` /
``evc_spgto_integrals_batch`` and the dipole integrals, for molecules of s and p shells, WITHOUT McMurchie-Davidson:

  * the primitive s-type closed forms (overlap, kinetic energy, nuclear attraction, (ss|ss), and (P - O) S for the dipole)
    are written symbolically (sympy) with a function ``Boys(n, t)`` whose derivative in t is ``-Boys(n + 1, t)``;
  * a p component is ``(1 / 2a) d/dA_x`` of the s form, times the ratio of the primitive norms; a centre derivative is one
    more differentiation;
  * every expression is evaluated with mpmath at 40 digits, ``F_n(t) = gammainc(n + 1/2, 0, t) / (2 t^(n + 1/2))`` and
    ``F_n(0) = 1 / (2n + 1)``; the float64 inputs are taken as exact.

The tabulated coefficients are used as they stand (``renormalize=False``).  Per case the file holds the inputs (``R``, ``Z``,
``origin``, and the shells flattened: ``shell_atom``, ``shell_l``, ``shell_off``, ``ex``, ``co``) and per array
``<name>_hi`` / ``<name>_lo``, the value as a double-double (``lo`` as float32), as tests/golden/sgto_truth.npz does.
Cases:
  a          three non-collinear centres: s + p of two primitives, and two s of two primitives
  b, b_flat  two centres, both s + p of one primitive, with |P - Q| on both sides of the Boys crossover (t = 12) among
             the quartets; b_flat: the same with the centres coincident in one coordinate
  c          a tight and a diffuse centre (exponents 5000 and 0.1)
  d          12 Bohr apart: large t
  e_lo, e_hi the basis of b with the distance chosen so that t of the (AA|BB) quartets is 12 - 1e-3 and 12 + 1e-3: the
             longest series and the least stable upward recursion of the Boys scheme, side by side
The cases are kept in two files (FILES): spgto_truth.npz and, added later, spgto_truth_crossover.npz, so that new cases
never touch the stored bits of the old ones.  A few minutes on 16 processes.

    python tests/golden/make_spgto_truth.py [case ...]     # no argument: all cases, writes both files
                                                           # with arguments: recomputes those and compares with their file
    python tests/golden/make_spgto_truth.py --write spgto_truth_crossover.npz      # writes that file alone
    python tests/golden/make_spgto_truth.py --boys [case ...]   # prints t of every quartet class and attraction term
"""
import os
import sys
from functools import lru_cache
from multiprocessing import Pool

import numpy as np
import sympy as sp
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = {"spgto_truth.npz": ("a", "b", "b_flat", "c", "d"), "spgto_truth_crossover.npz": ("e_lo", "e_hi")}
mp.dps = 40
NAMES = ("enuc", "S", "hcore", "eri", "ipovlp", "dhcore", "eri_ip1", "gnuc", "dip")


def cases():
    """name -> (R (A,3), Z (A,), shells per atom [(l, exponents, coefficients), ...], origin)."""
    sp2 = lambda e, cs, cp: [(0, e, cs), (1, e, cp)]
    one = lambda e: sp2((e,), (1.0,), (1.0,))
    return {
        "a": ([[0.1, -0.2, 0.05], [1.5, 0.3, -0.4], [-0.6, 1.4, 0.7]], [8.0, 1.0, 1.0],
              [sp2((5.0331513, 0.380389), (0.3, 0.8), (0.45, 0.7)), [(0, (3.42525091, 0.1688554), (0.35, 0.75))],
               [(0, (1.3, 0.4), (0.5, 0.6))]], (0.3, -0.1, 0.2)),
        # exponents 3.0 and 2.2: t = rho |P - Q|^2 is 0 for the one-centre quartets, 2.8 for (AA|AB) and 14.1 for (AA|BB)
        "b": ([[0.0, 0.0, 0.0], [1.9, 1.2, 0.7]], [3.0, 2.0], [one(3.0), one(2.2)], (0.0, 0.0, 0.0)),
        "b_flat": ([[0.0, 0.4, 0.0], [2.1, 0.4, 0.9]], [3.0, 2.0], [one(3.0), one(2.2)], (0.0, 0.0, 0.0)),
        "c": ([[0.0, 0.0, 0.0], [0.7, -0.5, 0.9]], [8.0, 1.0], [one(5000.0), one(0.1)], (0.2, 0.0, -0.3)),
        "d": ([[0.0, 0.0, 0.0], [7.0, -8.0, 5.5677643628]], [1.0, 2.0], [one(1.1), one(0.6)], (0.0, 0.0, 0.0)),
        # (AA|BB): rho = 6.0 x 4.4 / 10.4, t = rho |A - B|^2 = 11.999000000 and 12.001000000 (--boys prints every class)
        "e_lo": ([[0.0, 0.0, 0.0], [1.5, 1.2, 1.0182724527]], [3.0, 2.0], [one(3.0), one(2.2)], (0.3, -0.1, 0.2)),
        "e_hi": ([[0.0, 0.0, 0.0], [1.5, 1.2, 1.0186592495]], [3.0, 2.0], [one(3.0), one(2.2)], (0.3, -0.1, 0.2)),
    }


class Boys(sp.Function):
    """F_n(t); d/dt F_n = -F_{n+1}."""
    nargs = 2

    def fdiff(self, argindex=2):
        if argindex != 2:
            raise sp.function.ArgumentIndexError(self, argindex)
        return -Boys(self.args[0] + 1, self.args[1])


def boys_mp(n, t):
    n = int(n)
    if t == 0:
        return mpf(1) / (2 * n + 1)
    return mp.gammainc(n + mpf(1) / 2, 0, t) / (2 * t ** (n + mpf(1) / 2))


a, b, c, d = sp.symbols("a b c d", positive=True)
CEN = {k: sp.symbols(f"{k}0:3", real=True) for k in "ABCDNO"}
EXPO = {"A": a, "B": b, "C": c, "D": d}
ARGS1 = (a, b) + CEN["A"] + CEN["B"] + CEN["N"] + CEN["O"]
ARGS2 = (a, b, c, d) + CEN["A"] + CEN["B"] + CEN["C"] + CEN["D"]


def _pair(x, y, X, Y):
    p = x + y
    r2 = sum((X[k] - Y[k]) ** 2 for k in range(3))
    return p, x * y / p, r2, [(x * X[k] + y * Y[k]) / p for k in range(3)]


def s_form(kind):
    """The closed form over unnormalised s primitives."""
    A, B, C, D, N, O = (CEN[k] for k in "ABCDNO")
    p, mu, r2, P = _pair(a, b, A, B)
    S = (sp.pi / p) ** sp.Rational(3, 2) * sp.exp(-mu * r2)
    if kind == "S":
        return S
    if kind == "T":
        return mu * (3 - 2 * mu * r2) * S
    if kind == "V":      # unit charge at N
        return -2 * sp.pi / p * sp.exp(-mu * r2) * Boys(0, p * sum((P[k] - N[k]) ** 2 for k in range(3)))
    if kind.startswith("dip"):
        k = int(kind[3])
        return (P[k] - O[k]) * S
    q, nu, s2, Q = _pair(c, d, C, D)
    return (2 * sp.pi ** sp.Rational(5, 2) / (p * q * sp.sqrt(p + q)) * sp.exp(-mu * r2 - nu * s2)
            * Boys(0, p * q / (p + q) * sum((P[k] - Q[k]) ** 2 for k in range(3))))


@lru_cache(maxsize=None)
def compiled(kind, dirs, der):
    """The integral ``kind`` over primitives with the p directions ``dirs`` (per centre letter: -1 = s, else 0, 1, 2),
    differentiated once more by ``der`` = (centre letter, x) or None, as an mpmath function of ARGS1 / ARGS2."""
    e = s_form(kind)
    for letter, x in dirs:
        if x >= 0:
            e = sp.diff(e, CEN[letter][x]) / (2 * EXPO[letter])
    if der is not None:
        e = sp.diff(e, CEN[der[0]][der[1]])
    return sp.lambdify(ARGS2 if kind == "eri" else ARGS1, e, modules=[{"Boys": boys_mp}, "mpmath"], cse=True)


def functions(shells):
    """Per AO: (atom, direction, [(exponent, coefficient x primitive norm), ...]); AO order atoms, shells, x y z."""
    out = []
    for at, atom in enumerate(shells):
        for l, ex, co in atom:
            for comp in range(2 * l + 1):
                prims = []
                for e, k in zip(ex, co):
                    e = mpf(float(e))
                    norm = (2 * e / mp.pi) ** (mpf(3) / 4) * (2 * mp.sqrt(e) if l == 1 else 1)
                    prims.append((e, mpf(float(k)) * norm))
                out.append((at, comp if l == 1 else -1, prims))
    return out


def row_job(args):
    """Everything of one ordered AO pair (mu, nu) of one case."""
    name, mu, nu = args
    R, Z, shells, origin = cases()[name]
    X = [[mpf(float(v)) for v in r] for r in R]
    Zm = [mpf(float(z)) for z in Z]
    O = [mpf(float(v)) for v in origin]
    fn = functions(shells)
    n, A = len(fn), len(R)
    am, dm, pm = fn[mu]
    an, dn, pn = fn[nu]
    dirs1 = (("A", dm), ("B", dn))
    zero = lambda *s: np.full(s, mpf(0), dtype=object)
    res = {"S": mpf(0), "T": mpf(0), "V": mpf(0), "dS": zero(3), "dH": zero(3), "op": zero(A, 3), "dip": zero(3),
           "eri": zero(n, n), "ip1": zero(3, n, n)}
    for ea, wa in pm:
        for eb, wb in pn:
            w = wa * wb
            base = (ea, eb) + tuple(X[am]) + tuple(X[an])
            nowhere = (mpf(0),) * 3
            res["S"] += w * compiled("S", dirs1, None)(*base, *nowhere, *O)
            res["T"] += w * compiled("T", dirs1, None)(*base, *nowhere, *O)
            for k in range(3):
                res["dip"][k] += w * compiled(f"dip{k}", dirs1, None)(*base, *nowhere, *O)
                res["dS"][k] += w * compiled("S", dirs1, ("A", k))(*base, *nowhere, *O)
                res["dH"][k] += w * compiled("T", dirs1, ("A", k))(*base, *nowhere, *O)
            for at in range(A):
                res["V"] += w * Zm[at] * compiled("V", dirs1, None)(*base, *X[at], *O)
                for k in range(3):
                    res["dH"][k] += w * Zm[at] * compiled("V", dirs1, ("A", k))(*base, *X[at], *O)
                    res["op"][at, k] += w * Zm[at] * compiled("V", dirs1, ("N", k))(*base, *X[at], *O)
    for ka in range(n):
        for la in range(ka + 1):
            ak, dk, pk = fn[ka]
            al, dl, pl = fn[la]
            dirs2 = dirs1 + (("C", dk), ("D", dl))
            fs = [compiled("eri", dirs2, None)] + [compiled("eri", dirs2, ("A", k)) for k in range(3)]
            acc = [mpf(0)] * 4
            for ea, wa in pm:
                for eb, wb in pn:
                    for ec, wc in pk:
                        for ed, wd in pl:
                            argv = (ea, eb, ec, ed) + tuple(X[am]) + tuple(X[an]) + tuple(X[ak]) + tuple(X[al])
                            w = wa * wb * wc * wd
                            for i in range(4):
                                acc[i] += w * fs[i](*argv)
            res["eri"][ka, la] = res["eri"][la, ka] = acc[0]
            for k in range(3):
                res["ip1"][k, ka, la] = res["ip1"][k, la, ka] = -acc[1 + k]      # electron gradient = - centre gradient
    return res


def assemble(name, rows):
    R, Z, shells, origin = cases()[name]
    fn = functions(shells)
    n, A = len(fn), len(R)
    zero = lambda *s: np.full(s, mpf(0), dtype=object)
    out = {"enuc": zero(), "S": zero(n, n), "hcore": zero(n, n), "eri": zero(n, n, n, n), "ipovlp": zero(3, n, n),
           "dhcore": zero(A, 3, n, n), "eri_ip1": zero(3, n, n, n, n), "gnuc": zero(A, 3), "dip": zero(3, n, n)}
    for (mu, nu), r in rows.items():
        out["S"][mu, nu] = r["S"]
        out["hcore"][mu, nu] = r["T"] + r["V"]
        out["eri"][mu, nu] = r["eri"]
        out["eri_ip1"][:, mu, nu] = r["ip1"]
        out["dip"][:, mu, nu] = r["dip"]
        out["ipovlp"][:, mu, nu] = -r["dS"]
        out["dhcore"][:, :, mu, nu] += r["op"]
        # the functions of an atom move with it: dH of (mu, nu) is the row term of (mu, nu) and the column term of (nu, mu)
        out["dhcore"][fn[mu][0], :, mu, nu] += r["dH"]
        out["dhcore"][fn[mu][0], :, nu, mu] += r["dH"]
    X = [[mpf(float(v)) for v in r] for r in R]
    for i in range(A):
        for j in range(A):
            if i == j:
                continue
            dv = [X[i][k] - X[j][k] for k in range(3)]
            r = mp.sqrt(sum(v * v for v in dv))
            zz = mpf(float(Z[i])) * mpf(float(Z[j]))
            if j > i:
                out["enuc"][()] += zz / r
            for k in range(3):
                out["gnuc"][i, k] -= zz * dv[k] / r ** 3
    return out


def pack(name, arrays):
    R, Z, shells, origin = cases()[name]
    out = {"R": np.asarray(R, dtype=np.float64), "Z": np.asarray(Z, dtype=np.float64),
           "origin": np.asarray(origin, dtype=np.float64)}
    flat = [(at, l, ex, co) for at, atom in enumerate(shells) for l, ex, co in atom]
    out["shell_atom"] = np.array([f[0] for f in flat], dtype=np.int32)
    out["shell_l"] = np.array([f[1] for f in flat], dtype=np.int32)
    out["shell_off"] = np.concatenate([[0], np.cumsum([len(f[2]) for f in flat])]).astype(np.int32)
    out["ex"] = np.concatenate([np.asarray(f[2], dtype=np.float64) for f in flat])
    out["co"] = np.concatenate([np.asarray(f[3], dtype=np.float64) for f in flat])
    for k in NAMES:
        out[k + "_hi"] = np.vectorize(float, otypes=[np.float64])(arrays[k])
        out[k + "_lo"] = np.vectorize(lambda x: float(x - mpf(float(x))), otypes=[np.float64])(arrays[k]).astype(np.float32)
    return out


def boys_arguments(name):
    """{label: t} of every class of primitive quartets (t = rho |P - Q|^2) and of every nuclear-attraction term
    (t = p |P - C|^2) of a case; a class is a pair of shell pairs, since the primitives of a shell share their centre."""
    R, Z, shells, origin = cases()[name]
    prims = [(at, s, k, float(e)) for at, atom in enumerate(shells) for s, (l, ex, co) in enumerate(atom)
             for k, e in enumerate(ex)]
    R = np.asarray(R, dtype=np.float64)
    pairs = {}
    for i, (ai, si, ki, ea) in enumerate(prims):
        for aj, sj, kj, eb in prims[:i + 1]:
            pairs[f"{ai}.{si}.{ki} {aj}.{sj}.{kj}"] = (ea + eb, (ea * R[ai] + eb * R[aj]) / (ea + eb))
    out = {}
    for kb, (p, P) in pairs.items():
        for c in range(len(Z)):
            out[f"<{kb}| 1/r_{c}"] = p * float(np.sum((P - R[c]) ** 2))
        for kk, (q, Q) in pairs.items():
            out[f"({kb}|{kk})"] = p * q / (p + q) * float(np.sum((P - Q) ** 2))
    return out


def main(argv):
    if argv[:1] == ["--boys"]:
        for name in argv[1:] or sorted(cases()):
            seen = {}
            for label, t in boys_arguments(name).items():
                seen.setdefault(round(t, 9), label)
            print(f"{name}: t of the distinct classes (atom.shell.primitive; the first of each value)")
            for t in sorted(seen):
                print(f"    t = {t:16.9f}   {seen[t]}")
        return 0
    only = None
    if argv[:1] == ["--write"]:
        only, argv = argv[1], []
        chosen = list(FILES[only])
    else:
        chosen = argv or sorted(cases())
    where = {name: os.path.join(HERE, f) for f, names in FILES.items() for name in names}
    jobs = []
    for name in chosen:
        n = len(functions(cases()[name][2]))
        jobs += [(name, mu, nu) for mu in range(n) for nu in range(n)]
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        res = pool.map(row_job, jobs, chunksize=1)
    made = {}
    for name in chosen:
        rows = {(mu, nu): r for (nm, mu, nu), r in zip(jobs, res) if nm == name}
        made.update({f"{name}/{k}": v for k, v in pack(name, assemble(name, rows)).items()})
    if not argv:
        for f, names in FILES.items():
            if only not in (None, f):
                continue
            part = {k: v for k, v in made.items() if k.split("/")[0] in names}
            np.savez_compressed(os.path.join(HERE, f), **part)
            print(f"wrote {f}: {os.path.getsize(os.path.join(HERE, f))} bytes, {len(part)} arrays")
        return 0
    status = 0
    for name in chosen:
        with np.load(where[name]) as old:
            same = all(np.array_equal(old[k], v) and old[k].dtype == v.dtype for k, v in made.items()
                       if k.split("/")[0] == name)
        print(f"{name}: {'reproduces' if same else 'DIFFERS FROM'} {os.path.basename(where[name])}")
        status |= 0 if same else 1
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
