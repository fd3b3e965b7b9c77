"""Generates tests/golden/spdfgto_truth.npz: arrays of ``gto_spdf.spdf_gaussian_mol`` / ``evc_spdfgto_integrals_batch``,
the dipole integrals and their gradient for molecules with real spherical f shells, WITHOUT McMurchie-Davidson, by the
method of tests/golden/make_spdgto_truth.py, whose closed forms, ``Jet`` arithmetic and assembly are imported: the
primitive s-type closed forms are evaluated once on truncated Taylor polynomials in the displaced centre coordinates
(mpmath, 40 digits), a Cartesian power is a short sum of centre derivatives of the s function,

    x^3 e^{-a r^2} = ((1/8a^3) d_x^3 + (3/4a^2) d_x) e^{-a r^2}

is the one addition, and the seven spherical combinations and the norm (2a/pi)^{3/4} (4a)^{3/2} are applied afterwards.
The total order of a derivative goes up to 13.

Stored as double-doubles, in the layout of spdgto_truth.npz: the one-electron arrays, ``enuc``, ``gnuc``, ``dip`` and
``ipdip`` in full; ``eri`` / ``eri_ip1`` as a sample (``sample``): one element of every class of shell types of the case
that contains an f shell, the components rotating so that every f component stands on every index position (asserted),
with all three derivative directions.  Case a, whose f shell has two primitives, stops at classes of two f shells, and
classes of three or four f shells take their f components from the four of one or two monomials.

Cases:
  a          three non-collinear centres: s + f (the f shell of two primitives), p + d, s
  b_flat     two centres with one coordinate coincident, s + p + f and d + f of one primitive each: EVERY class of shell
             types that contains an f shell
  c          f exponents 5000 and 0.1
  d_lo, d_hi (AA|BB) at t = 12 - 1e-3 and 12 + 1e-3 with f shells on both centres (the geometries of d_lo / d_hi of
             spdgto_truth.npz): the longest series of F13 and its least stable upward recursion

    python tests/golden/make_spdfgto_truth.py
"""
import itertools
import os
import sys
import time
from multiprocessing import Pool

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_spdgto_truth as base      # noqa: E402

mp.dps = 40
OUT = os.path.join(HERE, "spdfgto_truth.npz")
AT1, AT2 = base.AT1, base.AT2


def f_monomials():
    r24, r40, r60 = 1 / mp.sqrt(24), 1 / mp.sqrt(40), 1 / mp.sqrt(60)
    return ((((2, 1, 0), 3 * r24), ((0, 3, 0), -r24)),
            (((1, 1, 1), mpf(1)),),
            (((0, 1, 2), 4 * r40), ((2, 1, 0), -r40), ((0, 3, 0), -r40)),
            (((0, 0, 3), 2 * r60), ((2, 0, 1), -3 * r60), ((0, 2, 1), -3 * r60)),
            (((1, 0, 2), 4 * r40), ((3, 0, 0), -r40), ((1, 2, 0), -r40)),
            (((2, 0, 1), mpf(1) / 2), ((0, 2, 1), -mpf(1) / 2)),
            (((3, 0, 0), r24), ((1, 2, 0), -3 * r24)))


def cases():
    """name -> (R (A,3), Z (A,), shells per atom [(l, exponents, coefficients), ...], origin)."""
    fs = lambda e: [(3, (e,), (1.0,)), (0, (e,), (1.0,))]
    fp = lambda e: [(3, (e,), (1.0,)), (1, (e,), (1.0,))]
    return {
        "a": ([[0.1, -0.2, 0.05], [1.5, 0.3, -0.4], [-0.6, 1.4, 0.7]], [8.0, 1.0, 1.0],
              [[(0, (1.3,), (1.0,)), (3, (1.1, 0.45), (0.6, 0.5))], [(1, (0.9,), (1.0,)), (2, (0.8,), (1.0,))],
               [(0, (0.7,), (1.0,))]], (0.3, -0.1, 0.2)),
        "b_flat": ([[0.0, 0.4, 0.0], [2.1, 0.4, 0.9]], [3.0, 2.0],
                   [[(0, (3.0,), (1.0,)), (1, (3.0,), (1.0,)), (3, (3.0,), (1.0,))],
                    [(2, (2.2,), (1.0,)), (3, (2.2,), (1.0,))]], (0.0, 0.0, 0.0)),
        "c": ([[0.0, 0.0, 0.0], [0.7, -0.5, 0.9]], [8.0, 1.0], [fs(5000.0), fp(0.1)], (0.2, 0.0, -0.3)),
        "d_lo": ([[0.0, 0.0, 0.0], [1.5, 1.2, 1.0182724527]], [3.0, 2.0], [fs(3.0), fp(2.2)], (0.3, -0.1, 0.2)),
        "d_hi": ([[0.0, 0.0, 0.0], [1.5, 1.2, 1.0186592495]], [3.0, 2.0], [fs(3.0), fp(2.2)], (0.3, -0.1, 0.2)),
    }


CHEAP_F = (1, 5, 6, 0)       # f components of one or two monomials: xyz, z(x^2 - y^2), x(x^2 - 3y^2), y(3x^2 - y^2)
MAX_F = {"a": 2}              # case a has an f shell of two primitives: its classes stop at two f shells
EXTRA = {"d_lo": [(1, 1, 9, 9)], "d_hi": [(1, 1, 9, 9)]}      # (AA|BB), xyz on all four positions, at the crossover


def sample(name):
    """One element of every class of shell types of the case that contains an f shell (at most ``MAX_F`` of them), the
    components rotating over the positions; in classes of three or four f shells the f components are taken from
    ``CHEAP_F`` (a three-monomial component on every position costs 81 jets per primitive quartet)."""
    fn = functions(cases()[name][2])
    ls = sorted({f[1] for f in fn})
    by_l = {l: [i for i, f in enumerate(fn) if f[1] == l] for l in ls}
    out = []
    for count, cl in enumerate(itertools.product(ls, repeat=4)):
        nf = cl.count(3)
        if nf == 0 or nf > MAX_F.get(name, 4):
            continue
        el = []
        for pos, l in enumerate(cl):
            pool = by_l[l]
            if l == 3 and nf >= 3:
                pool = [i for i in pool if fn[i][2] in CHEAP_F]
            el.append(pool[(count * 7 + 3 * pos + count // 5) % len(pool)])
        out.append(tuple(el))
    return out + [e for e in EXTRA.get(name, []) if e not in out]


def operator(powers, e, first):
    terms = [(mpf(1), {})]
    for dim, n in enumerate(powers):
        per = {0: [(mpf(1), 0)], 1: [(1 / (2 * e), 1)], 2: [(1 / (4 * e * e), 2), (1 / (2 * e), 0)],
               3: [(1 / (8 * e ** 3), 3), (3 / (4 * e * e), 1)]}[n]
        terms = [(c0 * c1, {**o, **({first + dim: k} if k else {})}) for c0, o in terms for c1, k in per]
    return terms


def functions(shells):
    out = []
    for at, atom in enumerate(shells):
        for l, ex, co in atom:
            for comp in range(2 * l + 1):
                prims = []
                for e, k in zip(ex, co):
                    e = mpf(float(e))
                    norm = (2 * e / mp.pi) ** (mpf(3) / 4) * (1, 2 * mp.sqrt(e), 4 * e, 8 * e * mp.sqrt(e))[l]
                    prims.append((e, mpf(float(k)) * norm))
                mono = (((0, 0, 0), mpf(1)),) if l == 0 else \
                    ((tuple(int(comp == x) for x in range(3)), mpf(1)),) if l == 1 else \
                    base.d_monomials()[comp] if l == 2 else f_monomials()[comp]
                out.append((at, l, comp, mono, prims))
    return out


# the imported machinery reads these three through its module
base.cases, base.operator, base.functions = cases, operator, functions


def one_job(args):
    """``base.one_job`` and the gradient of the dipole integrals, <d_x mu| r_c - O_c |nu> = - d/dA_x."""
    name, mu, nu = args
    res = base.one_job(args)
    X, _, O, fn = base.setup(name)
    fns, where = (fn[mu], fn[nu]), (AT1["A"], AT1["B"])
    res["ipdip"] = [[-base.contracted(f"dip{c}", fns, X, where, (mpf(0),) * 3 + O, {AT1["A"] + x: 1}) for c in range(3)]
                    for x in range(3)]
    return res


def two_job(args):
    t = time.time()
    out = base.two_job(args)
    print(args, f"{time.time() - t:.0f} s", flush=True)
    return out


def main():
    ones, twos = [], []
    for name in cases():
        n = len(functions(cases()[name][2]))
        ones += [(name, mu, nu) for mu in range(n) for nu in range(n)]
        twos += [(name,) + e for e in sample(name)]
    print(f"{len(ones)} one-electron pairs, {len(twos)} two-electron elements", flush=True)
    fns = {name: functions(cases()[name][2]) for name in cases()}
    for pos in range(4):      # every f component stands on every index position
        assert {fns[e[0]][e[1 + pos]][2] for e in twos if fns[e[0]][e[1 + pos]][1] == 3} == set(range(7)), pos
    twos.sort(key=lambda e: -sum(len(fns[e[0]][i][3]) * len(fns[e[0]][i][4]) * (1 + fns[e[0]][i][1]) for i in e[1:]))
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        r2 = pool.map_async(two_job, twos, chunksize=1)
        r1 = pool.map(one_job, ones, chunksize=4)
        print("one-electron part done", flush=True)
        r2 = r2.get()
    made = {}
    for name in cases():
        rows = {(mu, nu): r for (nm, mu, nu), r in zip(ones, r1) if nm == name}
        arrays = base.assemble(name, rows)
        n = len(functions(cases()[name][2]))
        arrays["ipdip"] = np.full((3, 3, n, n), mpf(0), dtype=object)
        for (mu, nu), r in rows.items():
            for x in range(3):
                for c in range(3):
                    arrays["ipdip"][x, c, mu, nu] = r["ipdip"][x][c]
        idx = [e[1:] for e in twos if e[0] == name]
        two = [r for e, r in zip(twos, r2) if e[0] == name]
        packed = base.pack(name, arrays, idx, two)
        packed["ipdip_hi"], packed["ipdip_lo"] = base.double_double(arrays["ipdip"])
        made.update({f"{name}/{k}": v for k, v in packed.items()})
    np.savez_compressed(OUT, **made)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(made)} arrays")


if __name__ == "__main__":
    main()
