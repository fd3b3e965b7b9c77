"""Generates tests/golden/spdgto_truth.npz: the arrays of ``gto_spd.spd_gaussian_mol`` / ``evc_spdgto_integrals_batch``
and the dipole integrals for molecules with real spherical d shells, WITHOUT McMurchie-Davidson (no Hermite expansion,
no ``E``, no ``R_tuv``):

  * the primitive s-type closed forms and ``Boys`` are those of tests/golden/make_spgto_truth.py, imported unchanged
    (sympy expressions; ``F_n(t) = gammainc(n + 1/2, 0, t) / (2 t^(n + 1/2))`` in mpmath);
  * Cartesian powers come in as derivatives of the s form with respect to the centre:
        x   e^{-a r^2} = (1/2a) d_x                  e^{-a r^2}
        x^2 e^{-a r^2} = ((1/4a^2) d_x^2 + 1/2a)     e^{-a r^2}
    per dimension, so a monomial is a short sum of mixed derivatives; the derivative for the centre of the first function
    is one more d_x.  The spherical combination (xy, yz, (2z^2 - x^2 - y^2)/sqrt(12), xz, (x^2 - y^2)/2) and the norms are
    applied afterwards;
  * the mixed derivatives (total order up to 9) come from evaluating the closed form ONCE on truncated Taylor
    polynomials in the displaced centre coordinates (``Jet``: exact polynomial arithmetic in mpmath at 40 digits;
    ``exp`` by its series, ``Boys`` by d^k F_n / dt^k = (-1)^k F_{n+k}): d^alpha f = alpha! c[alpha].  One sixth-order
    derivative of the (ss|ss) form was compared with mpmath's numerical ``diff``: relative difference 2e-41.  The float64 inputs are taken as exact.

The one-electron arrays, ``enuc``, ``gnuc`` and the dipole integrals are stored in full.  ``eri`` and ``eri_ip1`` are
stored as a SAMPLE: per case one element of every class of shell types (ss|ss) ... (dd|dd) that the case has, the
components rotating so that every d component stands on every index position, with all three derivative directions:
``eri_idx`` (K,4), ``eri_hi/lo`` (K,), ``eri_ip1_hi/lo`` (3,K).  Values are double-doubles (``lo`` as float32), the
inputs are stored as in spgto_truth.npz.  The tabulated coefficients are used as they stand (``renormalize=False``).

Cases:
  a          three non-collinear centres, one with s + p + d and a d shell of two primitives
  b, b_flat  two s + p + d centres of one primitive each (exponents 3.0 and 2.2): t = 0, 2.8 and 14.1 among the
             quartets; b_flat: one coordinate coincident
  c          exponents 5000 and 0.1 on d shells
  d_lo, d_hi (AA|BB) at t = 12 - 1e-3 and 12 + 1e-3 with d shells on both centres (the geometries of e_lo / e_hi of
             spgto_truth_crossover.npz): the longest series of F9 and its least stable upward recursion

    python tests/golden/make_spdgto_truth.py [case ...]      # no argument: all cases, writes the file
"""
import itertools
import os
import sys
from multiprocessing import Pool

import numpy as np
import sympy as sp
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_spgto_truth import ARGS1, ARGS2, boys_mp, s_form      # noqa: E402  (the closed forms and Boys, unchanged)

mp.dps = 40
OUT = os.path.join(HERE, "spdgto_truth.npz")
FULL = ("enuc", "S", "hcore", "ipovlp", "dhcore", "gnuc", "dip")
# first argument index of a centre's coordinates in ARGS1 / ARGS2
AT1 = {"A": 2, "B": 5, "N": 8, "O": 11}
AT2 = {"A": 4, "B": 7, "C": 10, "D": 13}


def d_monomials():
    r3, r12 = 1 / mp.sqrt(3), 1 / mp.sqrt(12)
    return ((((1, 1, 0), mpf(1)),), (((0, 1, 1), mpf(1)),), (((0, 0, 2), r3), ((2, 0, 0), -r12), ((0, 2, 0), -r12)),
            (((1, 0, 1), mpf(1)),), (((2, 0, 0), mpf(1) / 2), ((0, 2, 0), -mpf(1) / 2)))


def cases():
    """name -> (R (A,3), Z (A,), shells per atom [(l, exponents, coefficients), ...], origin)."""
    spd = lambda e: [(0, (e,), (1.0,)), (1, (e,), (1.0,)), (2, (e,), (1.0,))]
    ds = lambda e: [(2, (e,), (1.0,)), (0, (e,), (1.0,))]
    dp = lambda e: [(2, (e,), (1.0,)), (1, (e,), (1.0,))]
    return {
        "a": ([[0.1, -0.2, 0.05], [1.5, 0.3, -0.4], [-0.6, 1.4, 0.7]], [8.0, 1.0, 1.0],
              [[(0, (5.0331513, 0.380389), (0.3, 0.8)), (1, (1.1695961,), (1.0,)), (2, (1.185, 0.4), (0.7, 0.45))],
               [(0, (3.42525091, 0.1688554), (0.35, 0.75))], [(0, (1.3,), (1.0,))]], (0.3, -0.1, 0.2)),
        "b": ([[0.0, 0.0, 0.0], [1.9, 1.2, 0.7]], [3.0, 2.0], [spd(3.0), spd(2.2)], (0.0, 0.0, 0.0)),
        "b_flat": ([[0.0, 0.4, 0.0], [2.1, 0.4, 0.9]], [3.0, 2.0], [spd(3.0), spd(2.2)], (0.0, 0.0, 0.0)),
        "c": ([[0.0, 0.0, 0.0], [0.7, -0.5, 0.9]], [8.0, 1.0], [ds(5000.0), dp(0.1)], (0.2, 0.0, -0.3)),
        "d_lo": ([[0.0, 0.0, 0.0], [1.5, 1.2, 1.0182724527]], [3.0, 2.0], [ds(3.0), dp(2.2)], (0.3, -0.1, 0.2)),
        "d_hi": ([[0.0, 0.0, 0.0], [1.5, 1.2, 1.0186592495]], [3.0, 2.0], [ds(3.0), dp(2.2)], (0.3, -0.1, 0.2)),
    }


class Jet:
    """A truncated Taylor polynomial in the displacements h_i of some arguments: ``c[alpha]`` is the coefficient of
    prod h_i^alpha_i, alpha_i < shape_i (an object array of mpf).  The closed forms are evaluated on jets, so ONE
    evaluation gives every mixed derivative up to the orders wanted: d^alpha f = alpha! c[alpha]."""
    __slots__ = ("c",)

    def __init__(self, c):
        self.c = c

    def lift(self, x):
        c = np.full(self.c.shape, mpf(0), dtype=object)
        c[(0,) * c.ndim] = x
        return Jet(c)

    def __add__(self, o):
        if isinstance(o, Jet):
            return Jet(self.c + o.c)
        c = self.c.copy()
        c[(0,) * c.ndim] += o
        return Jet(c)

    __radd__ = __add__

    def __neg__(self):
        return Jet(-self.c)

    def __sub__(self, o):
        return self + (-o)

    def __rsub__(self, o):
        return (-self) + o

    def __mul__(self, o):
        if not isinstance(o, Jet):
            return Jet(self.c * o)
        a, b = self.c, o.c
        out = np.full(a.shape, mpf(0), dtype=object)
        for idx in zip(*np.nonzero(a != 0)):
            src = tuple(slice(0, n - i) for n, i in zip(a.shape, idx))
            dst = tuple(slice(i, None) for i in idx)
            out[dst] += b[src] * a[idx]
        return Jet(out)

    __rmul__ = __mul__

    def __truediv__(self, o):           # by a number
        return Jet(self.c / o)

    def __pow__(self, n):
        r = self
        for _ in range(int(n) - 1):
            r = r * self
        return r

    def split(self):
        """(value, the jet without it, the highest total degree)."""
        c0 = self.c[(0,) * self.c.ndim]
        return c0, self + (-c0), sum(n - 1 for n in self.c.shape)


def jexp(x):
    if not isinstance(x, Jet):
        return mp.exp(x)
    c0, d, K = x.split()
    res = term = x.lift(mpf(1))
    for k in range(1, K + 1):
        term = term * d / k
        res = res + term
    return res * mp.exp(c0)


def jboys(n, t):
    """F_n of a jet by its Taylor series in t: d^k F_n / dt^k = (-1)^k F_{n+k}."""
    if not isinstance(t, Jet):
        return boys_mp(n, t)
    t0, d, K = t.split()
    res, term = t.lift(boys_mp(n, t0)), t.lift(mpf(1))
    for k in range(1, K + 1):
        term = term * d / k
        res = res + term * ((-1) ** k * boys_mp(n + k, t0))
    return res


_NUMERIC, _CACHE = {}, {}


def numeric(kind):
    if kind not in _NUMERIC:
        _NUMERIC[kind] = sp.lambdify(ARGS2 if kind == "eri" else ARGS1, s_form(kind),
                                     modules=[{"Boys": jboys, "exp": jexp}, "mpmath"])
    return _NUMERIC[kind]


def jet(kind, args, highest):
    """The s form ``kind`` at ``args`` (mpf) as a jet in the arguments of ``highest`` = ((argument index, order), ...)."""
    key = (kind, args, highest)
    if key not in _CACHE:
        if len(_CACHE) > 64:
            _CACHE.clear()
        full, shape = list(args), tuple(n + 1 for _, n in highest)
        for pos, (i, _) in enumerate(highest):
            c = np.full(shape, mpf(0), dtype=object)
            c[(0,) * len(shape)] = args[i]
            c[tuple(int(q == pos) for q in range(len(shape)))] = mpf(1)
            full[i] = Jet(c)
        _CACHE[key] = numeric(kind)(*full)
    return _CACHE[key]


def deriv(kind, args, orders, highest):
    """The mixed derivative ``orders`` ({argument index: order}) from the jet of the orders ``highest``."""
    if not highest:
        return jet(kind, args, highest)
    alpha = tuple(orders.get(i, 0) for i, _ in highest)
    fact = mpf(1)
    for k in alpha:
        fact *= mp.factorial(k)
    return fact * jet(kind, args, highest).c[alpha]


def operator(powers, e, first):
    """x^i y^j z^k e^{-e r^2} as [(coefficient, {argument index: order})] acting on the s function; ``first``: the
    argument index of the centre's x."""
    terms = [(mpf(1), {})]
    for dim, n in enumerate(powers):
        per = {0: [(mpf(1), 0)], 1: [(1 / (2 * e), 1)], 2: [(1 / (4 * e * e), 2), (1 / (2 * e), 0)]}[n]
        terms = [(c0 * c1, {**o, **({first + dim: k} if k else {})}) for c0, o in terms for c1, k in per]
    return terms


def functions(shells):
    """Per AO: (atom, l, component, [(powers, weight)], [(exponent, coefficient x primitive norm)])."""
    out = []
    for at, atom in enumerate(shells):
        for l, ex, co in atom:
            for comp in range(2 * l + 1):
                prims = []
                for e, k in zip(ex, co):
                    e = mpf(float(e))
                    norm = (2 * e / mp.pi) ** (mpf(3) / 4) * (1, 2 * mp.sqrt(e), 4 * e)[l]
                    prims.append((e, mpf(float(k)) * norm))
                mono = (((0, 0, 0), mpf(1)),) if l == 0 else \
                    ((tuple(int(comp == x) for x in range(3)), mpf(1)),) if l == 1 else d_monomials()[comp]
                out.append((at, l, comp, mono, prims))
    return out


def contracted(kind, fns, X, where, tail, extra=None):
    """sum over primitives, monomials and operator terms of the functions ``fns`` (on the centre letters of ``where``) of
    the s form ``kind``, with the derivative orders ``extra`` added; ``tail``: the remaining arguments (N, O)."""
    total = mpf(0)
    for prims in itertools.product(*[f[4] for f in fns]):
        exps = tuple(e for e, _ in prims)
        args = exps + tuple(v for f in fns for v in X[f[0]]) + tail
        wp = mpf(1)
        for _, w in prims:
            wp *= w
        for monos in itertools.product(*[f[3] for f in fns]):
            wm = wp
            for _, w in monos:
                wm *= w
            ops = [operator(m[0], e, where[i]) for i, (m, e) in enumerate(zip(monos, exps))]
            top = dict(extra or {})
            for i, (m, _) in enumerate(monos):
                for dim, n in enumerate(m):
                    if n:
                        top[where[i] + dim] = top.get(where[i] + dim, 0) + n
            highest = tuple(sorted(top.items()))
            for combo in itertools.product(*ops):
                coef, orders = wm, dict(extra or {})
                for c, o in combo:
                    coef *= c
                    for i, n in o.items():
                        orders[i] = orders.get(i, 0) + n
                total += coef * deriv(kind, args, orders, highest)
    return total


def setup(name):
    R, Z, shells, origin = cases()[name]
    X = [tuple(mpf(float(v)) for v in r) for r in R]
    return X, [mpf(float(z)) for z in Z], tuple(mpf(float(v)) for v in origin), functions(shells)


def one_job(args):
    """The one-electron quantities of one ordered AO pair (mu, nu) of one case."""
    name, mu, nu = args
    X, Zm, O, fn = setup(name)
    A = len(X)
    fns, where = (fn[mu], fn[nu]), (AT1["A"], AT1["B"])
    nowhere = (mpf(0),) * 3
    q = lambda kind, N=nowhere, extra=None: contracted(kind, fns, X, where, tuple(N) + O, extra)
    res = {"S": q("S"), "T": q("T"), "V": mpf(0), "dS": [mpf(0)] * 3, "dH": [mpf(0)] * 3,
           "op": [[mpf(0)] * 3 for _ in range(A)], "dip": [q(f"dip{k}") for k in range(3)]}
    for k in range(3):
        res["dS"][k] = q("S", extra={AT1["A"] + k: 1})
        res["dH"][k] = q("T", extra={AT1["A"] + k: 1})
    for at in range(A):
        res["V"] += Zm[at] * q("V", X[at])
        for k in range(3):
            res["dH"][k] += Zm[at] * q("V", X[at], {AT1["A"] + k: 1})
            res["op"][at][k] = Zm[at] * q("V", X[at], {AT1["N"] + k: 1})
    return res


def two_job(args):
    """(value, the three electron-gradient components for the first index) of one element of eri."""
    name, mu, nu, ka, la = args
    X, _, _, fn = setup(name)
    fns, where = (fn[mu], fn[nu], fn[ka], fn[la]), (AT2["A"], AT2["B"], AT2["C"], AT2["D"])
    val = contracted("eri", fns, X, where, ())
    return val, [-contracted("eri", fns, X, where, (), {AT2["A"] + k: 1}) for k in range(3)]


def sample(name):
    """One element per class of shell types, components rotating over the positions."""
    fn = functions(cases()[name][2])
    by_l = {l: [i for i, f in enumerate(fn) if f[1] == l] for l in (0, 1, 2)}
    out = []
    for count, ls in enumerate(itertools.product((0, 1, 2), repeat=4)):
        if any(not by_l[l] for l in ls):
            continue
        out.append(tuple(by_l[l][(count * 7 + 3 * pos + count // 5) % len(by_l[l])] for pos, l in enumerate(ls)))
    return out


def assemble(name, rows):
    X, Zm, _, fn = setup(name)
    n, A = len(fn), len(X)
    zero = lambda *s: np.full(s, mpf(0), dtype=object)
    out = {"enuc": zero(), "S": zero(n, n), "hcore": zero(n, n), "ipovlp": zero(3, n, n), "dhcore": zero(A, 3, n, n),
           "gnuc": zero(A, 3), "dip": zero(3, n, n)}
    for (mu, nu), r in rows.items():
        out["S"][mu, nu] = r["S"]
        out["hcore"][mu, nu] = r["T"] + r["V"]
        for k in range(3):
            out["dip"][k, mu, nu] = r["dip"][k]
            out["ipovlp"][k, mu, nu] = -r["dS"][k]
            for at in range(A):
                out["dhcore"][at, k, mu, nu] += r["op"][at][k]
            # the functions of an atom move with it: the row term of (mu, nu) and the column term of (nu, mu)
            out["dhcore"][fn[mu][0], k, mu, nu] += r["dH"][k]
            out["dhcore"][fn[mu][0], k, nu, mu] += r["dH"][k]
    for i in range(A):
        for j in range(A):
            if i == j:
                continue
            dv = [X[i][k] - X[j][k] for k in range(3)]
            r = mp.sqrt(sum(v * v for v in dv))
            if j > i:
                out["enuc"][()] += Zm[i] * Zm[j] / r
            for k in range(3):
                out["gnuc"][i, k] -= Zm[i] * Zm[j] * dv[k] / r ** 3
    return out


def double_double(arr):
    hi = np.vectorize(float, otypes=[np.float64])(arr)
    lo = np.vectorize(lambda x: float(x - mpf(float(x))), otypes=[np.float64])(arr).astype(np.float32)
    return hi, lo


def pack(name, arrays, idx, two):
    R, Z, shells, origin = cases()[name]
    out = {"R": np.asarray(R, dtype=np.float64), "Z": np.asarray(Z, dtype=np.float64),
           "origin": np.asarray(origin, dtype=np.float64)}
    flat = [(at, l, ex, co) for at, atom in enumerate(shells) for l, ex, co in atom]
    out["shell_atom"] = np.array([f[0] for f in flat], dtype=np.int32)
    out["shell_l"] = np.array([f[1] for f in flat], dtype=np.int32)
    out["shell_off"] = np.concatenate([[0], np.cumsum([len(f[2]) for f in flat])]).astype(np.int32)
    out["ex"] = np.concatenate([np.asarray(f[2], dtype=np.float64) for f in flat])
    out["co"] = np.concatenate([np.asarray(f[3], dtype=np.float64) for f in flat])
    for k in FULL:
        out[k + "_hi"], out[k + "_lo"] = double_double(arrays[k])
    out["eri_idx"] = np.array(idx, dtype=np.int32).reshape(-1, 4)
    out["eri_hi"], out["eri_lo"] = double_double(np.array([v for v, _ in two], dtype=object))
    out["eri_ip1_hi"], out["eri_ip1_lo"] = double_double(np.array([[g[k] for _, g in two] for k in range(3)], dtype=object))
    return out


def main(argv):
    chosen = argv or list(cases())
    ones, twos = [], []
    for name in chosen:
        n = len(functions(cases()[name][2]))
        ones += [(name, mu, nu) for mu in range(n) for nu in range(n)]
        twos += [(name,) + e for e in sample(name)]
    print(f"{len(ones)} one-electron pairs, {len(twos)} two-electron elements", flush=True)
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        twos.sort(key=lambda e: -sum(functions(cases()[e[0]][2])[i][1] for i in e[1:]))      # the dear ones first
        r2 = pool.map_async(two_job, twos, chunksize=1)
        r1 = pool.map(one_job, ones, chunksize=4)
        print("one-electron part done", flush=True)
        r2 = r2.get()
    made = {}
    for name in chosen:
        rows = {(mu, nu): r for (nm, mu, nu), r in zip(ones, r1) if nm == name}
        idx = [e[1:] for e in twos if e[0] == name]
        two = [r for e, r in zip(twos, r2) if e[0] == name]
        made.update({f"{name}/{k}": v for k, v in pack(name, assemble(name, rows), idx, two).items()})
    if argv:
        with np.load(OUT) as old:
            for name in chosen:
                same = all(np.array_equal(old[k], v) for k, v in made.items() if k.split("/")[0] == name)
                print(f"{name}: {'reproduces' if same else 'DIFFERS FROM'} {os.path.basename(OUT)}")
        return 0
    np.savez_compressed(OUT, **made)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(made)} arrays")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
