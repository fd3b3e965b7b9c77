"""Shared by the tests of ``evcont_amd.gto_spd`` / ``csrc/spdgto.hip``: the molecules several files use and the gates.

Measure: ``spgto_cases.scaled_diff``, max |x - ref| / max(1, max |ref|) per array.  Gates: the project's own
(tests/spgto_cases.py): ``DEVICE_HOST_GATE`` = 1e-10 for the device against the host statement; ``SP_GATE`` for the
general statement against ``sp_gaussian_mol`` on molecules of s and p shells by the rule of ``truth_gate``: 10 times the
measured difference (worst array: 1.7e-16 on STO-3G water, 3.0e-16 on 6-31G water, 1.5e-16 on case a of spgto_truth.npz;
the dipole integrals agree to the bit), at least 8e-15, at most 1e-10 -- so 8e-15."""
import os

import numpy as np

from evcont_amd.gto_spd import Shell
from spgto_cases import CEILING, DEVICE_HOST_GATE, NAMES, scaled_diff, unpack_eri, unpack_ip1     # noqa: F401

SP_MEASURED = 3.0e-16
SP_GATE = min(CEILING, max(10 * SP_MEASURED, 8e-15))


def spd_centre(a_s, a_p, a_d):
    """One centre of one-primitive s, p and d shells: 9 functions."""
    return [Shell(0, [a_s], [1.0]), Shell(1, [a_p], [1.0]), Shell(2, [a_d], [1.0])]


def two_centre():
    """Two s + p + d centres of one-primitive shells: N = 18, Ms = 171, the smallest shape whose kets span more than two
    blocks of 64.  -> (R (2,3), Z, shells)"""
    R = np.array([[0.0, 0.0, 0.0], [0.9, -0.6, 1.3]])
    return R, np.array([3.0, 2.0]), [spd_centre(1.1, 0.9, 0.8), spd_centre(0.7, 1.4, 0.5)]


def bent_three_centre():
    """A bent three-centre molecule, one centre with s + p + d and a d shell of two primitives, one with d + p, one with
    s alone: N = 18.  -> (R, Z, shells)"""
    R = np.array([[0.0, 0.0, 0.0], [0.3, 1.4, -0.2], [-1.1, 0.4, 0.9]])
    shells = [[Shell(0, [1.1], [1.0]), Shell(1, [0.9], [1.0]), Shell(2, [0.8, 0.3], [0.6, 0.5])],
              [Shell(0, [0.7], [1.0])],
              [Shell(2, [1.3], [1.0]), Shell(1, [0.5], [1.0])]]
    return R, np.array([3.0, 1.0, 2.0]), shells


def small_bent():
    """A bent three-centre molecule of one-primitive shells, s + p + d, s and d: N = 15, what the finite-difference test
    rebuilds six times.  -> (R, Z, shells)"""
    R = np.array([[0.0, 0.0, 0.0], [0.3, 1.4, -0.2], [-1.1, 0.4, 0.9]])
    return R, np.array([3.0, 1.0, 2.0]), [spd_centre(1.1, 0.9, 0.8), [Shell(0, [0.7], [1.0])], [Shell(2, [1.3], [1.0])]]


def limit_molecule():
    """Seven s + p + d centres (63 functions) and one s centre: N = 64, Ms = 2080, 22 shells, 128 primitives (s and p
    shells of eight, d shells of one, the d shell of centre 3 of two), primitive offsets up to the last shell."""
    rng = np.random.default_rng(5)
    ex8 = np.geomspace(0.15, 40.0, 8)
    co8 = np.array([0.3, 0.4, 0.5, 0.4, 0.3, 0.2, 0.1, 0.05])
    shells = []
    for c in range(7):
        d = Shell(2, [0.9, 0.35], [0.6, 0.5]) if c == 3 else Shell(2, [0.6 + 0.1 * c], [1.0])
        shells.append([Shell(0, ex8 * (1 + 0.05 * c), co8), Shell(1, ex8[::-1] * (0.5 + 0.03 * c), co8), d])
    shells.append([Shell(0, ex8 * 0.7, co8[::-1])])
    grid = np.array([[i, j, k] for i in range(2) for j in range(2) for k in range(2)], dtype=float)
    R = 2.2 * grid + 0.3 * rng.standard_normal((8, 3))
    Z = np.array([3.0, 1.0, 2.0, 1.0, 4.0, 1.0, 2.0, 1.0])
    return R, Z, shells


LIMIT_PAIRS = ((0, 7), (3, 7))        # pairs of centres of the limit shape held to the host statement


def limit_pair(atoms):
    """The limit molecule with functions on ``atoms`` alone, the other nuclei kept bare.  -> (R, Z, shells)"""
    R, Z, shells = limit_molecule()
    return R, Z, [shells[a] if a in atoms else [] for a in range(8)]


def eight_primitive_d():
    """A contracted d shell of eight primitives beside an s function: N = 6.  -> (R, Z, shells)"""
    ex8 = np.geomspace(0.2, 25.0, 8)
    shells = [[Shell(2, ex8, [0.1, 0.2, 0.3, 0.4, 0.4, 0.3, 0.2, 0.1])], [Shell(0, [0.8], [1.0])]]
    return np.array([[0.0, 0.0, 0.0], [0.7, -0.9, 1.2]]), np.array([2.0, 1.0]), shells


HOST_REFS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spdgto_host_refs.npz")


def boys_grid():
    """72 values of t from 0 to 1e5, the crossover at 12 included from both sides."""
    return np.concatenate([[0.0], np.geomspace(1e-6, 1e5, 64), [11.9, 11.999, 12.0 - 1e-9, 12.0, 12.001, 12.1, 40.0]])


def boys_grid_errors(nmax=9):
    """(nmax + 1,) worst relative error of ``gto_small.boys`` over ``boys_grid`` per order, against mpmath at 50
    digits."""
    from mpmath import mp, mpf
    from evcont_amd.gto_host import boys
    t = boys_grid()
    got = boys(nmax, t)
    worst = np.zeros(nmax + 1)
    with mp.workdps(50):
        for j, tj in enumerate(t):
            for n in range(nmax + 1):
                x = mpf(float(tj))
                ref = mpf(1) / (2 * n + 1) if x == 0 else mp.gammainc(n + mpf(1) / 2, 0, x) / (2 * x ** (n + mpf(1) / 2))
                worst[n] = max(worst[n], abs(float((mpf(float(got[n, j])) - ref) / ref)))
    return worst


# ---- the truth file ----------------------------------------------------------------------------------------------------
# tests/golden/spdgto_truth.npz (make_spdgto_truth.py: closed s forms differentiated with respect to the centres in
# mpmath, no Hermite expansion).  One-electron arrays, enuc, gnuc and the dipole integrals in full; eri and eri_ip1 as a
# sample (``eri_idx``: one element per class of shell types and case, with its three derivative directions).
TRUTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spdgto_truth.npz")
TRUTH_CASES = ("a", "b", "b_flat", "c", "d_lo", "d_hi")
TRUTH_FIELDS = ("enuc", "S", "hcore", "eri", "ipovlp", "dhcore", "eri_ip1", "gnuc", "dip")
TRUTH_FLOOR = 8e-16          # spgto_cases.DEVICE_RECORDED: the gate is at least ten times this
# max |host statement - truth| / max(1, max |truth|), in the order of TRUTH_FIELDS (printed by ``python tests/spdgto_cases.py``)
HOST_MEASURED = {
    #     enuc        S    hcore      eri   ipovlp   dhcore  eri_ip1     gnuc      dip
    "a": (1.4e-16, 2.2e-16, 2.7e-16, 3.2e-16, 6.7e-16, 7.9e-16, 3.8e-16, 1.6e-16, 2.1e-16),
    "b": (2.8e-17, 4.4e-16, 6.4e-16, 9.4e-18, 3.8e-16, 9.0e-16, 4.4e-17, 2.7e-16, 3.5e-16),
    "b_flat": (1.1e-16, 4.4e-16, 7.5e-16, 2.5e-18, 3.8e-16, 1.3e-15, 3.0e-17, 2.4e-16, 2.1e-16),
    "c": (6.3e-17, 8.9e-16, 1.3e-15, 1.9e-16, 1.9e-16, 2.1e-15, 3.9e-17, 1.1e-16, 3.3e-16),
    "d_lo": (1.0e-16, 4.4e-16, 5.4e-16, 2.4e-16, 2.6e-16, 7.7e-16, 2.1e-16, 1.7e-16, 4.1e-16),
    "d_hi": (1.0e-16, 4.4e-16, 7.9e-16, 2.4e-16, 2.6e-16, 7.3e-16, 2.1e-16, 2.0e-16, 4.1e-16),
}


def load_truth():
    with np.load(TRUTH) as z:
        return {k: z[k] for k in z.files}


def truth_shells(T, name):
    sa, sl, so, ex, co = (T[f"{name}/{k}"] for k in ("shell_atom", "shell_l", "shell_off", "ex", "co"))
    shells = [[] for _ in range(len(T[f"{name}/Z"]))]
    for s in range(len(sa)):
        shells[sa[s]].append(Shell(int(sl[s]), ex[so[s]:so[s + 1]], co[so[s]:so[s + 1]]))
    return shells


def truth_mol(T, name):
    """The case as a host molecule with the coefficients as they stand."""
    from evcont_amd.gto_spd import spd_gaussian_mol
    return spd_gaussian_mol(T[f"{name}/R"], T[f"{name}/Z"], truth_shells(T, name), renormalize=False)


def truth_err(x, T, name, field):
    """max |x - truth| / max(1, max |truth|) of one array (full form); eri and eri_ip1 over the sample of the file."""
    x = np.asarray(x, dtype=np.float64)
    hi, lo = T[f"{name}/{field}_hi"], T[f"{name}/{field}_lo"].astype(np.float64)
    if field in ("eri", "eri_ip1"):
        i = T[f"{name}/eri_idx"]
        x = x[i[:, 0], i[:, 1], i[:, 2], i[:, 3]] if field == "eri" else x[:, i[:, 0], i[:, 1], i[:, 2], i[:, 3]]
    return float(np.abs((x - hi) - lo).max() / max(1.0, np.abs(hi).max()))


def truth_gate(case, field):
    """The rule of ``spgto_cases.truth_gate``: ten times the host's measured error, at least 8e-15, at most 1e-10."""
    return min(CEILING, max(10 * HOST_MEASURED[case][TRUTH_FIELDS.index(field)], 10 * TRUTH_FLOOR))


def host_truth_errors(T, name):
    m = truth_mol(T, name)
    out = {f: truth_err(getattr(m, f), T, name, f) for f in NAMES}
    out["dip"] = truth_err(m.dipole_integrals(T[f"{name}/origin"]), T, name, "dip")
    return out


if __name__ == "__main__":
    T = load_truth()
    print("# " + " ".join(f"{f:>8s}" for f in TRUTH_FIELDS))
    for case in TRUTH_CASES:
        e = host_truth_errors(T, case)
        print(f'    "{case}": (' + ", ".join(f"{e[f]:.1e}" for f in TRUTH_FIELDS) + "),")
