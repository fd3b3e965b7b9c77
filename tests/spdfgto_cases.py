"""Shared by the tests of ``evcont_amd.gto_spdf`` / ``csrc/spdfgto.hip``: the molecules several files use and the gates.

Measure: ``spgto_cases.scaled_diff``, max |x - ref| / max(1, max |ref|) per array.  Gates: the project's own
(tests/spgto_cases.py, tests/spdgto_cases.py): ``DEVICE_HOST_GATE`` = 1e-10 for the device against the host statement;
``SPD_GATE`` for ``evc_spdfgto_*`` against ``evc_spdgto_*`` on a molecule with l <= 2 by the rule of ``SP_GATE``: 10 times
the difference measured on MI355X, at least 8e-15, at most 1e-10."""
import os

import numpy as np

from evcont_amd.gto_spdf import Shell
from spgto_cases import CEILING, DEVICE_HOST_GATE, NAMES, scaled_diff, unpack_eri, unpack_ip1     # noqa: F401

# worst array of spdgto_cases.two_centre through evc_spdfgto_* against evc_spdgto_*, full and packed forms, on MI355X
# (tests/test_gpu_spdfgto.py::test_spd_molecule_against_the_spd_kernels prints it)
SPD_MEASURED = 3.9e-16
SPD_GATE = min(CEILING, max(10 * SPD_MEASURED, 8e-15))


def small_f():
    """A centre with s and a one-primitive f shell, a second with p: N = 11, what the CPU tests rebuild.
    -> (R (2,3), Z, shells)"""
    R = np.array([[0.0, 0.0, 0.0], [0.3, 1.1, -0.7]])
    return R, np.array([3.0, 2.0]), [[Shell(0, [1.3], [1.0]), Shell(3, [0.9], [1.0])], [Shell(1, [0.7], [1.0])]]


def two_centre():
    """s + f on one centre, p + d + f on the other, one-primitive shells: N = 23, Ms = 276, the kets span five blocks of
    64 and every class of bra and ket pair (highest l 0 ... 3) is present.  -> (R (2,3), Z, shells)"""
    R = np.array([[0.0, 0.0, 0.0], [0.9, -0.6, 1.3]])
    shells = [[Shell(0, [1.1], [1.0]), Shell(3, [0.8], [1.0])],
              [Shell(1, [0.9], [1.0]), Shell(2, [0.7], [1.0]), Shell(3, [1.2], [1.0])]]
    return R, np.array([3.0, 2.0]), shells


def atom():
    """One centre with s, p, d and f (the f shell of two primitives): N = 16, every P - A = 0, the coincident-centre
    path.  -> (R (1,3), Z, shells)"""
    shells = [[Shell(0, [1.1], [1.0]), Shell(1, [0.9], [1.0]), Shell(2, [0.8], [1.0]), Shell(3, [1.4, 0.5], [0.6, 0.5])]]
    return np.array([[0.2, -0.1, 0.4]]), np.array([4.0]), shells


def eight_primitive_f():
    """A contracted f shell of eight primitives beside an s function: N = 8.  -> (R, Z, shells)"""
    ex8 = np.geomspace(0.2, 25.0, 8)
    shells = [[Shell(3, ex8, [0.1, 0.2, 0.3, 0.4, 0.4, 0.3, 0.2, 0.1])], [Shell(0, [0.8], [1.0])]]
    return np.array([[0.0, 0.0, 0.0], [0.7, -0.9, 1.2]]), np.array([2.0, 1.0]), shells


def limit_molecule(reverse=False):
    """Three centres of s + p + d + f (16 functions each) and four of s + p (4 each): N = 64, Ms = 2080, 20 shells, 128
    primitives (s and p shells of eight, d shells of four -- that of centre 1 of two --, f shells of two): no padding in
    any of the kernels' tables, primitive offsets up to 120.  ``reverse``: every atom lists its shells in the opposite
    order -- the same functions in another AO order, with other primitive offsets and another sorted order of the kets.
    -> (R, Z, shells)"""
    ex8 = np.geomspace(0.15, 40.0, 8)
    co8 = np.array([0.3, 0.4, 0.5, 0.4, 0.3, 0.2, 0.1, 0.05])
    shells = []
    for c in range(7):
        atom = [Shell(0, ex8 * (1 + 0.05 * c), co8), Shell(1, ex8[::-1] * (0.5 + 0.03 * c), co8)]
        if c < 3:
            d = [0.9, 0.35] if c == 1 else [2.1, 0.9, 0.4, 0.17]
            atom += [Shell(2, d, [0.6, 0.5, 0.3, 0.2][:len(d)]), Shell(3, [1.3 + 0.2 * c, 0.45], [0.6, 0.5])]
        shells.append(atom[::-1] if reverse else atom)
    grid = np.array([[i, j, k] for i in range(2) for j in range(2) for k in range(2)], dtype=float)[:7]
    R = 2.2 * grid + 0.3 * np.random.default_rng(5).standard_normal((7, 3))
    return R, np.array([3.0, 1.0, 2.0, 1.0, 4.0, 1.0, 2.0]), shells


def water_sto3g_f():
    """Water in STO-3G with one f shell on O: N = 14.  -> (R, Z, shells)"""
    from evcont_amd import gto_small
    m = gto_small.BASES["sto-3g"]
    sp = lambda sym: [Shell(l, ex, c) for ex, cs, cp in m[sym] for l, c in ((0, cs), (1, cp)) if c is not None]
    shells = [sp("O") + [Shell(3, [1.1], [1.0])], sp("H"), sp("H")]
    return gto_small.water_coords(), np.array([8.0, 1.0, 1.0]), shells


def _even_tempered(first, ratio, count):
    return tuple(first * ratio ** k for k in range(count))


def tz_shape_water():
    """Water in an EVEN-TEMPERED basis of the cc-pVTZ SHAPE: O [4s3p2d1f] with the two inner s contractions of eight
    primitives each, H [3s2p1d]; N = 58, 42 primitives, exponent ratios of about 3 so that S stays well conditioned.  It
    has the shape and NOT the numbers of Dunning's basis: the exponents are geometric series and the contraction
    coefficients smooth made-up weights, so energies in it mean nothing chemically.  -> (table, R (3,3), Z, shells)"""
    o_s = _even_tempered(0.35, 3.0, 8)[::-1]
    table = {
        "O": [(0, o_s, (0.001, 0.008, 0.04, 0.13, 0.3, 0.42, 0.25, 0.02)),
              (0, o_s, (-0.0003, -0.002, -0.009, -0.03, -0.08, -0.17, -0.1, 0.6)),
              (0, (1.0,), (1.0,)), (0, (0.3,), (1.0,)),
              (1, _even_tempered(1.2, 3.2, 3)[::-1], (0.05, 0.25, 0.5)), (1, (0.7,), (1.0,)), (1, (0.22,), (1.0,)),
              (2, (2.3,), (1.0,)), (2, (0.65,), (1.0,)),
              (3, (1.4,), (1.0,))],
        "H": [(0, _even_tempered(0.9, 3.1, 3)[::-1], (0.03, 0.2, 0.55)), (0, (0.33,), (1.0,)), (0, (0.1,), (1.0,)),
              (1, (1.4,), (1.0,)), (1, (0.39,), (1.0,)),
              (2, (1.05,), (1.0,))],
    }
    from evcont_amd import gto_spdf
    Z, shells = gto_spdf.water_shells(table)
    return table, gto_spdf.water_coords(), np.array(Z), shells


HOST_REFS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spdfgto_host_refs.npz")
HOST_REF_CASES = {"two_centre": two_centre, "atom": atom}
REF_ORIGIN = (0.3, 0.1, -0.2)
WATER_REFS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spdfgto_water_refs.npz")


def water_ref_coords():
    """The shaken water geometry of the recorded host arrays of ``water_sto3g_f`` (``WATER_REFS``)."""
    from evcont_amd.gto_small import water_coords
    return water_coords(1.8088, 104.5) + 0.05 * np.random.default_rng(1).standard_normal((3, 3))


def load_water_ref():
    """The recorded host statement of ``water_sto3g_f`` at ``water_ref_coords`` as a host molecule (full forms)."""
    from evcont_amd.gto_spdf import SpdfGaussianMol
    _, Z, shells = water_sto3g_f()
    with np.load(WATER_REFS) as z:
        a = {k: z[k] for k in z.files}
    n = a["S"].shape[0]
    slices = np.array([[0, 12], [12, 13], [13, 14]], dtype=np.int64)
    return SpdfGaussianMol(S=a["S"], hcore=a["hcore"], eri=unpack_eri(a["eri"], n), ipovlp=a["ipovlp"], dhcore=a["dhcore"],
                           eri_ip1=unpack_ip1(a["eri_ip1"], n), aoslices=slices, enuc=float(a["enuc"]), gnuc=a["gnuc"],
                           integral_symmetry=True, coords=water_ref_coords(), nelec=(5, 5), charges=Z, shells=shells,
                           renormalize=True)


def boys_grid():
    """``spdgto_cases.boys_grid`` and t = 13 ... 30: 78 values, the crossover at 12 included from both sides."""
    import spdgto_cases
    return np.concatenate([spdgto_cases.boys_grid(), [13.0, 14.0, 16.0, 20.0, 25.0, 30.0]])


# worst relative error of ``gto_host.boys(13, t)`` over ``boys_grid`` per order against mpmath at 50 digits, as measured on
# a CPU: F0 ... F13 (``python tests/spdfgto_cases.py`` prints them)
BOYS_MEASURED = (3.7e-16, 4.4e-16, 4.5e-16, 4.9e-16, 4.9e-16, 5.6e-16, 5.9e-16, 6.4e-16, 7.4e-16, 7.6e-16,
                 9.0e-16, 1.2e-15, 1.4e-15, 1.8e-15)


def boys_grid_errors(nmax=13):
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


def load_host_refs():
    with np.load(HOST_REFS) as z:
        return {k: z[k] for k in z.files}


def ref_diffs(arrays, refs, name, names=NAMES):
    """name -> ``scaled_diff`` of full-form arrays against the recorded host arrays of case ``name``; eri and eri_ip1
    over the recorded sample ``eri_idx``."""
    i = refs[f"{name}/eri_idx"].astype(np.int64)
    out = {}
    for k in names:
        x = np.asarray(arrays[k], dtype=np.float64)
        if k == "eri":
            x = x[i[:, 0], i[:, 1], i[:, 2], i[:, 3]]
        if k == "eri_ip1":
            x = x[:, i[:, 0], i[:, 1], i[:, 2], i[:, 3]]
        out[k] = scaled_diff(x, refs[f"{name}/{k}"])
    return out


# ---- the truth file ----------------------------------------------------------------------------------------------------
# tests/golden/spdfgto_truth.npz (make_spdfgto_truth.py: closed s forms differentiated with respect to the centres in
# mpmath up to total order 13, no Hermite expansion).  One-electron arrays, enuc, gnuc, the dipole integrals and their
# gradient in full; eri and eri_ip1 as a sample (``eri_idx``: one element per class of shell types with an f shell).
TRUTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spdfgto_truth.npz")
TRUTH_CASES = ("a", "b_flat", "c", "d_lo", "d_hi")
TRUTH_FIELDS = ("enuc", "S", "hcore", "eri", "ipovlp", "dhcore", "eri_ip1", "gnuc", "dip", "ipdip")
TRUTH_FLOOR = 8e-16          # spgto_cases.DEVICE_RECORDED: the gate is at least ten times this
# max |host statement - truth| / max(1, max |truth|), in the order of TRUTH_FIELDS (printed by ``python tests/spdfgto_cases.py``)
HOST_MEASURED = {
    #     enuc        S    hcore      eri   ipovlp   dhcore  eri_ip1     gnuc      dip    ipdip
    "a": (1.4e-16, 8.9e-16, 2.1e-16, 8.8e-17, 5.8e-16, 7.8e-16, 1.1e-16, 1.6e-16, 7.0e-16, 7.4e-16),
    "b_flat": (1.1e-16, 4.4e-16, 7.1e-16, 3.1e-17, 3.9e-16, 1.8e-15, 6.4e-16, 2.4e-16, 4.2e-16, 4.9e-16),
    "c": (6.3e-17, 8.9e-16, 7.9e-16, 1.4e-18, 8.2e-15, 1.7e-14, 4.4e-14, 1.1e-16, 1.1e-15, 5.9e-15),
    "d_lo": (1.0e-16, 3.3e-16, 6.1e-16, 2.0e-17, 7.3e-16, 1.7e-15, 2.5e-16, 1.7e-16, 4.1e-16, 5.9e-16),
    "d_hi": (1.0e-16, 3.3e-16, 6.2e-16, 2.4e-17, 7.3e-16, 1.7e-15, 2.5e-16, 2.0e-16, 4.1e-16, 5.9e-16),
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
    from evcont_amd.gto_spdf import spdf_gaussian_mol
    return spdf_gaussian_mol(T[f"{name}/R"], T[f"{name}/Z"], truth_shells(T, name), renormalize=False)


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
    out["ipdip"] = truth_err(m.dipole_grad_integrals(T[f"{name}/origin"]), T, name, "ipdip")
    return out


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("BOYS_MEASURED = (" + ", ".join(f"{e:.1e}" for e in boys_grid_errors()) + ")")
    T = load_truth()
    print("# " + " ".join(f"{f:>8s}" for f in TRUTH_FIELDS))
    for case in TRUTH_CASES:
        e = host_truth_errors(T, case)
        print(f'    "{case}": (' + ", ".join(f"{e[f]:.1e}" for f in TRUTH_FIELDS) + "),")
