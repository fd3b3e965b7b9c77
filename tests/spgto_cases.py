"""Shared by the tests of ``evcont_amd.gto_small`` / ``csrc/spgto.hip``: the cases of tests/golden/spgto_truth.npz and
tests/golden/spgto_truth_crossover.npz (tests/golden/make_spgto_truth.py: sympy and mpmath, no McMurchie-Davidson) as
molecules, the error measure and the gates.

Measure: max |x - truth| / max(1, max |truth|) per array.  HOST_MEASURED holds it for the host statement, per case and
array, on a CPU; the table is printed by

    python tests/spgto_cases.py

One entry stands out: 2.1e-12, dhcore of the tight + diffuse case "c" (one function has exponent 5000 and one-electron
derivative terms of 1e5 cancel there); every other array of every case is below 1e-15.  The gate against the truth is per
(case, array), for the host statement and the device alike (``truth_gate``): 10 times the host's value, but no less than
10 times DEVICE_RECORDED (8e-16, the worst the device has shown outside dhcore of "c") and no
more than the hard ceiling of 1e-10 (the project's energy parity).  DEVICE_MEASURED is for entries where the device's
honest rounding exceeds that: such an entry is the value measured on MI355X times 10 and says so.  Against the host
statement the device is held to 100 times the host's worst error (the summation orders differ), capped by the ceiling."""
import os

import numpy as np

NAMES = ("enuc", "S", "hcore", "eri", "ipovlp", "dhcore", "eri_ip1", "gnuc")
FIELDS = NAMES + ("dip",)
CASES = ("a", "b", "b_flat", "c", "d", "e_lo", "e_hi")
HOST_WORST = 2.1e-12
CEILING = 1e-10
DEVICE_RECORDED = 8e-16
# max |host statement - truth| / max(1, max |truth|), in the order of FIELDS
HOST_MEASURED = {
    #     enuc        S    hcore      eri   ipovlp   dhcore  eri_ip1     gnuc      dip
    "a": (1.4e-16, 1.3e-16, 1.6e-16, 1.7e-16, 2.5e-16, 2.9e-16, 1.5e-16, 1.6e-16, 1.3e-16),
    "b": (2.8e-17, 4.4e-16, 3.7e-16, 4.1e-16, 4.4e-16, 9.0e-16, 3.4e-16, 2.7e-16, 2.3e-16),
    "b_flat": (1.1e-16, 4.4e-16, 2.8e-16, 4.1e-16, 4.4e-16, 7.5e-16, 3.4e-16, 2.4e-16, 2.1e-16),
    "c": (6.3e-17, 6.7e-16, 5.3e-16, 7.2e-16, 6.4e-16, 2.1e-12, 7.7e-16, 1.1e-16, 2.5e-16),
    "d": (1.8e-17, 4.4e-16, 5.2e-16, 2.8e-16, 2.8e-16, 1.1e-16, 3.6e-16, 3.1e-18, 3.3e-16),
    "e_lo": (1.0e-16, 4.4e-16, 2.8e-16, 4.1e-16, 4.4e-16, 7.8e-16, 3.4e-16, 1.7e-16, 4.1e-16),
    "e_hi": (1.0e-16, 4.4e-16, 2.3e-16, 4.1e-16, 4.4e-16, 8.7e-16, 3.4e-16, 2.0e-16, 4.1e-16),
}
# (case, array) -> the device's value measured on MI355X, where it is above the floor and is rounding, not a defect
DEVICE_MEASURED = {}
# the largest entry of the table (dhcore of "c"); what is not a comparison with the truth of one case and array uses it
TRUTH_GATE = min(10 * HOST_WORST, CEILING)
DEVICE_HOST_GATE = min(100 * HOST_WORST, CEILING)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATHS = (os.path.join(GOLDEN, "spgto_truth.npz"), os.path.join(GOLDEN, "spgto_truth_crossover.npz"))


def truth_gate(case, field):
    """The gate of one array of one case against the truth file."""
    gate = max(10 * HOST_MEASURED[case][FIELDS.index(field)], 10 * DEVICE_RECORDED)
    if (case, field) in DEVICE_MEASURED:
        gate = max(gate, 10 * DEVICE_MEASURED[case, field])
    return min(CEILING, gate)


def load_truth():
    out = {}
    for path in PATHS:
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def case_shells(T, name):
    from evcont_amd.gto_small import Shell
    sa, sl, so, ex, co = (T[f"{name}/{k}"] for k in ("shell_atom", "shell_l", "shell_off", "ex", "co"))
    shells = [[] for _ in range(len(T[f"{name}/Z"]))]
    for s in range(len(sa)):
        shells[sa[s]].append(Shell(int(sl[s]), ex[so[s]:so[s + 1]], co[so[s]:so[s + 1]]))
    return shells


def case_mol(T, name, need_grad=True):
    """The case as a ``GaussianMol`` with the tabulated coefficients as they stand, as the truth file uses them."""
    from evcont_amd.gto_small import sp_gaussian_mol
    return sp_gaussian_mol(T[f"{name}/R"], T[f"{name}/Z"], case_shells(T, name), need_grad, renormalize=False)


def rel_err(x, T, name, field):
    """max |x - truth| / max(1, max |truth|), the truth as the double-double hi + lo."""
    hi, lo = T[f"{name}/{field}_hi"], T[f"{name}/{field}_lo"].astype(np.float64)
    return float(np.abs((np.asarray(x, dtype=np.float64) - hi) - lo).max() / max(1.0, np.abs(hi).max()))


def host_errors(T, name):
    """{array: rel_err of the host statement} of one case, the dipole integrals included."""
    m = case_mol(T, name)
    out = {f: rel_err(getattr(m, f), T, name, f) for f in NAMES}
    out["dip"] = rel_err(m.dipole_integrals(T[f"{name}/origin"]), T, name, "dip")
    return out


def scaled_diff(x, y):
    return float(np.abs(np.asarray(x) - np.asarray(y)).max() / max(1.0, np.abs(np.asarray(y)).max()))


def unpack_eri(e, n):
    """(Ms,Ms) s4 -> (n,n,n,n)."""
    iu, ju = np.tril_indices(n)
    half = np.zeros((n, n, e.shape[1]))
    half[iu, ju] = e
    half[ju, iu] = e
    full = np.zeros((n, n, n, n))
    full[:, :, iu, ju] = half
    full[:, :, ju, iu] = half
    return full


def unpack_ip1(p, n):
    """(3,n,n,Ms) s2kl -> (3,n,n,n,n)."""
    iu, ju = np.tril_indices(n)
    full = np.zeros((3, n, n, n, n))
    full[..., iu, ju] = p
    full[..., ju, iu] = p
    return full


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(GOLDEN)))
    T = load_truth()
    print("# " + " ".join(f"{f:>8s}" for f in FIELDS))
    for case in CASES:
        e = host_errors(T, case)
        print(f'    "{case}": (' + ", ".join(f"{e[f]:.1e}" for f in FIELDS) + "),")
