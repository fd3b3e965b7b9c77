"""Shared by the tests of ``evcont_amd.gto_small`` / ``csrc/spgto.hip``: the cases of tests/golden/spgto_truth.npz
(tests/golden/make_spgto_truth.py: sympy and mpmath, no McMurchie-Davidson) as molecules, the error measure and the gates.

Measure: max |x - truth| / max(1, max |truth|) per array.  Measured on the CPU for the host statement over all cases and
arrays: 2.1e-12 (dhcore of the tight + diffuse case "c": one function has exponent 5000 and one-electron derivative terms
of 1e5 cancel there; every other array of every case is below 1e-15).  The gate is 10 times that, below the hard ceiling
of 1e-10 (the project's energy parity).  The device is held to the same gate against the truth and, against the host
statement, to 100 times the host's error (the summation orders differ), capped by the same ceiling."""
import os

import numpy as np

NAMES = ("enuc", "S", "hcore", "eri", "ipovlp", "dhcore", "eri_ip1", "gnuc")
CASES = ("a", "b", "b_flat", "c", "d")
HOST_MEASURED = 2.1e-12
CEILING = 1e-10
TRUTH_GATE = min(10 * HOST_MEASURED, CEILING)
DEVICE_HOST_GATE = min(100 * HOST_MEASURED, CEILING)
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spgto_truth.npz")


def load_truth():
    with np.load(PATH) as z:
        return {k: z[k] for k in z.files}


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
