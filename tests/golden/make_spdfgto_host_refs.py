"""Generates tests/golden/spdfgto_host_refs.npz: arrays of the HOST statement ``gto_spdf.spdf_gaussian_mol`` on the
molecules ``spdfgto_cases.HOST_REF_CASES`` (N = 23 and N = 16), where it takes from half a minute to minutes, so that the
GPU tests can hold the device to it without running it (tests/test_gpu_spdfgto.py).  Per case: enuc, S, hcore, ipovlp,
dhcore, gnuc, the dipole integrals and their gradient at ``spdfgto_cases.REF_ORIGIN`` in full; eri and eri_ip1 at a
recorded random sample of index quadruples ``eri_idx`` (the full arrays of N = 23 would be 9 MB), drawn so that every
class of shell types of the molecule is in it.  And tests/golden/spdfgto_water_refs.npz: all arrays of water / STO-3G
with an f shell on O (N = 14, ``spdfgto_cases.water_sto3g_f`` at ``spdfgto_cases.water_ref_coords()``), eri in the s4
and eri_ip1 in the s2kl form, for the end-to-end test of energies and forces (tests/test_gpu_spdfgto_md.py).  Recorded
results of a numpy program, no device involved.

    python tests/golden/make_spdfgto_host_refs.py
"""
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SAMPLE = {"two_centre": 9000, "atom": 4000}


def job(name):
    import spdfgto_cases as fc
    from evcont_amd.gto_spdf import spdf_gaussian_mol
    m = spdf_gaussian_mol(*fc.HOST_REF_CASES[name]())
    n = m.S.shape[0]
    out = {k: np.asarray(getattr(m, k)) for k in fc.NAMES if k not in ("eri", "eri_ip1")}
    out["dip"] = m.dipole_integrals(fc.REF_ORIGIN)
    out["ipdip"] = m.dipole_grad_integrals(fc.REF_ORIGIN)
    # the l of every function, then one quadruple of every class of l and a random rest
    ls = np.concatenate([np.full(2 * sh.l + 1, sh.l) for atom_shells in m.shells for sh in atom_shells])
    rng = np.random.default_rng(17)
    first = {}
    for q in rng.integers(0, n, size=(200000, 4)):
        first.setdefault(tuple(ls[q]), q)
    assert len(first) == len(set(ls)) ** 4, "the sample must hold every class of shell types"
    idx = np.concatenate([np.array(list(first.values())), rng.integers(0, n, size=(SAMPLE[name], 4))]).astype(np.int16)
    i = idx.astype(np.int64)
    out["eri_idx"] = idx
    out["eri"] = m.eri[i[:, 0], i[:, 1], i[:, 2], i[:, 3]]
    out["eri_ip1"] = m.eri_ip1[:, i[:, 0], i[:, 1], i[:, 2], i[:, 3]]
    return {f"{name}/{k}": v for k, v in out.items()}


def water(_):
    import spdfgto_cases as fc
    from evcont_amd.gto_spdf import spdf_gaussian_mol
    _, Z, shells = fc.water_sto3g_f()
    m = spdf_gaussian_mol(fc.water_ref_coords(), Z, shells)
    out = {k: np.asarray(getattr(m, k)) for k in fc.NAMES}
    iu, ju = np.tril_indices(m.S.shape[0])
    out["eri"] = m.eri[iu, ju][:, iu, ju]
    out["eri_ip1"] = m.eri_ip1[..., iu, ju]
    np.savez_compressed(fc.WATER_REFS, **out)
    print(f"wrote {fc.WATER_REFS}: {os.path.getsize(fc.WATER_REFS)} bytes")
    return {}


def main():
    import spdfgto_cases as fc
    names = sorted(fc.HOST_REF_CASES)
    with Pool(len(names) + 1) as pool:
        extra = pool.map_async(water, [0])
        parts = pool.map(job, names)
        extra.get()
    made = {k: v for part in parts for k, v in part.items()}
    np.savez_compressed(fc.HOST_REFS, **made)
    print(f"wrote {fc.HOST_REFS}: {os.path.getsize(fc.HOST_REFS)} bytes")


if __name__ == "__main__":
    main()
