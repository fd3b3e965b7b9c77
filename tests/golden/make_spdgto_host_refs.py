"""Generates tests/golden/spdgto_host_refs.npz: arrays of the HOST statement ``gto_spd.spd_gaussian_mol`` on molecules where
it takes from half a minute to minutes, so that the GPU tests can hold the device to it without running it
(tests/test_gpu_spdgto_limits.py): the two pairs ``spdgto_cases.LIMIT_PAIRS`` of the N = 64 limit shape (the other
nuclei bare; S, hcore, eri, enuc, without derivatives) and the molecule with a d shell of eight primitives (all eight
arrays and the dipole integrals).  Recorded results of a numpy program, no device involved.

    python tests/golden/make_spdgto_host_refs.py
"""
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

ORIGIN = (0.3, 0.1, -0.2)


def job(name):
    import spdgto_cases as dc
    from evcont_amd.gto_spd import spd_gaussian_mol
    if name == "d8":
        m = spd_gaussian_mol(*dc.eight_primitive_d())
        out = {k: np.asarray(getattr(m, k)) for k in dc.NAMES}
        out["dip"] = m.dipole_integrals(ORIGIN)
    else:
        atoms = tuple(int(c) for c in name[4:].split("_"))
        m = spd_gaussian_mol(*dc.limit_pair(atoms), need_grad=False)
        out = {k: np.asarray(getattr(m, k)) for k in ("enuc", "S", "hcore", "eri")}
    return {f"{name}/{k}": v for k, v in out.items()}


def main():
    import spdgto_cases as dc
    names = ["d8"] + ["pair" + "_".join(str(a) for a in atoms) for atoms in dc.LIMIT_PAIRS]
    with Pool(len(names)) as pool:
        parts = pool.map(job, names)
    made = {k: v for part in parts for k, v in part.items()}
    made["origin"] = np.asarray(ORIGIN)
    np.savez_compressed(dc.HOST_REFS, **made)
    print(f"wrote {dc.HOST_REFS}: {os.path.getsize(dc.HOST_REFS)} bytes")


if __name__ == "__main__":
    main()
