"""Writes the input files of tools/micro/spdfgto_cpu_check.hip: per molecule the flattened basis, the geometry and the
arrays of the host statement ``gto_spdf.spdf_gaussian_mol`` (full forms), as raw int32 / float64 in the order the program
reads them.  Two small molecules that between them have every l and every class of pair:

    small_f   s + f on one centre, p on another (tests/spdfgto_cases.small_f): N = 11
    df_atom   d + f on one centre and a bare second nucleus: N = 12, every P - A = 0

usage: python tools/micro/spdfgto_cpu_check.py PREFIX     (writes PREFIX.small_f.bin and PREFIX.df_atom.bin)"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

ORIGIN = (0.3, 0.1, -0.2)


def df_atom():
    from evcont_amd.gto_spdf import Shell
    R = np.array([[0.2, -0.1, 0.4], [1.0, 0.8, -0.5]])
    return R, np.array([3.0, 1.0]), [[Shell(2, [0.8], [1.0]), Shell(3, [1.4, 0.5], [0.6, 0.5])], []]


def write(path, R, Z, shells):
    from evcont_amd.gto_host import contraction_coefficients, flatten_shells
    from evcont_amd.gto_spdf import spdf_gaussian_mol
    m = spdf_gaussian_mol(R, Z, shells)
    sa, sl, so, ex, co, _, n = flatten_shells(shells, contraction_coefficients(shells, True))
    with open(path, "wb") as f:
        np.array([len(Z), len(sl), len(ex), n], dtype=np.int32).tofile(f)
        for a in (sa, sl, so):
            np.ascontiguousarray(a, dtype=np.int32).tofile(f)
        for a in (ex, co, R, Z, ORIGIN, m.S, m.hcore, m.ipovlp, m.dhcore, m.eri, m.eri_ip1, m.dipole_integrals(ORIGIN),
                  m.dipole_grad_integrals(ORIGIN)):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    print(f"wrote {path}: N = {n}")


def main():
    import spdfgto_cases as fc
    prefix = sys.argv[1]
    write(prefix + ".small_f.bin", *fc.small_f())
    write(prefix + ".df_atom.bin", *df_atom())


if __name__ == "__main__":
    main()
