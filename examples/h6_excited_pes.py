#!/usr/bin/env python3
"""Lowest singlet surfaces of a 6-atom hydrogen chain from excited-state continuations: three training sets, holding root
0, root 1, and roots 0 and 1 of the FCI at three spacings each, and the two lowest surfaces each of them predicts
(``approximate_multistate_OAO``), against the exact singlets.

Without a spin penalty the FCI solvers here are spin-adapted through Ms only, so "root 1" of ``nelec = (3, 3)`` is a
triplet; ``--spin-penalty 0.2`` (the default) makes the solver see ``H + 0.2 S^2`` and the trained states singlets, as a
solver with singlet symmetry would give them.  ``--spin-penalty 0`` shows the mix.  <S^2> of every trained state is printed.

    python examples/h6_excited_pes.py                              # needs a HIP device for the continuation itself
    python examples/h6_excited_pes.py --solver device-davidson     # the FCI and its eigensolver on the GPU as well
    python examples/h6_excited_pes.py --oscillator                 # f_0k of the predicted states along the scan
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evcont_amd.FCI_EVCont import FCI_EVCont_obj                                       # noqa: E402
from evcont_amd.ab_initio_eigenvector_continuation import approximate_multistate_OAO, \
    get_multistate_properties                                                          # noqa: E402
from evcont_amd.properties import oscillator_strength                                  # noqa: E402
from evcont_amd.electron_integral_utils import get_basis, get_integrals               # noqa: E402
from evcont_amd.fci_small import SmallFCI                                              # noqa: E402
from evcont_amd.hchain import hydrogen_chain                                           # noqa: E402

N_ATOMS, NELEC = 6, (3, 3)
TRAIN_DISTS = (1.0, 1.8, 2.6)
PROTOCOLS = ([0], [1], [0, 1])


def make_solver(kind, penalty):
    if kind == "host":
        return SmallFCI(spin_penalty=penalty)
    from evcont_amd.fci_device import DeviceFCI
    return DeviceFCI(eigensolver="davidson" if kind == "device-davidson" else "host", spin_penalty=penalty)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--solver", choices=("host", "device", "device-davidson"), default="host")
    p.add_argument("--spin-penalty", type=float, default=0.2,
                   help="shift of H + shift (S^2 - S(S+1)) in the FCI of the training states; 0: no penalty, and the "
                        "excited training states are triplets")
    p.add_argument("--points", type=int, default=25, help="geometries of the scan between 0.9 and 2.8 Bohr")
    p.add_argument("--oscillator", action="store_true",
                   help="also the oscillator strengths f_0k = 2/3 (E_k - E_0) |mu_0k|^2 of the predicted states along the "
                        "scan (get_multistate_properties), written to oscillator_strengths_roots_*.txt")
    a = p.parse_args()
    solver = make_solver(a.solver, a.spin_penalty)
    test_dists = np.linspace(0.9, 2.8, a.points)
    test_mols = [hydrogen_chain(N_ATOMS, float(d), need_grad=False) for d in test_dists]
    # the exact two lowest states of the multiplicity the solver is held to
    exact = []
    for mol in test_mols:
        h1, h2 = get_integrals(mol, get_basis(mol))
        exact.append(np.array(solver.kernel(h1, h2, N_ATOMS, NELEC, nroots=2)[0]) + mol.energy_nuc())
    exact = np.array(exact)
    np.savetxt("exact_surfaces.txt", np.column_stack([test_dists, exact]))
    for roots in PROTOCOLS:
        cont = FCI_EVCont_obj(cisolver=solver, cibasis="OAO", nroots=max(roots) + 1, roots_train=list(roots))
        for d in TRAIN_DISTS:
            before = len(cont.fcivecs)
            cont.append_to_rdms(hydrogen_chain(N_ATOMS, d, need_grad=False))
            for k, vec in zip(roots, cont.fcivecs[before:]):
                ss = solver.spin_square(vec, N_ATOMS, NELEC)[0]
                print(f"roots_train={roots} d={d:.1f} root {k}: E = {cont.ens[before + roots.index(k)]:.8f} "
                      f"<S^2> = {round(ss, 6) + 0.0:.6f}")
        nstates = min(2, cont.ntrain)
        pred = np.array([approximate_multistate_OAO(m, cont.one_rdm, cont.two_rdm, cont.overlap, nroots=nstates)[0]
                         for m in test_mols])
        tag = "".join(str(r) for r in roots)
        np.savetxt(f"predicted_surfaces_roots_{tag}.txt", np.column_stack([test_dists, pred]))
        err = np.abs(pred - exact[:, :nstates]).max(axis=0)
        print(f"roots_train={roots}: {cont.ntrain} states, max |error| of the {nstates} lowest surfaces: "
              + ", ".join(f"{x:.2e}" for x in err) + " Ha")
        if a.oscillator and nstates > 1:
            # f_0k along the scan: the transition dipoles of every geometry in one batched device call
            pairs = [(0, k) for k in range(1, nstates)]
            E, props = get_multistate_properties(test_mols, cont.one_rdm, cont.two_rdm, cont.overlap, nstates, pairs)
            f = np.stack([oscillator_strength(E[:, 0], E[:, k], props["dipole"][:, p]) for p, (_, k) in enumerate(pairs)],
                         axis=1)
            np.savetxt(f"oscillator_strengths_roots_{tag}.txt", np.column_stack([test_dists, f]))
            print(f"roots_train={roots}: f_0k along the scan between {f.min():.3e} and {f.max():.3e}")


if __name__ == "__main__":
    main()
