#!/usr/bin/env python3
"""MD of a water molecule on the continuation surface of FCI training states, with nothing third-party -- the
reference's ``scripts/MD/H2O/md_H2O_6_31G_FCI.py`` without PySCF: the AO integrals come from ``evcont_amd.gto_small``
(numpy) for the training states and, per MD step, either from the same host statement or from the device
(``evcont_amd.gto_device``, csrc/spgto.hip: coordinates in, forces out).

    FCI_EVCont_obj(cisolver=SmallFCI() | DeviceFCI())  <-  training states along the symmetric stretch
    state_swarm([mol], one_rdm, two_rdm, overlap, root=0, integrals="host" | "device")

    python examples/h2o_fci_md.py [--basis sto-3g|6-31g] [--integrals host|device] [--solver small|device]
                                  [--states 4] [--steps 20] [--dt 5]

STO-3G (7 orbitals, 441 determinants) takes seconds; 6-31G (13 orbitals, 1.7 million determinants) needs
``--solver device`` and minutes.  Both ``--integrals`` routes print the same energies.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evcont_amd.FCI_EVCont import FCI_EVCont_obj            # noqa: E402
from evcont_amd.MD_utils import state_swarm                 # noqa: E402
from evcont_amd.gto_small import ANGSTROM, water            # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--basis", default="sto-3g", choices=["sto-3g", "6-31g"])
p.add_argument("--integrals", default="device", choices=["host", "device"])
p.add_argument("--solver", default="small", choices=["small", "device"])
p.add_argument("--states", type=int, default=4)
p.add_argument("--steps", type=int, default=20)
p.add_argument("--dt", type=float, default=5.0)
a = p.parse_args()

if a.solver == "device":
    from evcont_amd.fci_device import DeviceFCI
    solver = DeviceFCI()
else:
    from evcont_amd.fci_small import SmallFCI
    solver = SmallFCI()

t0 = time.time()
cont = FCI_EVCont_obj(cisolver=solver, cibasis="OAO")
for r in np.linspace(0.85, 1.35, a.states) * ANGSTROM:      # symmetric stretch around the equilibrium bond length
    cont.append_to_rdms(water(a.basis, r_oh=r, need_grad=False))
print(f"{a.states} FCI training states of water / {a.basis} (N = {cont.one_rdm.shape[-1]}): {time.time() - t0:.1f} s")

init = water(a.basis, r_oh=1.15 * 0.9572 * ANGSTROM)          # a stretched start: the molecule vibrates
t0 = time.time()
frames = state_swarm([init], cont.one_rdm, cont.two_rdm, cont.overlap, root=0, dt=a.dt, steps=a.steps,
                     integrals=a.integrals)
wall = time.time() - t0
for f in frames[:: max(1, a.steps // 10)]:
    r1 = np.linalg.norm(f["coord"][0, 1] - f["coord"][0, 0]) / ANGSTROM
    print(f"t = {f['time']:7.1f}  r(OH) = {r1:.4f} A  E_pot = {f['epot'][0]:.10f}  E_tot = {f['epot'][0] + f['ekin'][0]:.10f}")
etot = np.array([f["epot"][0] + f["ekin"][0] for f in frames])
print(f"{a.steps} NVE steps with integrals on the {a.integrals}: {wall:.2f} s wall, drift of the total energy "
      f"{np.abs(etot - etot[0]).max():.2e} Ha")
assert np.all(np.isfinite(etot))
print("OK")
