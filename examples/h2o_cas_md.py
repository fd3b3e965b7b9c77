#!/usr/bin/env python3
"""MD of a water molecule in cc-pVDZ on the continuation surface of CASCI training states, with nothing third-party --
the reference's ``scripts/MD/H2O/md_H2O_vdz_CAS_continuation.py`` without PySCF.  Every AO integral comes from the device
(``evcont_amd.gto_spd_device``, csrc/spdgto.hip: s, p and real spherical d shells): the training geometries through
``DeviceSpdGaussians.to_mol`` (RHF + CASCI on downloaded arrays), the MD steps from the coordinates.

    CAS_EVCont_obj(ncas, neleca, cisolver=DeviceFCI() | SmallFCI())  <-  training states along the symmetric stretch
    state_swarm([mol], one_rdm, two_rdm, overlap, root=0, integrals="device")

    python examples/h2o_cas_md.py [--small] [--states 4] [--steps 20] [--dt 5] [--nroots R --root k [--spin-penalty 0.2]]
                                  [--resident]

Default: CAS(8,8) with the device FCI solver; ``--small``: CAS(4,4) with the numpy solver (seconds).
``--nroots R``: R CASCI roots per training geometry (``CAS_EVCont_obj(..., nroots=R)``, one block call per geometry,
DESIGN.md 8.1.6) and the dynamics on surface ``--root k``; the first frame prints the vertical excitation energies and
the oscillator strengths from the ground state.  ``--spin-penalty`` keeps the roots to the ground state's multiplicity.
``--resident``: the training set grows on the device (``resident.ResidentCAS_EVCont_obj``; device FCI
solver, CAS(8,8) or with ``--small`` CAS(4,4)) and the calls below read ``cont.device_trdms()``.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evcont_amd.CASCI_EVCont import CAS_EVCont_obj                    # noqa: E402
from evcont_amd.MD_utils import state_swarm                          # noqa: E402
from evcont_amd.ab_initio_eigenvector_continuation import get_multistate_properties   # noqa: E402
from evcont_amd.gto_spd import ANGSTROM, water_coords, water_shells  # noqa: E402
from evcont_amd.gto_spd_device import DeviceSpdGaussians             # noqa: E402
from evcont_amd.properties import oscillator_strength                # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--small", action="store_true", help="CAS(4,4) with SmallFCI instead of CAS(8,8) with DeviceFCI")
p.add_argument("--states", type=int, default=4)
p.add_argument("--steps", type=int, default=20)
p.add_argument("--dt", type=float, default=5.0)
p.add_argument("--nroots", type=int, default=1, help="CASCI roots per training geometry")
p.add_argument("--root", type=int, default=0, help="surface of the dynamics (0 = ground state)")
p.add_argument("--spin-penalty", type=float, default=0.0, help="penalty on S^2 in the active-space solver")
p.add_argument("--resident", action="store_true", help="keep the two-body rows on the device (ResidentCAS_EVCont_obj)")
a = p.parse_args()
if not 0 <= a.root < a.nroots:
    p.error(f"--root {a.root} needs --nroots of at least {a.root + 1}")

if a.small and not a.resident:
    from evcont_amd.fci_small import SmallFCI
    ncas, nelecas, solver = 4, (2, 2), SmallFCI(spin_penalty=a.spin_penalty)
else:
    from evcont_amd.fci_device import DeviceFCI
    ncas, nelecas = (4, (2, 2)) if a.small else (8, (4, 4))
    solver = DeviceFCI(spin_penalty=a.spin_penalty)

dg = DeviceSpdGaussians(*water_shells("cc-pvdz"), nelec=(5, 5))
t0 = time.time()
if a.resident:
    from evcont_amd.resident import ResidentCAS_EVCont_obj
    cont = ResidentCAS_EVCont_obj(ncas, nelecas, cisolver=solver, nroots=a.nroots, layout="sym8")
else:
    cont = CAS_EVCont_obj(ncas, nelecas, cisolver=solver, nroots=a.nroots)
for r in np.linspace(0.90, 1.08, a.states) * ANGSTROM:      # symmetric stretch around the equilibrium bond length
    cont.append_to_rdms(dg.to_mol(water_coords(r_oh=r), need_grad=False))
print(f"{cont.ntrain} CAS({sum(nelecas)},{ncas}) training states ({a.nroots} per geometry) of water / cc-pVDZ (N = {cont.one_rdm.shape[-1]}): "
      f"{time.time() - t0:.1f} s, E = " + " ".join(f"{e:.6f}" for e in cont.ens))

init = dg.to_mol(water_coords(r_oh=1.06 * 0.9572 * ANGSTROM))       # a stretched start: the molecule vibrates
# what the excited-state calls read: the host arrays, or the resident container's view
arrays, kw = ((cont.one_rdm, None, cont.overlap), dict(device_trdms=cont.device_trdms())) if a.resident else \
    ((cont.one_rdm, cont.two_rdm, cont.overlap), {})
if a.nroots > 1:
    pairs = [(0, k) for k in range(1, a.nroots)]
    E, props = get_multistate_properties([init], *arrays, a.nroots, pairs, **kw)
    for i, (_, k) in enumerate(pairs):
        print(f"first frame: E_{k} - E_0 = {E[0, k] - E[0, 0]:.6f} Ha, f_0{k} = "
              f"{float(oscillator_strength(E[0, 0], E[0, k], props['dipole'][0, i])):.6f}")
t0 = time.time()
frames = state_swarm([init], *arrays, root=a.root, dt=a.dt, steps=a.steps, integrals="device", **kw)
wall = time.time() - t0
for f in frames:
    r1 = np.linalg.norm(f["coord"][0, 1] - f["coord"][0, 0]) / ANGSTROM
    print(f"t = {f['time']:7.1f}  r(OH) = {r1:.4f} A  E_pot = {f['epot'][0]:.10f}  E_tot = {f['epot'][0] + f['ekin'][0]:.10f}")
etot = np.array([f["epot"][0] + f["ekin"][0] for f in frames])
print(f"{a.steps} NVE steps with integrals on the device: {wall:.2f} s wall, drift of the total energy "
      f"{np.abs(etot - etot[0]).max():.2e} Ha")
assert np.all(np.isfinite(etot))
print("OK")
