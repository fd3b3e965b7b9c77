"""Active-learning MD of a hydrogen chain trained on the package's own CASCI states: the reference's
``converge_EVCont_MD(CAS_EVCont_obj(ncas, neleca), mol, ...)`` with nothing third-party.

Each training state is RHF (``scf_small.rhf``) + CASCI(10,10) on the H30 / STO-3G chain (``cas_small.casci``, the
active-space eigensolver on the device: ``DeviceFCI(eigensolver="davidson")``); the transition RDMs between CAS states in
the different orbital sets of the different geometries are reduced to a non-orthogonal ``transform_ci`` and an
active-space row call and expanded to the 30 OAO orbitals on the device (``DeviceFCI.cas_trans_rdm12_rows``, DESIGN.md
8.1.5).  The MD inner loop is the evaluator's, as in examples/h30_md.py.

usage: python examples/h30_cas_md.py [--small] [--steps 20] [--dt 5] [--iterations 4] [--workdir DIR]
       --small: H8, CAS(4,4): a quick run"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evcont_amd.CASCI_EVCont import CAS_EVCont_obj          # noqa: E402
from evcont_amd.MD_utils import converge_EVCont_MD          # noqa: E402
from evcont_amd.fci_device import DeviceFCI                 # noqa: E402
from evcont_amd.hchain import hydrogen_chain                # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--small", action="store_true", help="H8, CAS(4,4)")
p.add_argument("--steps", type=int, default=20)
p.add_argument("--dt", type=float, default=5.0)
p.add_argument("--iterations", type=int, default=4, help="active-learning iterations at most")
p.add_argument("--spacing", type=float, default=1.8)
p.add_argument("--workdir", default=None)
a = p.parse_args()

natm, ncas, nact = (8, 4, 4) if a.small else (30, 10, 10)
mol = hydrogen_chain(natm, a.spacing)
cont = CAS_EVCont_obj(ncas, nact, cisolver=DeviceFCI(eigensolver="davidson"))
workdir = a.workdir or tempfile.mkdtemp(prefix="h_cas_md_")
os.makedirs(workdir, exist_ok=True)
t0 = time.perf_counter()
traj = converge_EVCont_MD(cont, mol, steps=a.steps, dt=a.dt, convergence_thresh=1e-4, max_iterations=a.iterations,
                          workdir=workdir)
dt = time.perf_counter() - t0
print(f"H{natm} CAS({nact},{ncas}), ncore = {cont.cascis[0].ncore}: {cont.ntrain} training states in {dt:.1f} s, "
      f"trajectory {traj.shape}, files in {workdir}")
print("CASCI energies of the training states:", " ".join(f"{e:.8f}" for e in cont.ens))
print("overlap of the newest state with the others:", np.array2string(cont.overlap[-1], precision=6))
assert np.isfinite(traj).all() and np.abs(np.diag(cont.overlap) - 1.0).max() < 1e-8
print("OK")
