"""Active-learning MD of a hydrogen chain trained on the package's own CASCI states: the reference's
``converge_EVCont_MD(CAS_EVCont_obj(ncas, neleca), mol, ...)`` with nothing third-party.

Each training state is RHF (``scf_small.rhf``) + CASCI(10,10) on the H30 / STO-3G chain (``cas_small.casci``, the
active-space eigensolver on the device: ``DeviceFCI(eigensolver="davidson")``); the transition RDMs between CAS states in
the different orbital sets of the different geometries are reduced to a non-orthogonal ``transform_ci`` and an
active-space row call and expanded to the 30 OAO orbitals on the device (``DeviceFCI.cas_trans_rdm12_rows``, DESIGN.md
8.1.5).  The MD inner loop is the evaluator's, as in examples/h30_md.py.

usage: python examples/h30_cas_md.py [--small] [--steps 20] [--dt 5] [--iterations 4] [--workdir DIR]
       --small: H8, CAS(4,4): a quick run
       --nroots R --root k [--spin-penalty 0.2] [--states 3]: R CASCI roots per training geometry at
       --states spacings around --spacing, then ``state_swarm`` on surface k with the integrals made on the device (the
       active-learning loop is for one root per geometry); the first frame prints the vertical excitation energies and
       the oscillator strengths from the ground state
       --resident: the training set grows on the device (``resident.ResidentCAS_EVCont_obj``): the
       two-body rows are written in place in the evaluator's sym8 layout and every call below reads
       ``cont.device_trdms()``"""
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
p.add_argument("--nroots", type=int, default=1, help="CASCI roots per training geometry")
p.add_argument("--root", type=int, default=0, help="surface of the dynamics (0 = ground state)")
p.add_argument("--spin-penalty", type=float, default=0.0, help="penalty on S^2 in the active-space solver")
p.add_argument("--states", type=int, default=3, help="training geometries of the --nroots route")
p.add_argument("--resident", action="store_true", help="keep the two-body rows on the device (ResidentCAS_EVCont_obj)")
a = p.parse_args()
if not 0 <= a.root < a.nroots:
    p.error(f"--root {a.root} needs --nroots of at least {a.root + 1}")

natm, ncas, nact = (8, 4, 4) if a.small else (30, 10, 10)
mol = hydrogen_chain(natm, a.spacing)
solver = DeviceFCI(eigensolver="davidson", spin_penalty=a.spin_penalty)
if a.resident:
    from evcont_amd.resident import ResidentCAS_EVCont_obj
    cont = ResidentCAS_EVCont_obj(ncas, nact, cisolver=solver, nroots=a.nroots, layout="sym8")
else:
    cont = CAS_EVCont_obj(ncas, nact, cisolver=solver, nroots=a.nroots)
# what the excited-state calls read: the host arrays, or the resident container's view
data = lambda: ((cont.one_rdm, None, cont.overlap), dict(device_trdms=cont.device_trdms())) if a.resident else \
    ((cont.one_rdm, cont.two_rdm, cont.overlap), {})
if a.nroots > 1:
    from evcont_amd.MD_utils import state_swarm
    from evcont_amd.ab_initio_eigenvector_continuation import get_multistate_properties
    from evcont_amd.properties import oscillator_strength
    t0 = time.perf_counter()
    for d in a.spacing + 0.05 * (np.arange(a.states) - (a.states - 1) / 2):
        cont.append_to_rdms(hydrogen_chain(natm, float(d), need_grad=False))
    print(f"H{natm} CAS({nact},{ncas}): {cont.ntrain} training states ({a.nroots} per geometry) in "
          f"{time.perf_counter() - t0:.1f} s")
    pairs = [(0, k) for k in range(1, a.nroots)]
    arrays, kw = data()
    E, props = get_multistate_properties([mol], *arrays, a.nroots, pairs, **kw)
    for i, (_, k) in enumerate(pairs):
        print(f"first frame: E_{k} - E_0 = {E[0, k] - E[0, 0]:.6f} Ha, f_0{k} = "
              f"{float(oscillator_strength(E[0, 0], E[0, k], props['dipole'][0, i])):.6f}")
    frames = state_swarm([mol], *arrays, root=a.root, dt=a.dt, steps=a.steps, integrals="device", **kw)
    etot = np.array([f["epot"][0] + f["ekin"][0] for f in frames])
    print(f"{a.steps} NVE steps on root {a.root}: E_tot = {etot[0]:.10f}, drift {np.abs(etot - etot[0]).max():.2e} Ha")
    assert np.isfinite(etot).all()
    print("OK")
    sys.exit(0)
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
