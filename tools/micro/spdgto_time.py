"""Device time of the s, p and d Gaussian AO integrals evc_spdgto_integrals_batch (csrc/spdgto.hip) for water in cc-pVDZ
(N = 24), one geometry and 32 per call, packed with derivatives: HIP events around the C call alone, coordinates and
outputs resident, median of 20 calls after 3 warm-up calls; beside it the batched energy+force call the integrals feed
(``BatchedEvaluator`` on a seeded synthetic training set of 6 states in the compressed layout, the same count of
geometries).  As the comparison with the s + p kernels: water / 6-31G (N = 13) through both ``evc_spgto_*`` and
``evc_spdgto_*`` in the same run, and their ratio.

usage: python tools/micro/spdgto_time.py [--out profiles/spdgto_time.txt]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from evcont_amd import _lib, gto_small, gto_spd                              # noqa: E402
from evcont_amd.evaluator import BatchedEvaluator                            # noqa: E402
from evcont_amd.gto_device import DeviceGaussians                            # noqa: E402
from evcont_amd.gto_spd_device import DeviceSpdGaussians                     # noqa: E402
from spgto_time import FIELDS, REPS, T, WARM, synthetic_training, timed      # noqa: E402


def time_integrals(lib, dg, R0, G, d):
    """(median, min, max) ms of the C call of ``dg`` on G shaken copies of R0, and the DeviceAOBatch it wrote."""
    A = R0.shape[0]
    R = np.repeat(R0[None], G, axis=0) + 0.01 * np.random.default_rng(G).standard_normal((G, A, 3))
    dR = torch.from_numpy(R).to(d)
    aob = dg.integrals(dR, packed=True)                           # (allocates the outputs and the workspace)
    out = _lib.SgtoOutputs(**{k: getattr(aob, k).data_ptr() for k in FIELDS})
    st = torch.cuda.current_stream(d).cuda_stream
    fn = getattr(lib, dg._INTEGRALS)
    call = lambda: _lib.check(fn(A, len(dg.shell_l), G, dR.data_ptr(), dg.charges.data_ptr(), *dg._basis_args(),
                                 C.byref(out), _lib.FLAG_ERI_S4 | _lib.FLAG_IP1_S2KL, dg._ws.data_ptr(),
                                 int(dg._ws.numel()), st), dg._INTEGRALS)
    return timed(call), aob


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "spdgto_time.txt"))
    args = ap.parse_args()
    d = torch.device("cuda", 0)
    lib = _lib.load()
    lines = [f"# tools/micro/spdgto_time.py on {torch.cuda.get_device_name(0)}: median [min, max] ms of {REPS} calls after "
             f"{WARM}, HIP events around the C call (packed forms, with derivatives)"]
    R0 = gto_spd.water_coords()
    dg = DeviceSpdGaussians(*gto_spd.water_shells("cc-pvdz"), device=d)
    n = dg.nao
    trd = synthetic_training(n, d)
    lines.append(f"\nwater / cc-pVDZ: N = {n}, Ms = {n * (n + 1) // 2}, 3 atoms, {len(dg.shell_l)} shells, "
                 f"{dg.exponents.shape[0]} primitives (evc_spdgto_integrals_batch)")
    for G in (1, 32):
        (t_ms, lo, hi), aob = time_integrals(lib, dg, R0, G, d)
        lines.append(f"  G = {G:2d}  integrals    {t_ms:9.4f} ms [{lo:.4f}, {hi:.4f}]  = {t_ms / G * 1e3:9.2f} us / geometry")
        ev = BatchedEvaluator(trd, 3, G)
        e_ms, elo, ehi = timed(lambda: ev.enqueue(aob))
        lines.append(f"          batched energy+force call on these integrals (T = {T}, sym8)  {e_ms:9.4f} ms "
                     f"[{elo:.4f}, {ehi:.4f}]  = {e_ms / G * 1e3:9.2f} us / geometry; integrals / evaluation = "
                     f"{t_ms / e_ms:5.2f}")
        del ev
    del trd, dg
    torch.cuda.empty_cache()
    mol = gto_small.water("6-31g", need_grad=False)
    old = DeviceGaussians.from_mol(mol, device=d)
    new = DeviceSpdGaussians(mol.charges, [[gto_spd.Shell(s.l, s.exponents, s.coefficients) for s in atom]
                                           for atom in mol.shells], device=d)
    lines.append(f"\nwater / 6-31G: N = {old.nao}, {old.exponents.shape[0]} primitives, the same molecule through both "
                 f"families")
    for G in (1, 32):
        (t0, lo0, hi0), _ = time_integrals(lib, old, mol.atom_coords(), G, d)
        (t1, lo1, hi1), _ = time_integrals(lib, new, mol.atom_coords(), G, d)
        lines.append(f"  G = {G:2d}  evc_spgto_integrals_batch  {t0:9.4f} ms [{lo0:.4f}, {hi0:.4f}]   "
                     f"evc_spdgto_integrals_batch {t1:9.4f} ms [{lo1:.4f}, {hi1:.4f}]   spd / sp = {t1 / t0:5.2f}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
