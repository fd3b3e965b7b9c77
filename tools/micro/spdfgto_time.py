"""Device time of the s, p, d and f Gaussian AO integrals evc_spdfgto_integrals_batch (csrc/spdfgto.hip), one geometry
and 32 per call, packed with derivatives: HIP events around the C call alone, coordinates and outputs resident, median
of REPS calls after WARM warm-up calls (tools/micro/spgto_time.py), for

  the two-centre s + f / p + d + f molecule of the tests (N = 23),
  the even-tempered basis of the cc-pVTZ shape (tests/spdfgto_cases.tz_shape_water, N = 58), beside the batched
  energy+force call its integrals feed (a seeded synthetic training set in the compressed layout), and
  water / cc-pVDZ (N = 24) through ``evc_spdfgto_*`` beside ``evc_spdgto_*`` in the same run, and their ratio.

The large shapes are timed with fewer calls (``--reps``), each of them being seconds at G = 32.

usage: python tools/micro/spdfgto_time.py [--out profiles/spdfgto_time.txt] [--reps 5]"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import spgto_time                                                            # noqa: E402
from evcont_amd import _lib, gto_spd, gto_spdf                               # noqa: E402
from evcont_amd.evaluator import BatchedEvaluator                            # noqa: E402
from evcont_amd.gto_spd_device import DeviceSpdGaussians                     # noqa: E402
from evcont_amd.gto_spdf_device import DeviceSpdfGaussians                   # noqa: E402
from spdgto_time import time_integrals                                       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "spdfgto_time.txt"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import spdfgto_cases as fc
    spgto_time.REPS, spgto_time.WARM = args.reps, 1
    d = torch.device("cuda", 0)
    lib = _lib.load()
    lines = [f"# tools/micro/spdfgto_time.py on {torch.cuda.get_device_name(0)}: median [min, max] ms of {args.reps} calls "
             f"after 1, HIP events around the C call (packed forms, with derivatives)"]

    def row(dg, R0, G):
        (t_ms, lo, hi), aob = time_integrals(lib, dg, R0, G, d)
        lines.append(f"  G = {G:2d}  {dg._INTEGRALS:28s} {t_ms:10.3f} ms [{lo:.3f}, {hi:.3f}]  = {t_ms / G:9.3f} ms / geometry")
        print(lines[-1], flush=True)
        return t_ms, aob

    R0, Z, shells = fc.two_centre()
    dg = DeviceSpdfGaussians(Z, shells, device=d)
    lines.append(f"\ntwo-centre s + f / p + d + f: N = {dg.nao}, {dg.exponents.shape[0]} primitives")
    for G in (1, 32):
        row(dg, R0, G)
    new = DeviceSpdfGaussians(*gto_spd.water_shells("cc-pvdz"), device=d)
    old = DeviceSpdGaussians(*gto_spd.water_shells("cc-pvdz"), device=d)
    lines.append(f"\nwater / cc-pVDZ: N = {old.nao}, {old.exponents.shape[0]} primitives, the same molecule through both "
                 f"families")
    for G in (1, 32):
        t0, _ = row(old, gto_spd.water_coords(), G)
        t1, _ = row(new, gto_spd.water_coords(), G)
        lines.append(f"          spdf / spd = {t1 / t0:5.2f}")
    del old, new, dg
    torch.cuda.empty_cache()
    _, R0, Z, shells = fc.tz_shape_water()
    dg = DeviceSpdfGaussians(Z, shells, device=d)
    n = dg.nao
    lines.append(f"\neven-tempered basis of the cc-pVTZ shape: N = {n}, Ms = {n * (n + 1) // 2}, "
                 f"{dg.exponents.shape[0]} primitives")
    trd = spgto_time.synthetic_training(n, d)
    for G in (1, 32):
        t_ms, aob = row(dg, R0, G)
        ev = BatchedEvaluator(trd, 3, G)
        e_ms, elo, ehi = spgto_time.timed(lambda: ev.enqueue(aob))
        lines.append(f"          batched energy+force call on these integrals (T = {spgto_time.T}, sym8)  {e_ms:9.4f} ms "
                     f"[{elo:.4f}, {ehi:.4f}]; integrals / evaluation = {t_ms / e_ms:7.1f}")
        del ev, aob
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
