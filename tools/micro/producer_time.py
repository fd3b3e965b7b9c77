"""Host time of one ``integrals`` call of the three device integral producers (``DeviceSGaussians``, ``DeviceGaussians``,
``DeviceSpdGaussians``): what the Python side adds around the C call.  Small molecules (H4, water / STO-3G, an s + p + d
centre beside an s centre) at G = 1 and 2, device-resident coordinates, packed with derivatives, so that the kernels are
short and the wrapper shows: wall time of 200 back-to-back calls after 20 warm-up calls, one synchronisation at the end,
per call; median [min, max] of 7 such loops.

usage: python tools/micro/producer_time.py [--out profiles/producer_time.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from evcont_amd import gto_small, gto_spd, hchain                            # noqa: E402
from evcont_amd.MD_utils import _device_producer                             # noqa: E402

WARM, CALLS, LOOPS = 20, 200, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "producer_time.txt"))
    args = ap.parse_args()
    d = torch.device("cuda", 0)
    sh = gto_spd.Shell
    mols = (("H4", hchain.hydrogen_chain(4, 1.8, need_grad=False)),
            ("water / STO-3G", gto_small.water("sto-3g", need_grad=False)),
            ("s+p+d centre and s centre", gto_spd.spd_gaussian_mol(
                [[0.0, 0.0, 0.0], [0.9, -0.6, 1.3]], [3.0, 1.0],
                [[sh(0, [1.1], [1.0]), sh(1, [0.9], [1.0]), sh(2, [0.8], [1.0])], [sh(0, [0.7], [1.0])]], need_grad=False)))
    lines = [f"# tools/micro/producer_time.py on {torch.cuda.get_device_name(0)}: us per integrals(R, packed=True) call, wall "
             f"time of {CALLS} calls and one synchronisation, median [min, max] of {LOOPS} loops"]
    for name, mol in mols:
        p = _device_producer(mol).from_mol(mol, device=d)
        for G in (1, 2):
            R = torch.from_numpy(np.repeat(mol.atom_coords()[None], G, axis=0)).to(d)
            for _ in range(WARM):
                p.integrals(R, packed=True)
            torch.cuda.synchronize()
            us = []
            for _ in range(LOOPS):
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    p.integrals(R, packed=True)
                torch.cuda.synchronize()
                us.append((time.perf_counter() - t0) / CALLS * 1e6)
            lines.append(f"{type(p).__name__:20s} {name:28s} G = {G}  {statistics.median(us):8.2f} us [{min(us):.2f}, {max(us):.2f}]")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
