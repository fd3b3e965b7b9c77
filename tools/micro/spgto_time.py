"""Device time of the s and p Gaussian AO integrals evc_spgto_integrals_batch (csrc/spgto.hip) for water in STO-3G (N = 7)
and 6-31G (N = 13) and for Zundel in 6-31G (N = 28), one geometry and 32 per call, packed with derivatives: HIP events
around the C call alone, coordinates and outputs resident, median of 20 calls after 3 warm-up calls.  Beside each: the
numpy statement ``gto_small.sp_gaussian_mol`` of one geometry on this machine (one call, with derivatives), and the batched
energy+force call the integrals feed (``BatchedEvaluator`` on a seeded synthetic training set of 6 states in the compressed
layout, the same count of geometries).

usage: python tools/micro/spgto_time.py [--out profiles/spgto_time.txt] [--no-host]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from evcont_amd import _lib, gto_small                                       # noqa: E402
from evcont_amd.evaluator import BatchedEvaluator, DeviceTRDMs               # noqa: E402
from evcont_amd.gto_device import DeviceGaussians                            # noqa: E402

WARM, REPS, T = 3, 20, 6
FIELDS = ("enuc", "S", "hcore", "eri", "ipovlp", "dhcore", "eri_ip1", "gnuc")


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def synthetic_training(n, device):
    """Seeded stand-in for a training set of T states in the compressed layout (shapes and symmetries only)."""
    rng = np.random.default_rng(7)
    A = rng.standard_normal((T, T))
    S = A @ A.T / T + np.eye(T)
    d = rng.standard_normal((T, T, n, n)) / n
    one = 0.5 * (d + d.transpose(1, 0, 3, 2))
    n2 = n * n
    two = rng.standard_normal((T * (T + 1) // 2, n2 * (n2 + 1) // 2)) / n2
    return DeviceTRDMs(one, two, S, device, compress="sym8")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "spgto_time.txt"))
    ap.add_argument("--no-host", action="store_true", help="skip the numpy timings (tens of seconds for Zundel)")
    args = ap.parse_args()
    d = torch.device("cuda", 0)
    lib = _lib.load()
    lines = [f"# tools/micro/spgto_time.py on {torch.cuda.get_device_name(0)}: median [min, max] ms of {REPS} calls after "
             f"{WARM}, HIP events around the C call (packed forms, with derivatives); host: one sp_gaussian_mol call on the "
             f"same machine"]
    systems = (("water / STO-3G", lambda g: gto_small.water("sto-3g", need_grad=g)),
               ("water / 6-31G", lambda g: gto_small.water("6-31g", need_grad=g)),
               ("Zundel / 6-31G", lambda g: gto_small.zundel("6-31g", need_grad=g)))
    for name, make in systems:
        mol = make(False)
        n, A = mol.nao, mol.natm
        ms = n * (n + 1) // 2
        host = None
        if not args.no_host:
            t0 = time.perf_counter()
            make(True)
            host = time.perf_counter() - t0
        trd = synthetic_training(n, d)
        dg = DeviceGaussians.from_mol(mol, device=d)
        nprim = int(dg.exponents.shape[0])
        lines.append(f"\n{name}: N = {n}, Ms = {ms}, {A} atoms, {len(dg.shell_l)} shells, {nprim} primitives")
        for G in (1, 32):
            R = np.repeat(mol.atom_coords()[None], G, axis=0) + 0.01 * np.random.default_rng(G).standard_normal((G, A, 3))
            dR = torch.from_numpy(R).to(d)
            ev = BatchedEvaluator(trd, A, G)
            aob = dg.integrals(dR, packed=True)                   # (allocates the outputs and the workspace)
            out = _lib.SgtoOutputs(**{k: getattr(aob, k).data_ptr() for k in FIELDS})
            st = torch.cuda.current_stream(d).cuda_stream
            call = lambda: _lib.check(lib.evc_spgto_integrals_batch(
                A, len(dg.shell_l), G, dR.data_ptr(), dg.charges.data_ptr(), *dg._basis_args(), C.byref(out),
                _lib.FLAG_ERI_S4 | _lib.FLAG_IP1_S2KL, dg._ws.data_ptr(), int(dg._ws.numel()), st),
                "evc_spgto_integrals_batch")
            t_ms, lo, hi = timed(call)
            line = f"  G = {G:2d}  integrals    {t_ms:9.4f} ms [{lo:.4f}, {hi:.4f}]  = {t_ms / G * 1e3:9.2f} us / geometry"
            if host is not None:
                line += f";  host sp_gaussian_mol {host * 1e3:10.1f} ms / geometry = {host * 1e3 * G / t_ms:9.0f} x"
            lines.append(line)
            e_ms, elo, ehi = timed(lambda: ev.enqueue(aob))
            lines.append(f"          batched energy+force call on these integrals (T = {T}, sym8)  {e_ms:9.4f} ms "
                         f"[{elo:.4f}, {ehi:.4f}]  = {e_ms / G * 1e3:9.2f} us / geometry; integrals / evaluation = "
                         f"{t_ms / e_ms:5.2f}")
            del ev
        del trd, dg
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
