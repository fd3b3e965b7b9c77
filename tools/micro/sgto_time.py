"""Device time of the s-Gaussian AO integrals evc_sgto_integrals_batch (csrc/sgto.hip) at H10, H20 and H30 (1.8 Bohr,
STO-3G), one geometry and 32 per call, packed (s4 / s2kl, with derivatives) and energy-only: HIP events around the C
call alone, coordinates and outputs resident, median of 20 calls after 3 warm-up calls.  Beside each: the host
``hchain.s_gaussian_mol`` of one geometry on this machine (one call, with derivatives / without), and the batched
energy+force call the integrals feed (``BatchedEvaluator`` on a seeded synthetic training set of 20 states in the
compressed layout, the same count of geometries).

The rate: primitive quartets per second, G N^2 Ms K^4 (with derivatives) or G Ms^2 K^4 (energy-only) over the time of
the whole call, and that rate times the vector instructions of one pass of the quartet loop (counted in the compiled ISA
with both branches of the Boys function, DESIGN.md section 8.2: an upper estimate, a wave whose lanes all take one branch
skips the other) against the vector issue rate of the device (its FP64 vector peak / 2 per lane).

usage: python tools/micro/sgto_time.py [--out profiles/sgto_time.txt] [--sizes 10 20 30] [--no-host]"""
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

from evcont_amd import _lib                                                  # noqa: E402
from evcont_amd.evaluator import BatchedEvaluator, DeviceTRDMs               # noqa: E402
from evcont_amd.hchain import hydrogen_chain                                 # noqa: E402
from evcont_amd.hchain_device import DeviceSGaussians                        # noqa: E402

WARM, REPS = 3, 20
SGTO_FIELDS = ("enuc", "S", "hcore", "eri", "ipovlp", "dhcore", "eri_ip1", "gnuc")
# vector instructions of one pass of the quartet loop of sgto_two_kernel<true> / <false>, both Boys branches counted (ISA)
LOOP_INSTRUCTIONS = {True: 252, False: 189}
# vector instructions per second and lane of the device: 256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz (a 64-lane FP64 or
# 32-bit instruction occupies its SIMD for 4 cycles) = the 78.6 TFLOP/s FP64 vector peak / 2
LANE_ISSUE = 256 * 4 * 16 * 2.4e9


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


def synthetic_training(n, T, device):
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sgto_time.txt"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[10, 20, 30])
    ap.add_argument("--no-host", action="store_true", help="skip the host s_gaussian_mol timings (24 s at H30)")
    args = ap.parse_args()
    d = torch.device("cuda", 0)
    lib = _lib.load()
    lines = [f"# tools/micro/sgto_time.py on {torch.cuda.get_device_name(0)}: median [min, max] ms of {REPS} calls after "
             f"{WARM}, HIP events around the C call; host: one s_gaussian_mol call on the same machine"]
    for n in args.sizes:
        mol = hydrogen_chain(n, 1.8, need_grad=False)
        K, ms = len(mol.exponents), n * (n + 1) // 2
        host = {}
        if not args.no_host:
            for grad in (True, False):
                t0 = time.perf_counter()
                hydrogen_chain(n, 1.8, need_grad=grad)
                host[grad] = time.perf_counter() - t0
        trd = synthetic_training(n, 20, d)
        lines.append(f"\nH{n} / STO-3G at 1.8 Bohr: N = {n}, Ms = {ms}, K = {K}")
        for G in (1, 32):
            R = np.repeat(mol.atom_coords()[None], G, axis=0) + 0.01 * np.random.default_rng(G).standard_normal((G, n, 3))
            dR = torch.from_numpy(R).to(d)
            sg = DeviceSGaussians.from_mol(mol, device=d)
            ev = BatchedEvaluator(trd, n, G)
            for grad in (True, False):
                aob = sg.integrals(dR, need_grad=grad, packed=True)       # (allocates the outputs and the workspace)
                out = _lib.SgtoOutputs(**{k: getattr(aob, k).data_ptr() for k in SGTO_FIELDS
                                          if getattr(aob, k) is not None})
                flags = _lib.FLAG_ERI_S4 | (_lib.FLAG_IP1_S2KL if grad else _lib.FLAG_ENERGY_ONLY)
                st = torch.cuda.current_stream(d).cuda_stream
                call = lambda: _lib.check(lib.evc_sgto_integrals_batch(
                    n, K, G, dR.data_ptr(), sg._charges.data_ptr(), sg.exponents.ctypes.data, sg.coefficients.ctypes.data,
                    C.byref(out), flags, sg._ws.data_ptr(), int(sg._ws.numel()), st), "evc_sgto_integrals_batch")
                t_ms, lo, hi = timed(call)
                quartets = G * (n * n if grad else ms) * ms * K ** 4
                rate = quartets / (t_ms * 1e-3)
                share = rate * LOOP_INSTRUCTIONS[grad] / LANE_ISSUE
                what = "packed, derivatives" if grad else "energy-only        "
                line = (f"  G = {G:2d}  {what}  {t_ms:9.4f} ms [{lo:.4f}, {hi:.4f}]  = {t_ms / G * 1e3:9.2f} us / geometry, "
                        f"{rate / 1e9:7.2f} G quartets/s, x {LOOP_INSTRUCTIONS[grad]} instructions = {100 * share:5.1f} % of "
                        f"the vector issue rate")
                if grad in host:
                    line += f";  host s_gaussian_mol {host[grad] * 1e3:10.1f} ms / geometry = {host[grad] * 1e3 * G / t_ms:9.0f} x"
                lines.append(line)
                if grad:
                    e_ms, elo, ehi = timed(lambda: ev.enqueue(aob))
                    lines.append(f"          batched energy+force call on these integrals (T = 20, sym8)  {e_ms:9.4f} ms "
                                 f"[{elo:.4f}, {ehi:.4f}]  = {e_ms / G * 1e3:9.2f} us / geometry; integrals / evaluation = "
                                 f"{t_ms / e_ms:5.2f}")
            del ev, sg
        del trd
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
