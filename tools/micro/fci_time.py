"""Device time of the three full-CI entry points (csrc/fci.hip) at H10 (5,5) and H12 (6,6): one t-RDM pair, one row call
of 21 kets, one sigma vector -- HIP events around the C call alone (vectors and tables resident, no host copies), median
of 20 calls after 3 warm-up calls -- next to fci_small.SmallFCI on the host CPUs of the same machine (one call each,
random normalised vectors) and next to two floors:

  matrix floor   2 N^4 dim flops (per ket; t-RDM product and the sigma GEMM alike) at the 78.6 TFLOP/s FP64 MFMA peak
  memory floor   the bytes the launches move through HBM, at 8 TB/s:
     t-RDM, K kets  D~_bra written once and read K times, each D_ket written and read once (rows x npad doubles each),
                    per ket the split-K partials written and read once (blocks x npad^2 doubles)
     sigma          D written and read once, G written once and read twice by the gather (npad x dim doubles each)

usage: python tools/micro/fci_time.py [--out profiles/fci_time.txt] [--sizes 10 12]"""
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

from evcont_amd import _lib                      # noqa: E402
from evcont_amd.fci_device import DeviceFCI      # noqa: E402
from evcont_amd.fci_small import SmallFCI        # noqa: E402

PEAK_FLOPS, PEAK_BYTES = 78.6e12, 8.0e12
WARM, REPS, KROW = 3, 20, 21


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fci_time.txt"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[10, 12])
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    lib = _lib.load()
    lines = [f"# tools/micro/fci_time.py on {torch.cuda.get_device_name(0)}: median [min, max] ms of {REPS} calls after "
             f"{WARM}, HIP events; host = fci_small.SmallFCI, one call, {os.environ.get('OMP_NUM_THREADS', '?')} threads",
             f"# floors: matrix = 2 N^4 dim K flops at {PEAK_FLOPS / 1e12} TFLOP/s, memory = bytes moved at "
             f"{PEAK_BYTES / 1e12} TB/s (formulas: docstring of the tool)"]
    for norb in args.sizes:
        nelec = (norb // 2, norb // 2)
        dev, host = DeviceFCI(), SmallFCI()
        _, dta, dtb, na, nb, grant = dev._setup(norb, nelec)
        dim, n2 = na * nb, norb * norb
        npad = dta.shape[1]
        rows = max(256, (-(-dim // 256) + 63) // 64 * 64)
        nblk = -(-dim // rows)
        rng = np.random.default_rng(norb)
        hv = []
        for _ in range(KROW):
            v = rng.standard_normal((na, nb))
            hv.append(v / np.linalg.norm(v))
        dv = [dev._upload(v, na, nb, cache=True) for v in hv]
        d = dev._device
        h1 = rng.standard_normal((norb, norb))
        h1 = 0.5 * (h1 + h1.T)
        h2 = rng.standard_normal((n2, n2))
        h2 = (0.5 * (h2 + h2.T)).reshape((norb,) * 4)
        dh1, dh2 = torch.from_numpy(h1).to(d), torch.from_numpy(h2.reshape(-1).copy()).to(d)
        ov = torch.empty(KROW, dtype=torch.float64, device=d)
        dm1 = torch.empty((KROW, n2), dtype=torch.float64, device=d)
        dm2 = torch.empty((KROW, n2 * n2), dtype=torch.float64, device=d)
        sig = torch.empty(dim, dtype=torch.float64, device=d)
        st = dev._stream()

        def trdm(K):
            ptrs = (C.c_void_p * K)(*[t.data_ptr() for t in dv[:K]])
            return lambda: _lib.check(lib.evc_fci_trdm_rows(
                norb, na, nb, dta.data_ptr(), dtb.data_ptr(), dv[0].data_ptr(), ptrs, K, ov.data_ptr(), dm1.data_ptr(),
                dm2.data_ptr(), dev._ws.data_ptr(), grant, st), "evc_fci_trdm_rows")

        sigma = lambda: _lib.check(lib.evc_fci_sigma(
            norb, na, nb, dta.data_ptr(), dtb.data_ptr(), dh1.data_ptr(), dh2.data_ptr(), dv[0].data_ptr(),
            sig.data_ptr(), dev._ws.data_ptr(), grant, st), "evc_fci_sigma")

        dbytes = nblk * rows * npad * 8
        pbytes = nblk * npad * npad * 8
        ldg = (dim + 63) // 64 * 64
        cases = [("t-RDM pair", trdm(1), 1, 2 * dbytes + 2 * dbytes + 2 * pbytes),
                 (f"t-RDM row of {KROW}", trdm(KROW), KROW, (1 + KROW) * dbytes + 2 * KROW * dbytes + 2 * KROW * pbytes),
                 ("sigma vector", sigma, 1, 5 * npad * ldg * 8)]
        lines.append(f"\nH{norb} {nelec}: {dim} determinants, npad {npad}, {nblk} split-K blocks of {rows}; workspace "
                     f"{grant / 2 ** 20:.0f} MiB; kernels: ")
        med = {}
        for name, fn, K, nbytes in cases:
            m, lo, hi = timed(fn)
            med[name] = m
            f_ms = 2.0 * n2 * n2 * dim * K / PEAK_FLOPS * 1e3
            b_ms = nbytes / PEAK_BYTES * 1e3
            floor = max(f_ms, b_ms)
            lines.append(f"  {name:16s} {m:9.3f} ms [{lo:.3f}, {hi:.3f}]   matrix floor {f_ms:8.4f} ms, memory floor "
                         f"{b_ms:8.4f} ms ({nbytes / 1e6:.0f} MB): {100 * floor / m:5.1f} % of the larger floor")
        lines[-4] += ", ".join(lib.evc_profile_kernel(s).decode() for s in (9, 10))
        lines.append(f"  row of {KROW} / {KROW} single pairs: {med[f't-RDM row of {KROW}'] / (KROW * med['t-RDM pair']):.3f}")
        if not args.no_host:
            t0 = time.perf_counter()
            host._ops(norb, nelec)
            t1 = time.perf_counter()
            host.trans_rdm12(hv[0], hv[1], norb, nelec)
            t2 = time.perf_counter()
            host.contract(h1, h2, hv[0], norb, nelec)
            t3 = time.perf_counter()
            lines.append(f"  host SmallFCI: trans_rdm12 pair {1e3 * (t2 - t1):.0f} ms, contract {1e3 * (t3 - t2):.0f} ms "
                         f"(operator tables {t1 - t0:.1f} s, once)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
