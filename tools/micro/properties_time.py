"""Device time of the observables call, H30 shape (N = 30, A = 30, T = 20, sym8, int2e packed), for G = 1 and G = 32
geometries with 1 root and with 4 roots + 6 transition pairs: evc_properties_roots_batch alone (every output but d_ao) on
the workspace an energy-only call left, next to the host route it replaces -- download of D (the roots call's d_pred) and
X of every geometry plus the numpy statement (evcont_amd/properties.py).

    python tools/micro/properties_time.py [--reps R]      # -> profiles/properties_time.txt

Device times: CUDA events around the call alone, median [min, max] of R repetitions after 3 warm-up calls, in two
interleaved rounds.  Host route: wall clock of the two downloads (synchronised) and of the numpy work, the same
repetitions; the energy-only call that precedes both routes is not in either number."""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from evcont_amd import properties as pr
from evcont_amd.evaluator import BatchedEvaluator, DeviceAOBatch, DeviceTRDMs
from evcont_amd.synthetic import make_device_ao, make_device_trdm_rows

dev = torch.device("cuda:0")
N, A, T, NROOTS = 30, 30, 20, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    S, one, rows = make_device_trdm_rows(N, T, 2, 1234, dev)
    trd = DeviceTRDMs.from_device_rows(one, rows, S, 2)
    del rows
    trd.compress_sym8_()
    one_host = trd.one[:, : N * N].cpu().numpy().reshape(T, T, N, N)
    rng = np.random.default_rng(1)
    diag1 = [(0, 0)]
    allp = [(k, k) for k in range(NROOTS)] + [(k, l) for k in range(NROOTS) for l in range(k + 1, NROOTS)]
    print(f"H30 shape: N={N} A={A} T={T} sym8; evc_properties_roots_batch (d_oao, dipole, mulliken, loewdin) on the "
          f"workspace of an energy-only call; median [min, max] of {a.reps} repetitions", flush=True)
    for G in (1, 32):
        daos = [make_device_ao(N, A, 7000 + k, dev, None, ip1_rs_symmetric=True).packed_ip1(eri=True) for k in range(G)]
        aob = DeviceAOBatch.stack(daos)
        ev = BatchedEvaluator(trd, A, G)
        dip = rng.standard_normal((G, 3, N, N))
        dip = torch.from_numpy(dip + dip.transpose(0, 1, 3, 2)).to(dev)
        charges = torch.ones(A, dtype=torch.float64, device=dev)
        coords = torch.from_numpy(rng.uniform(-5, 5, (G, A, 3))).to(dev)
        ev.enqueue(aob, NROOTS, energy_only=True)
        ev.synchronize()
        per_geo = ev.lib.evc_workspace_bytes(C.byref(trd.cstruct), A)
        Sh, diph, Rh, sl = aob.S.cpu().numpy(), dip.cpu().numpy(), coords.cpu().numpy(), aob.aoslices.cpu().numpy()
        for name, pairs in (("1 root", diag1), ("4 roots + 6 transitions", allp)):
            P = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32))
            want = ("d_oao", "dipole", "mulliken", "loewdin")

            def device():
                return ev._properties_device(aob, ev.coeffs, NROOTS, P, dip, charges, coords, (0.0, 0.0, 0.0), want)

            def timed_device():
                for _ in range(3):
                    device()
                torch.cuda.synchronize(dev)
                ts = []
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    device()
                    e1.record()
                    torch.cuda.synchronize(dev)
                    ts.append(e0.elapsed_time(e1) * 1e3)
                return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

            res = device()
            torch.cuda.synchronize(dev)
            D_dev = res["d_oao"]                                          # (P, G, N, N): what the host route downloads

            def host():
                t0 = time.perf_counter()
                D = D_dev.cpu().numpy()
                X = np.stack([ev.ws[g * per_geo: g * per_geo + N * N * 8].view(torch.float64).cpu().numpy()
                              for g in range(G)]).reshape(G, N, N)
                t1 = time.perf_counter()
                out = np.zeros((len(pairs), G, 3))
                for p, (k, l) in enumerate(pairs):
                    for g in range(G):
                        Pao = X[g] @ D[p, g] @ X[g].T
                        out[p, g] = pr.dip_moment(np.ones(A), Rh[g], diph[g], Pao, transition=k != l)
                        pr.mulliken_pop(Pao, Sh[g], sl)
                        pr.loewdin_pop(D[p, g], sl)
                t2 = time.perf_counter()
                return (t1 - t0) * 1e6, (t2 - t1) * 1e6, out

            def timed_host():
                for _ in range(3):
                    host()
                ts = np.array([host()[:2] for _ in range(a.reps)])
                return np.median(ts, axis=0), ts.sum(axis=1).min(), ts.sum(axis=1).max()

            d1, h1 = timed_device(), timed_host()
            d2, h2 = timed_device(), timed_host()
            diff = float(np.abs(res["dipole"].cpu().numpy() - host()[2]).max())
            print(f"G={G:2d}  {name:24s} P={len(pairs):2d}  device {d1[0]:8.1f} / {d2[0]:8.1f} us  [{d1[1]:.1f}, {d1[2]:.1f}]   "
                  f"host route: download {h1[0][0]:8.1f} / {h2[0][0]:8.1f} us + numpy {h1[0][1]:8.1f} / {h2[0][1]:8.1f} us  "
                  f"[{h1[1]:.1f}, {h1[2]:.1f}]   max |dipole device - host| {diff:.1e}", flush=True)


if __name__ == "__main__":
    main()
