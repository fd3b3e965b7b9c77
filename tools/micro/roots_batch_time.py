"""Device time of excited-state forces for a batch of geometries, H30 shape (N = 30, A = 30, T = 20, sym8, int2e /
int2e_ip1 packed, G = 32): the per-geometry loop (energy-only call + evc_phase_gradient_roots, G times) against the
batched energy-only call + evc_phase_gradient_roots_batch, for 4 roots on the diagonal and 4 roots with all 6 couplings.
Also the workspace bytes per slot at H30 and at N = 58, and the largest difference between the two paths' gradients.

    python tools/micro/roots_batch_time.py [--reps R] [--ip1-only]

--ip1-only: only the batched calls at P = 1 and P = 4 (diagonal), a few times each -- the run to put under
`rocprofv3 --kernel-trace --stats` for the time of the ip1 stage (ip1_dh_kernel<8, 1> vs <8, 4>)."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from evcont_amd import _lib
from evcont_amd.evaluator import BatchedEvaluator, ContinuationEvaluator, DeviceAOBatch, DeviceTRDMs
from evcont_amd.synthetic import make_device_ao, make_device_trdm_rows

dev = torch.device("cuda:0")
N, A, T, G, NROOTS = 30, 30, 20, 32, 4


def sym8_set(n, T):
    """A descriptor of the compressed layout (sizes only: for the workspace queries)."""
    ns = n * (n + 1) // 2
    cols = ns * (ns + 1) // 2
    rows = T * (T + 1) // 2
    return _lib.TrdmSet(n=n, ntrain=T, layout=_lib.LAYOUT_SYM8, rows2=rows, row_offset=0, rows2_total=rows,
                        cols2=cols, ld2=cols + (cols & 1), ld1=n * n, two_rdm=256, one_rdm=256, s_train=256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ip1-only", action="store_true")
    a = ap.parse_args()
    lib = _lib.load()
    S, one, rows = make_device_trdm_rows(N, T, 2, 1234, dev)
    trd = DeviceTRDMs.from_device_rows(one, rows, S, 2)
    del rows
    trd.compress_sym8_()
    daos = [make_device_ao(N, A, 7000 + k, dev, None, ip1_rs_symmetric=True).packed_ip1(eri=True) for k in range(G)]
    aob = DeviceAOBatch.stack(daos)
    flags = _lib.FLAG_IP1_S2KL
    diag = [(k, k) for k in range(NROOTS)]
    allp = diag + [(k, l) for k in range(NROOTS) for l in range(k + 1, NROOTS)]
    ev1 = ContinuationEvaluator(trd, A, want_two_rdm=False)
    evb = BatchedEvaluator(trd, A, G)
    ts = C.byref(trd.cstruct)

    def loop(pairs):
        P = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32))
        ev1._grow_workspace(lib.evc_workspace_bytes_roots(ts, A, len(pairs)))
        grads = torch.zeros((G, len(pairs), A, 3), dtype=torch.float64, device=dev)
        outs = [_lib.OutputsRoots(grad=grads[g].data_ptr(), d_pred=None, g_pred=None) for g in range(G)]
        geos = [d.cstruct() for d in daos]

        def run():
            for g in range(G):
                ev1.enqueue(daos[g], NROOTS, energy_only=True)
                _lib.check(lib.evc_phase_gradient_roots(ts, C.byref(geos[g]), ev1.coeffs.data_ptr(), NROOTS,
                                                        P.ctypes.data, len(pairs), C.byref(outs[g]), flags,
                                                        ev1.ws.data_ptr(), ev1.ws_bytes, ev1._sp()),
                           "evc_phase_gradient_roots")
        return run, grads

    def batched(pairs):
        P = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32))
        evb._grow_workspace(lib.evc_workspace_bytes_roots_batch(ts, A, G, len(pairs)))
        grads = torch.zeros((len(pairs), G, A, 3), dtype=torch.float64, device=dev)
        out = _lib.OutputsRoots(grad=grads.data_ptr(), d_pred=None, g_pred=None)
        gb = aob.cstruct()

        def run():
            evb.enqueue(aob, NROOTS, energy_only=True)
            _lib.check(lib.evc_phase_gradient_roots_batch(ts, C.byref(gb), evb.coeffs.data_ptr(), NROOTS,
                                                          P.ctypes.data, len(pairs), C.byref(out), flags,
                                                          evb.ws.data_ptr(), evb.ws_bytes, evb._sp()),
                       "evc_phase_gradient_roots_batch")
        return run, grads

    def timed(run, reps):
        for _ in range(3):
            run()
        torch.cuda.synchronize(dev)
        ts_ = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize(dev)
            ts_.append(e0.elapsed_time(e1) * 1e3)
        return float(np.median(ts_)), float(np.min(ts_)), float(np.max(ts_))

    if a.ip1_only:
        for pairs in (diag[:1], diag):
            run, _ = batched(pairs)
            for _ in range(5):
                run()
            torch.cuda.synchronize(dev)
            print(f"batched P={len(pairs)}: 5 calls done", flush=True)
        return
    print(f"H30 shape: N={N} A={A} T={T} sym8, packed int2e / int2e_ip1, G={G}, {NROOTS} roots; device time per batch "
          f"of {G} geometries (median [min, max] of {a.reps} repetitions, CUDA events)", flush=True)
    for name, pairs in (("4 roots, diagonal", diag), ("4 roots + 6 couplings", allp)):
        run_l, g_l = loop(pairs)
        run_b, g_b = batched(pairs)
        # interleaved: loop, batched, loop, batched
        tl1, tb1 = timed(run_l, a.reps), timed(run_b, a.reps)
        tl2, tb2 = timed(run_l, a.reps), timed(run_b, a.reps)
        tl, tb = min(tl1[0], tl2[0]), min(tb1[0], tb2[0])
        run_l()
        run_b()
        torch.cuda.synchronize(dev)
        # (the two paths run different eigensolver launches: a coupling slot may come back with the other sign)
        gb_ = g_b.transpose(0, 1)
        sgn = torch.sign((g_l * gb_).sum(dim=(2, 3), keepdim=True))
        diff = float((g_l - sgn * gb_).abs().max())
        per = G * len(pairs)
        print(f"{name:24s} P={len(pairs):2d}  loop {tl1[0]:9.1f} / {tl2[0]:9.1f} us  [{tl1[1]:.1f}, {tl1[2]:.1f}]   "
              f"batched {tb1[0]:9.1f} / {tb2[0]:9.1f} us  [{tb1[1]:.1f}, {tb1[2]:.1f}]   "
              f"per (geometry, slot): {tl / per:7.2f} -> {tb / per:7.2f} us  ({tl / tb:4.2f}x)   "
              f"max |grad loop - grad batched| {diff:.1e} (coupling signs aligned)", flush=True)
    for n, T_ in ((30, 20), (58, 20)):
        t = sym8_set(n, T_)
        print(f"workspace per slot, N={n} T={T_} sym8: "
              f"{lib.evc_workspace_bytes_roots_batch(C.byref(t), A, 1, 1) / 2**20:8.1f} MiB "
              f"(batch of {G} x 4 roots: {lib.evc_workspace_bytes_roots_batch(C.byref(t), A, G, 4) / 2**30:6.2f} GiB)",
              flush=True)


if __name__ == "__main__":
    main()
