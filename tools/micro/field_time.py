"""Device time of the electric-field calls of csrc/field.hip beside the integrals call they follow, and what one
finite-field response costs against the displaced-geometry route to the same atomic polar tensor.

Part 1, at H30 / STO-6G, water / 6-31G and water / cc-pVDZ, 32 geometries each: the producer's ``integrals`` call (packed
forms, with gradients), ``dipole_integrals``, ``dipole_grad_integrals`` and ``evc_field_fold_batch``; HIP events around
``inner`` back-to-back calls on one stream, median of 7 windows after 2 warm-up windows, per call.

Part 2, water / STO-3G with three FCI training states, two roots: wall time (host clock around work that ends in a
device synchronise; the second of two calls) of ``get_multistate_field_response`` on both routes -- seven field points,
one batched call -- against ``get_multistate_properties`` over the 6A = 18 displaced geometries whose dipoles give the
same tensor by central differences.

usage: python tools/micro/field_time.py [--out profiles/field_time.txt] [--count 32]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from evcont_amd import _lib, gto_small, gto_spd                              # noqa: E402
from evcont_amd.hchain import STO6G_H_COEFFICIENTS, STO6G_H_EXPONENTS, s_gaussian_mol   # noqa: E402

DEV = "cuda"


def per_call_ms(call, inner, windows=7, warm=2):
    times = []
    for w in range(warm + windows):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(inner):
            call()
        e.record()
        torch.cuda.synchronize()
        if w >= warm:
            times.append(s.elapsed_time(e) / inner)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def producers(count):
    chain = np.zeros((30, 3))
    chain[:, 0] = 1.8 * np.arange(30)
    from evcont_amd.gto_device import DeviceGaussians
    from evcont_amd.gto_spd_device import DeviceSpdGaussians
    from evcont_amd.hchain_device import DeviceSGaussians
    w = gto_small.water("6-31g", need_grad=False)
    Z, shells = gto_spd.water_shells("cc-pvdz")
    rng = np.random.default_rng(1)
    shake = lambda R: np.stack([R + 0.05 * rng.standard_normal(R.shape) for _ in range(count)])
    yield ("H30 / STO-6G", DeviceSGaussians(np.ones(30), STO6G_H_EXPONENTS, STO6G_H_COEFFICIENTS, device=DEV),
           shake(chain), 1)
    yield "water / 6-31G", DeviceGaussians.from_mol(w, device=DEV), shake(w.coords), 4
    yield "water / cc-pVDZ", DeviceSpdGaussians(Z, shells, device=DEV), shake(gto_spd.water_coords()), 1


def kernels(count, lines):
    origin = (0.1, -0.2, 0.3)
    o = (C.c_double * 3)(*origin)
    for name, sg, R, inner in producers(count):
        aob = sg.integrals(R, packed=True)
        Rd = sg.staged_coords(count)
        n, A = int(aob.S.shape[-1]), int(Rd.shape[1])
        F = torch.from_numpy(0.01 * np.random.default_rng(2).standard_normal((count, 3))).to(DEV)
        dip, ipdip = sg.dipole_integrals(Rd, origin), sg.dipole_grad_integrals(Rd, origin)
        st = torch.cuda.current_stream().cuda_stream

        def fold():
            _lib.check(sg.lib.evc_field_fold_batch(
                n, A, count, dip.data_ptr(), ipdip.data_ptr(), aob.aoslices.data_ptr(), sg.charges.data_ptr(),
                Rd.data_ptr(), F.data_ptr(), C.cast(o, C.c_void_p), 0, aob.hcore.data_ptr(), aob.dhcore.data_ptr(),
                aob.enuc.data_ptr(), aob.gnuc.data_ptr(), st), "evc_field_fold_batch")

        t_int = per_call_ms(lambda: sg.integrals(Rd, packed=True), inner)
        lines.append(f"\n{name}, N = {n}, {count} geometries: integrals (packed, with gradients) {t_int[0]:.3f} ms "
                     f"[{t_int[1]:.3f} .. {t_int[2]:.3f}]")
        total = 0.0
        for what, call in (("dipole_integrals", lambda: sg.dipole_integrals(Rd, origin)),
                           ("dipole_grad_integrals", lambda: sg.dipole_grad_integrals(Rd, origin)),
                           ("evc_field_fold_batch", fold)):
            t = per_call_ms(call, 50)
            total += t[0]
            lines.append(f"  {what:24s} {1e3 * t[0]:9.2f} us [{1e3 * t[1]:.2f} .. {1e3 * t[2]:.2f}]  "
                         f"{100 * t[0] / t_int[0]:7.3f} % of the integrals call")
        t_all = per_call_ms(lambda: sg.integrals(Rd, packed=True, field=F, origin=origin), inner)
        lines.append(f"  the three together {1e3 * total:.2f} us = {100 * total / t_int[0]:.3f} %; integrals(..., field=) "
                     f"{t_all[0]:.3f} ms [{t_all[1]:.3f} .. {t_all[2]:.3f}]")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def response(lines):
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    from evcont_amd.ab_initio_eigenvector_continuation import (get_multistate_field_response,
                                                               get_multistate_properties)
    from evcont_amd.fci_small import SmallFCI
    cont = FCI_EVCont_obj(cisolver=SmallFCI(), cibasis="OAO")
    for r, ang in ((1.6, 100.0), (1.85, 106.0), (2.2, 112.0)):
        cont.append_to_rdms(gto_small.water("sto-3g", r, ang, need_grad=False))
    S, one, two = cont.overlap, cont.one_rdm, cont.two_rdm
    mol = gto_small.water("sto-3g", 1.8088, 104.5)
    h, k = 1e-3, 4e-3
    lines.append("\nwater / STO-3G, three FCI training states, two roots; wall time of the second of two calls:")
    res = {}
    for route in ("device", "host"):
        fn = lambda: get_multistate_field_response(mol, one, two, S, 2, h, integrals=route)
        fn()
        t, res[route] = wall(fn)
        lines.append(f"  get_multistate_field_response(integrals={route!r}), 7 field points: {1e3 * t:9.1f} ms")

    def displaced():
        mols = []
        for a in range(3):
            for x in range(3):
                for s in (k, -k):
                    R = mol.coords.copy()
                    R[a, x] += s
                    mols.append(mol.with_coords(R, need_grad=False))
        mu = get_multistate_properties(mols, one, two, S, 2)[1]["dipole"]            # (18, 2, 3)
        return ((mu[0::2] - mu[1::2]) / (2 * k)).reshape(3, 3, 2, 3).transpose(2, 0, 1, 3)

    displaced()
    t, apt = wall(displaced)
    lines.append(f"  get_multistate_properties over 6A = 18 displaced geometries (host integrals): {1e3 * t:9.1f} ms")
    lines.append(f"  max |apt(finite field, h = {h}) - apt(displaced, k = {k})| = "
                 f"{np.abs(res['device']['apt'] - apt).max():.2e}; device - host route "
                 f"{np.abs(res['device']['apt'] - res['host']['apt']).max():.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "field_time.txt"))
    ap.add_argument("--count", type=int, default=32)
    args = ap.parse_args()
    lines = [f"# tools/micro/field_time.py on {torch.cuda.get_device_name(0)}: HIP events around back-to-back calls, "
             f"median [min .. max] of 7 windows after 2, per call"]
    kernels(args.count, lines)
    response(lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
