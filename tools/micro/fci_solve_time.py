"""Where the time of ``DeviceFCI.kernel`` goes, for the two eigensolvers, at H10 (5,5) and H12 (6,6), one and two roots
(hydrogen chain at spacing 1.8 Bohr; ``--cibasis OAO``: the Loewdin basis, ``--cibasis canonical``: the Hartree-Fock
basis of scf_small.rhf; ``--cibasis OAO canonical`` writes both, one after the other):

  host      ``DeviceFCI()``: scipy's eigsh on the host, every product a device sigma vector that is uploaded and downloaded
  davidson  ``DeviceFCI(eigensolver="davidson")``: block Davidson on device-resident vectors (csrc/fci_solve.hip)
  warm      the same with ``ci0`` = the converged vectors of a chain whose spacing differs by 0.05 Bohr

For each: the wall time of one ``kernel`` call (the second of two; the first pays the allocations), the number of sigma
vectors, and for the Davidson runs the device time of every kind of call, from HIP events around each call, summed over
the run and per iteration.

usage: python tools/micro/fci_solve_time.py [--out profiles/fci_solve_time.txt] [--sizes 10 12] [--roots 1 2]
                                            [--cibasis OAO canonical]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from evcont_amd import fci_device                                            # noqa: E402
from evcont_amd.electron_integral_utils import get_basis, get_integrals      # noqa: E402
from evcont_amd.fci_device import DeviceFCI                                  # noqa: E402
from evcont_amd.hchain import hydrogen_chain                                 # noqa: E402

KINDS = ("sigma", "dots", "combine", "correction", "hdiag")


class TimedOps(fci_device._DeviceOps):
    """The device back-end with a pair of HIP events around every call of the five kinds."""

    events = None

    def _timed(self, kind, fn, *a):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn(*a)
        e.record()
        TimedOps.events.append((kind, s, e))
        return out

    def prepare(self, *a):
        return self._timed("hdiag", super().prepare, *a)

    def sigma(self, *a):
        return self._timed("sigma", super().sigma, *a)

    def dots(self, *a):
        return self._timed("dots", super().dots, *a)

    def combine(self, *a):
        return self._timed("combine", super().combine, *a)

    def correction(self, *a):
        return self._timed("correction", super().correction, *a)


class CountingHost(DeviceFCI):
    nsigma = 0

    def _sigma(self, *a):
        self.nsigma += 1
        return super()._sigma(*a)


def integrals(norb, d, cibasis="OAO"):
    mol = hydrogen_chain(norb, d, need_grad=False)
    return get_integrals(mol, get_basis(mol, cibasis))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fci_solve_time.txt"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[10, 12])
    ap.add_argument("--roots", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--cibasis", nargs="*", choices=("OAO", "canonical"), default=["OAO"])
    args = ap.parse_args()
    lines = [f"# tools/micro/fci_solve_time.py on {torch.cuda.get_device_name(0)}: wall time of the second of two "
             f"DeviceFCI.kernel calls; device ms from HIP events around each call of the Davidson back-end (the events "
             f"of dots / correction include the small download that follows the kernels)"]
    plain = fci_device._DeviceOps
    for norb, cibasis in ((n, b) for n in args.sizes for b in args.cibasis):
        nelec = (norb // 2, norb // 2)
        h1, h2 = integrals(norb, 1.8, cibasis)
        g1, g2 = integrals(norb, 1.85, cibasis)
        for nroots in args.roots:
            host = CountingHost()
            host.kernel(h1, h2, norb, nelec, nroots=nroots)
            host.nsigma = 0
            t_host, (e_host, _) = wall(lambda: host.kernel(h1, h2, norb, nelec, nroots=nroots))
            dav = DeviceFCI(eigensolver="davidson")
            dav.kernel(h1, h2, norb, nelec, nroots=nroots)
            t_dav, (e_dav, _) = wall(lambda: dav.kernel(h1, h2, norb, nelec, nroots=nroots))
            info = dict(dav.davidson_info)
            _, near = dav.kernel(g1, g2, norb, nelec, nroots=nroots)
            t_warm, (e_warm, _) = wall(lambda: dav.kernel(h1, h2, norb, nelec, nroots=nroots, ci0=near))
            winfo = dict(dav.davidson_info)
            dim = dav._basis[1].shape[1]
            de = np.abs(np.atleast_1d(e_host) - np.atleast_1d(e_dav)).max()
            lines.append(f"\nH{norb} {nelec}, {cibasis} basis, {dim} determinants, {nroots} root(s): "
                         f"|E_davidson - E_host| = {de:.1e}, "
                         f"|E_warm - E_host| = {np.abs(np.atleast_1d(e_host) - np.atleast_1d(e_warm)).max():.1e}")
            lines.append(f"  host      {1e3 * t_host:9.1f} ms wall, {host.nsigma:4d} sigma vectors "
                         f"({1e3 * t_host / host.nsigma:.2f} ms per product, up- and download included)")
            for name, t, inf in (("davidson", t_dav, info), ("warm", t_warm, winfo)):
                lines.append(f"  {name:9s} {1e3 * t:9.1f} ms wall, {inf['nsigma']:4d} sigma vectors, {inf['iterations']} "
                             f"iterations, {inf['restarts']} restarts, converged={bool((inf['residuals'] <= dav.conv_tol).all())}")
            # the same Davidson run again with events around every call
            TimedOps.events = []
            fci_device._DeviceOps = TimedOps
            try:
                t_ev, _ = wall(lambda: dav.kernel(h1, h2, norb, nelec, nroots=nroots))
            finally:
                fci_device._DeviceOps = plain
            its = dav.davidson_info["iterations"]
            ms = {k: 0.0 for k in KINDS}
            cnt = {k: 0 for k in KINDS}
            for kind, s, e in TimedOps.events:
                ms[kind] += s.elapsed_time(e)
                cnt[kind] += 1
            total = sum(ms.values())
            lines.append(f"  davidson with events: {1e3 * t_ev:.1f} ms wall, {total:.1f} ms inside the calls, {its} iterations")
            for k in KINDS:
                lines.append(f"    {k:10s} {cnt[k]:5d} calls {ms[k]:9.2f} ms  {ms[k] / max(cnt[k], 1):7.3f} ms per call  "
                             f"{ms[k] / its:7.3f} ms per iteration  {100 * ms[k] / total:5.1f} %")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
