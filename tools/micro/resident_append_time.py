"""What one appended training state costs around the t-RDM row call, for T = 1 ... 20 at H10 (5,5) and H12 (6,6)
(hydrogen chains, OAO basis, ``DeviceFCI(eigensolver="davidson")``), on the two routes, in one process, with the same
CI vectors (each state is solved once):

  host      ``FCI_EVCont_obj._append_root``: ``trans_rdm12_rows`` (the dense K x N^4 rows come to the host), then
            ``_append_state`` (``containers.grow_trdms``, ``_invalidate``); then ``device_trdms("sym8")`` (numpy
            ``pack_rows`` over all T^2 blocks, upload, ``compress_sym8_``)
  resident  ``resident.ResidentFCI_EVCont_obj._append_root``: the vector's one upload, ``trans_rdm12_rows_packed`` into
            the device matrix, the host record; then ``device_trdms()`` (a view)

Each route runs the container's own code; the solver's row call is timed by a subclass that wraps it (``TimedFCI``).  Per
append and route the wall time (host clock, the device synchronised at both ends) inside the row call and of everything
else from the start of ``_append_root`` to a usable sym8 ``DeviceTRDMs``; the solve once.  The routes alternate at every T.  A first, untimed pass at
T = 1 ... 2 of each route pays the allocations and loads the kernels.  Host memory: ``tracemalloc`` (numpy buffers are
traced) -- what a route holds after the last append and the highest level it reached during one.

usage: python tools/micro/resident_append_time.py [--out profiles/resident_append_time.txt] [--sizes 10 12] [--states 20]"""
import argparse
import os
import sys
import time
import tracemalloc

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from evcont_amd.FCI_EVCont import FCI_EVCont_obj                             # noqa: E402
from evcont_amd.electron_integral_utils import get_basis, get_integrals      # noqa: E402
from evcont_amd.fci_device import DeviceFCI                                  # noqa: E402
from evcont_amd.hchain import hydrogen_chain                                 # noqa: E402
from evcont_amd.resident import ResidentFCI_EVCont_obj                       # noqa: E402


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


class Memory:
    """Traced host bytes of one route: what it holds, and the highest level during one of its steps."""

    def __init__(self):
        self.held = 0
        self.peak = 0

    def __enter__(self):
        self.start = tracemalloc.get_traced_memory()[0]
        tracemalloc.reset_peak()
        return self

    def __exit__(self, *exc):
        now, peak = tracemalloc.get_traced_memory()
        self.peak = max(self.peak, self.held + peak - self.start)
        self.held += now - self.start


class TimedFCI(DeviceFCI):
    """DeviceFCI whose two row calls are timed (device synchronised at both ends); the containers run their own code."""

    rows_s = 0.0

    def _timed(self, fn, *a):
        t0 = clock()
        out = fn(*a)
        self.rows_s += clock() - t0
        return out

    def trans_rdm12_rows(self, *a):
        return self._timed(super().trans_rdm12_rows, *a)

    def trans_rdm12_rows_packed(self, *a):
        return self._timed(super().trans_rdm12_rows_packed, *a)


def append(c, layout, vec, energy, n, nelec):
    """One trained root through the container's own ``_append_root``, then the first ``device_trdms`` after it:
    (seconds inside the solver's row call, seconds of everything else, the DeviceTRDMs)."""
    solver = c.cisolver
    solver.rows_s = 0.0
    t0 = clock()
    c._append_root(vec, energy, len(c.mol_index), n, nelec)
    trd = c.device_trdms(layout)
    total = clock() - t0
    return solver.rows_s, total - solver.rows_s, trd


def run(norb, states, solver, lines, warm=False):
    nelec = (norb // 2, norb // 2)
    host = FCI_EVCont_obj(cisolver=solver, cibasis="OAO")
    res = ResidentFCI_EVCont_obj(cisolver=solver, cibasis="OAO", layout="sym8", capacity=4)
    mem = {"host": Memory(), "resident": Memory()}
    rows = []
    for k in range(states):
        mol = hydrogen_chain(norb, 1.4 + 0.08 * k, need_grad=False)
        h1, h2 = get_integrals(mol, get_basis(mol, "OAO"))
        t0 = clock()
        e, vec = solver.kernel(h1, h2, norb, nelec)
        t_solve = clock() - t0
        order = (("host", "sym8", host), ("resident", None, res))
        out = {}
        for name, layout, c in (order if k % 2 == 0 else order[::-1]):
            with mem[name]:
                out[name] = append(c, layout, vec, e, norb, nelec)
        # (the host route compresses from the packed (T,T,M) form, which holds one of dm2[pq,rs] / dm2[rs,pq]: the two
        # routes sum elements that agree to rounding only, so their rows are compared by their largest difference)
        same = float((out["host"][2].two - out["resident"][2].two).abs().max())
        rows.append((k + 1, t_solve, out["host"][0], out["host"][1], out["resident"][0], out["resident"][1], same))
    if warm:
        return
    dim = int(np.asarray(host.fcivecs[0]).size)
    lines.append(f"\nH{norb} {nelec}, {dim} determinants, sym8 rows of {res.device_trdms().cols} columns; ms wall per append")
    lines.append("   T    solve | host: row call   around the row call | resident: row call   around the row call | max |row difference|")
    for T, ts, hr, ha, rr, ra, same in rows:
        lines.append(f"  {T:2d} {1e3 * ts:8.1f} | {1e3 * hr:14.2f} {1e3 * ha:20.2f} | {1e3 * rr:18.2f} {1e3 * ra:20.2f} | {same:.1e}")
    T, _, hr, ha, rr, ra, _ = rows[-1]
    lines.append(f"  at T = {T}: around the row call {1e3 * ha:.2f} ms (host) against {1e3 * ra:.2f} ms (resident), "
                 f"row call + around {1e3 * (hr + ha):.2f} ms against {1e3 * (rr + ra):.2f} ms")
    for name in ("host", "resident"):
        lines.append(f"  host memory, {name:8s} route: {mem[name].held / 2**20:9.1f} MiB held after T = {T}, "
                     f"{mem[name].peak / 2**20:9.1f} MiB at the highest point of an append")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resident_append_time.txt"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[10, 12])
    ap.add_argument("--states", type=int, default=20)
    args = ap.parse_args()
    lines = [f"# tools/micro/resident_append_time.py on {torch.cuda.get_device_name(0)}: host clock around work that ends "
             f"in a device synchronise, one measurement per T (no repeats: every append changes the training set); "
             f"tracemalloc on during the timed passes, for both routes alike"]
    tracemalloc.start()
    for norb in args.sizes:
        solver = TimedFCI(eigensolver="davidson")
        run(norb, 2, solver, [], warm=True)
        solver.forget()
        run(norb, args.states, solver, lines)
        del solver
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
