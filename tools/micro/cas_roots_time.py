"""What appending one geometry with R CASCI roots costs at H30 CAS(10,10) (ncore = 10, N = 30), R = 3, with G = 1 and 5
stored geometries (R G stored states, the new geometry's own roots included among the kets): the block call
(``DeviceFCI.cas_trans_rdm12_block``: intermediates once per stored geometry, one ``evc_fci_rotate_block`` per geometry)
against the loop of R ``DeviceFCI.cas_trans_rdm12_rows`` calls, which is what the parent of this change offers and runs
unchanged there (the baseline).  (Since DESIGN.md 8.1.7 ``cas_trans_rdm12_rows`` is the one-bra case of the block call and
both routes make their row calls through ``evc_fci_trdm_rows_block``: the loop then forms its intermediates once per
stored geometry and bra, and ``profiles/cas_roots_time.txt`` records the routes as they were when it was written;
``tools/micro/cas_resident_time.py`` is the current record.)

Both routes are split by wrapping their stages (host clock, the device synchronised at both ends of each): host
intermediates (``cas_small.pair_intermediates``), rotate (``_rotate`` / ``_rotate_block``), row calls
(``evc_fci_trdm_rows``), expand (``evc_cas_expand_rows``, dense layout) and the rest (uploads, the dense rows to the
host).  The rotate launches are counted from the shape: per rotation call one minor launch and one product launch per
panel of T_b, and the same for T_a unless both spins share a resident T.  The states are solved once, outside the timed
region; the first call of each route is a warm-up, then the median of ``--repeats`` timed calls is written, column by
column.  A record, not a pass/fail ratio.

usage: python tools/micro/cas_roots_time.py [--out profiles/cas_roots_time.txt] [--atoms 30] [--ncas 10] [--roots 3]
       [--geometries 1 5] [--repeats 5]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from evcont_amd import cas_small                                              # noqa: E402
from evcont_amd.fci_device import DeviceFCI                                   # noqa: E402
from evcont_amd.hchain import hydrogen_chain                                  # noqa: E402

STAGES = ("intermediates", "rotate", "row calls", "expand")


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


class Stages:
    def __init__(self):
        self.s = dict.fromkeys(STAGES, 0.0)
        self.rotations = []          # vectors of every rotation call

    def timed(self, name, fn):
        def wrapped(*a, **k):
            t0 = clock()
            out = fn(*a, **k)
            self.s[name] += clock() - t0
            return out
        return wrapped


class _TimedLib:
    """The loaded library with two of its entry points timed."""

    def __init__(self, lib, stages):
        self._lib = lib
        self.evc_fci_trdm_rows = stages.timed("row calls", lib.evc_fci_trdm_rows)
        self.evc_fci_trdm_rows_block = stages.timed("row calls", lib.evc_fci_trdm_rows_block)
        self.evc_cas_expand_rows = stages.timed("expand", lib.evc_cas_expand_rows)

    def __getattr__(self, name):
        return getattr(self._lib, name)


class TimedFCI(DeviceFCI):
    stages = None

    def _rotate(self, *a):
        self.stages.rotations.append(1)
        return self.stages.timed("rotate", super()._rotate)(*a)

    def _rotate_block(self, cis, *a):
        cis = list(cis)
        self.stages.rotations.append(len(cis))
        return self.stages.timed("rotate", super()._rotate_block)(cis, *a)

    def _setup(self, norb, nelec):
        out = super()._setup(norb, nelec)
        return (_TimedLib(out[0], self.stages),) + tuple(out[1:])


def timed_route(solver, route):
    st = solver.stages = Stages()
    real = cas_small.pair_intermediates
    cas_small.pair_intermediates = st.timed("intermediates", real)
    try:
        t0 = clock()
        out = route()
        total = clock() - t0
    finally:
        cas_small.pair_intermediates = real
    return out, total, st


def rotate_launches(st, ns, shared_resident=True):
    """Launches of the rotation calls of one route: per call, per panel of T_b one minor launch and one product launch
    per 16 vectors; T_a the same, without its minor launches where both spins share one resident T."""
    width = min(ns, max(64, (1 << 19) // ns // 64 * 64))
    panels = -(-ns // width)
    total = 0
    for nvec in st.rotations:
        products = -(-nvec // 16)
        total += panels * (1 + products) + panels * ((0 if shared_resident else 1) + products)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cas_roots_time.txt"))
    ap.add_argument("--atoms", type=int, default=30)
    ap.add_argument("--ncas", type=int, default=10)
    ap.add_argument("--roots", type=int, default=3)
    ap.add_argument("--geometries", type=int, nargs="*", default=[1, 5])
    ap.add_argument("--repeats", type=int, default=5, help="timed calls per route; the median of each column is written")
    args = ap.parse_args()
    n, ncas, R = args.atoms, args.ncas, args.roots
    solver = TimedFCI(eigensolver="davidson")
    solver.stages = Stages()
    geoms, t_solve = [], []
    for k in range(max(args.geometries)):
        t0 = clock()
        geoms.append(cas_small.casci_roots(hydrogen_chain(n, 1.8 + 0.01 * k, need_grad=False), ncas, ncas, solver, R))
        t_solve.append(clock() - t0)
    ns = geoms[0][0].ci.shape[0]
    prop = torch.cuda.get_device_properties(0)
    lines = [f"# tools/micro/cas_roots_time.py on {prop.name} ({getattr(prop, 'gcnArchName', '?')}, "
             f"{prop.multi_processor_count} CUs, {prop.total_memory >> 30} GiB; torch {torch.__version__}): H{n} "
             f"CAS({ncas},{ncas}), ncore = {geoms[0][0].ncore}, {geoms[0][0].ci.size} active determinants, R = {R} roots per "
             "geometry; host clock around work that ends in a device synchronise; per route one warm-up call, then "
             f"the median of {args.repeats} timed calls, column by column",
             f"# RHF + CASCI of {R} roots per geometry (outside the rows): {1e3 * np.mean(t_solve):.1f} ms mean, first "
             f"{1e3 * t_solve[0]:.1f} ms",
             "# ms wall per appended geometry: the rows of its R roots against all R G stored states, its own included",
             "#   G  route | total  intermediates  rotate  row calls  expand    rest | intermediates formed  rotation calls  "
             "rotate launches | rows equal bit for bit"]
    for G in args.geometries:
        kets = [s for g in geoms[:G] for s in g]
        bras = list(geoms[G - 1])
        loop = lambda: [solver.cas_trans_rdm12_rows(b, kets) for b in bras]
        block = lambda: solver.cas_trans_rdm12_block(bras, kets)
        results = {}
        for name, route in (("loop", loop), ("block", block)):
            timed_route(solver, route)
            runs = [timed_route(solver, route) for _ in range(args.repeats)]
            out, _, st = runs[0]
            results[name] = out
            total = float(np.median([t for _, t, _ in runs]))
            st.s = {k: float(np.median([x.s[k] for _, _, x in runs])) for k in STAGES}
            rest = float(np.median([t - sum(x.s.values()) for _, t, x in runs]))
            formed = {"loop": R * R * G, "block": G}[name]
            lines.append(f"  {G:3d}  {name:5s} | {1e3 * total:6.2f} {1e3 * st.s['intermediates']:13.2f} "
                         f"{1e3 * st.s['rotate']:7.2f} {1e3 * st.s['row calls']:10.2f} {1e3 * st.s['expand']:7.2f} "
                         f"{1e3 * rest:7.2f} | {formed:19d} {len(st.rotations):15d} {rotate_launches(st, ns):16d} | "
                         + ("" if name == "loop" else str(all(
                             np.array_equal(results["block"][i][r], results["loop"][r][i])
                             for r in range(R) for i in range(3)))))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
