"""What one appended CAS training state costs at H30 CAS(10,10) (ncore = 10, N = 30) with T = 1, 5, 20 stored states: the
t-RDM row of the new state against all T, on the device route (``DeviceFCI.cas_trans_rdm12_rows``) and by the host
statement (``cas_small.trans_rdm12_rows`` with ``fci_small``) on the same machine, with the same states.

The device route is split by a subclass that wraps its stages (host clock, the device synchronised at both ends of each):
host intermediates (``cas_small.pair_intermediates``, one per stored geometry), rotate (one ``evc_fci_rotate_block`` per
stored geometry; T ``evc_fci_rotate`` calls when ``profiles/cas_append_time.txt`` was written), row call (one
``evc_fci_trdm_rows_block`` with one bra, the single call's routine), expand (one ``evc_cas_expand_rows``, dense layout), and the rest (uploads, the dense (T, N^4) rows
to the host).  The states are solved once (RHF + CASCI at T geometries of the chain, spacing 1.8 + 0.01 k), outside the
timed region; the first call of each route at each T is a warm-up, the second is timed.  A record, not a pass/fail ratio.

usage: python tools/micro/cas_time.py [--out profiles/cas_append_time.txt] [--atoms 30] [--ncas 10] [--states 1 5 20]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from evcont_amd import _lib, cas_small                                        # noqa: E402
from evcont_amd.fci_device import DeviceFCI                                   # noqa: E402
from evcont_amd.hchain import hydrogen_chain                                  # noqa: E402


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


class Stages:
    def __init__(self):
        self.s = {"intermediates": 0.0, "rotate": 0.0, "row call": 0.0, "expand": 0.0}

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
        self.evc_fci_trdm_rows = stages.timed("row call", lib.evc_fci_trdm_rows)
        self.evc_fci_trdm_rows_block = stages.timed("row call", lib.evc_fci_trdm_rows_block)
        self.evc_cas_expand_rows = stages.timed("expand", lib.evc_cas_expand_rows)

    def __getattr__(self, name):
        return getattr(self._lib, name)


class TimedFCI(DeviceFCI):
    stages = None

    def _rotate(self, *a):
        return self.stages.timed("rotate", super()._rotate)(*a)

    def _rotate_block(self, *a):
        return self.stages.timed("rotate", super()._rotate_block)(*a)

    def _setup(self, norb, nelec):
        out = super()._setup(norb, nelec)
        return (_TimedLib(out[0], self.stages),) + tuple(out[1:])


def device_row(solver, bra, kets):
    st = solver.stages = Stages()
    real = cas_small.pair_intermediates
    cas_small.pair_intermediates = st.timed("intermediates", real)
    try:
        t0 = clock()
        out = solver.cas_trans_rdm12_rows(bra, kets)
        total = clock() - t0
    finally:
        cas_small.pair_intermediates = real
    return out, total, dict(st.s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cas_append_time.txt"))
    ap.add_argument("--atoms", type=int, default=30)
    ap.add_argument("--ncas", type=int, default=10)
    ap.add_argument("--states", type=int, nargs="*", default=[1, 5, 20])
    ap.add_argument("--host-states", type=int, default=20, help="largest T at which the host statement is timed too")
    args = ap.parse_args()
    n, ncas = args.atoms, args.ncas
    solver = TimedFCI(eigensolver="davidson")
    solver.stages = Stages()
    states, t_solve = [], []
    for k in range(max(args.states)):
        t0 = clock()
        states.append(cas_small.casci(hydrogen_chain(n, 1.8 + 0.01 * k, need_grad=False), ncas, ncas, solver))
        t_solve.append(clock() - t0)
    prop = torch.cuda.get_device_properties(0)
    lines = [f"# tools/micro/cas_time.py on {prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} "
             f"CUs, {prop.total_memory >> 30} GiB; torch {torch.__version__}): H{n} CAS({ncas},{ncas}), ncore = "
             f"{states[0].ncore}, {states[0].ci.size} active determinants; host clock around work that ends in a device "
             f"synchronise; one timed call per T after one warm-up call",
             f"# RHF + CASCI per state (outside the rows): {1e3 * np.mean(t_solve):.1f} ms mean, first {1e3 * t_solve[0]:.1f} ms",
             "#   T | device: total  intermediates  rotate  row call  expand    rest | host statement | max |d| device - host",
             "# (ms wall per appended state: its row against all T stored states, itself included)"]
    for T in args.states:
        bra, kets = states[T - 1], states[:T]
        device_row(solver, bra, kets)
        (ov, d1, d2), total, s = device_row(solver, bra, kets)
        rest = total - sum(s.values())
        if T <= args.host_states:
            t0 = time.perf_counter()
            want = cas_small.trans_rdm12_rows(bra, kets)
            t_host = time.perf_counter() - t0
            diff = max(float(np.abs(g - w).max()) for g, w in zip((ov, d1, d2), want))
            host = f"{1e3 * t_host:14.1f} | {diff:.1e}"
        else:
            host = f"{'-':>14s} | -"
        lines.append(f"  {T:3d} | {1e3 * total:13.2f} {1e3 * s['intermediates']:14.2f} {1e3 * s['rotate']:7.2f} "
                     f"{1e3 * s['row call']:9.2f} {1e3 * s['expand']:7.2f} {1e3 * rest:7.2f} | {host}")
    buf = C.create_string_buffer(2048)
    _lib.load().evc_cas_expand_describe(n, ncas, _lib.LAYOUT_FULL6, buf, len(buf))
    lines.append("# launches of the expand call (evc_cas_expand_describe; the steps and the core kernel once per ket):")
    lines += ["#   " + ln for ln in buf.value.decode().splitlines()]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
