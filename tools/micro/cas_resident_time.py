"""What appending one geometry costs at H30 CAS(10,10) (ncore = 10, N = 30) on the two CAS containers, in one run:

* host      ``CAS_EVCont_obj``'s append without its solve: ``DeviceFCI.cas_trans_rdm12_block(bras, kets)`` as it is
            now (dense rows to the host; the rectangular block, R (T + R) rows; its row calls already go through
            ``evc_fci_trdm_rows_block``, so this column is somewhat below what the loop of single calls gave) and ``containers.grow_trdms`` per root (new
            ``(T+1, T+1, N^4)`` arrays on the host), the two parts also given apart;
* resident  ``ResidentCAS_EVCont_obj``'s append without its solve: the CI vectors of the stored states already on the
            device, one triangular block call that writes the sym8 rows in place (``ResidentTRDMs.append_block``);
* row call  the active-space product alone, on the rotated kets of the resident route: once as R single
            ``evc_fci_trdm_rows`` calls (bra r against its T + r + 1 kets: what the loop of single calls launches),
            once as one ``evc_fci_trdm_rows_block`` call on the same ragged counts; the two must agree bit for bit.

R = 3 roots at G = 1 and 5 stored geometries (the new one included), and a single root at T = 20.  Host clock around work
that ends in a device synchronise; per route one warm-up, then the median of ``--repeats`` timed calls and their
min-max.  The states are solved once, outside the timed region; that solve is split into integrals, RHF, active-space
transform and solver: the integrals are the construction of the molecule (``hydrogen_chain``, numpy), the rest is
split by wrapping the calls of ``cas_small._casci_states``.  A record, not a pass/fail ratio.

usage: python tools/micro/cas_resident_time.py [--out profiles/cas_resident_time.txt] [--atoms 30] [--ncas 10]
       [--roots 3] [--geometries 1 5] [--single 20] [--repeats 5]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from evcont_amd import cas_small, integrals, scf_small                        # noqa: E402
from evcont_amd.containers import grow_trdms                                  # noqa: E402
from evcont_amd.fci_device import DeviceFCI                                   # noqa: E402
from evcont_amd.hchain import hydrogen_chain                                  # noqa: E402
from evcont_amd.resident import ResidentTRDMs                                 # noqa: E402

SOLVE_PARTS = ("integrals", "RHF", "solver")


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def med(xs):
    xs = [1e3 * x for x in xs]
    return f"{np.median(xs):8.2f} ({min(xs):.2f}-{max(xs):.2f})"


def timed(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        t0 = clock()
        fn()
        out.append(clock() - t0)
    return out


def solve_split(solver, make_mol, ncas, nroots, parts):
    """One molecule and one ``casci_roots`` on it with the four parts timed into ``parts`` (lists of seconds); returns
    the states."""
    spent = dict.fromkeys(SOLVE_PARTS, 0.0)
    t0 = clock()
    mol = make_mol()
    t_mol = clock() - t0

    def wrap(name, fn):
        def inner(*a, **k):
            t0 = clock()
            out = fn(*a, **k)
            spent[name] += clock() - t0
            return out
        return inner

    real = integrals.ao_arrays, scf_small.rhf, solver.kernel
    integrals.ao_arrays, scf_small.rhf = wrap("integrals", real[0]), wrap("RHF", real[1])
    solver.kernel = wrap("solver", real[2])
    try:
        t0 = clock()
        states = cas_small.casci_roots(mol, ncas, ncas, solver, nroots)
        total = clock() - t0 + t_mol
    finally:
        integrals.ao_arrays, scf_small.rhf = real[0], real[1]
        del solver.kernel
    spent["integrals"] += t_mol
    for k in SOLVE_PARTS:
        parts.setdefault(k, []).append(spent[k])
    parts.setdefault("transform", []).append(total - sum(spent.values()))   # core potential, h2 to the active space, U
    parts.setdefault("total", []).append(total)
    return states


def on_device(states, dev):
    return [cas_small.CASState(U=s.U, ncore=s.ncore, ncas=s.ncas, nelecas=s.nelecas,
                               ci=torch.from_numpy(np.ascontiguousarray(s.ci)).to(dev), e_tot=s.e_tot) for s in states]


def host_append(solver, stored, bras):
    """The host container's append of one geometry (``CAS_EVCont_obj._append_own`` / ``_append_own_roots``) without the
    solve, on arrays that already hold the stored states' blocks (zeros here: their values do not matter)."""
    T, R = len(stored), len(bras)
    n = bras[0].U.shape[0]
    ovlp = np.zeros((T, T)) if T else None
    one = np.zeros((T, T, n, n)) if T else None
    two = np.zeros((T, T, n, n, n, n)) if T else None

    def run():
        o, a, b = ovlp, one, two
        t0 = clock()
        if R == 1:
            ov, d1, d2 = (x[None] for x in solver.cas_trans_rdm12_rows(bras[0], stored + bras))
        else:
            ov, d1, d2 = solver.cas_trans_rdm12_block(bras, stored + bras)
        run.call.append(clock() - t0)
        for r in range(R):
            o, a, b = grow_trdms(o, a, b, ov[r, :T + r + 1], d1[r, :T + r + 1], d2[r, :T + r + 1])
        return o, a, b
    run.call = []                # seconds of the row call alone, one entry per run (the warm-up included)
    return run


def resident_append(solver, dstored, dbras, n):
    """The resident container's append without the solve: a matrix that holds T states, one triangular block call."""
    T = len(dstored)
    res = ResidentTRDMs(n, "sym8", capacity=max(16, T + len(dbras)))

    def run():
        res.T = T                    # (the rows of the stored states are zeros: their values do not matter)
        return res.append_block(solver, dbras, dstored + dbras)
    return run


def row_calls(solver, dstored, dbras, repeats):
    """R single row calls and one block call on the same rotated kets and ragged counts; (single, block, equal)."""
    bra0 = dbras[0]
    ncas, nelec = int(bra0.ncas), tuple(int(x) for x in bra0.nelecas)
    kets = dstored + dbras
    T, R = len(dstored), len(dbras)
    counts = [T + r + 1 for r in range(R)]
    total = sum(counts)
    dkets = []
    for first, count in cas_small.ket_groups(kets):
        fac, s_eff, _, _, _ = cas_small.pair_intermediates(bra0, kets[first])
        rot, _, _ = solver._rotate_block([k.ci for k in kets[first:first + count]], nelec, np.ascontiguousarray(s_eff.T))
        dkets.extend(t.mul_(fac) for t in rot)
    lib, dta, dtb, na, nb, grant = solver._setup(ncas, nelec)
    dev = dta.device
    full = lib.evc_fci_rows_block_workspace_bytes(ncas, na, nb, R, 0)
    ws = torch.empty(full, dtype=torch.uint8, device=dev)
    n2 = ncas * ncas
    outs = [[torch.empty(total * w, dtype=torch.float64, device=dev) for w in (1, n2, n2 * n2)] for _ in range(2)]
    kp = (C.c_void_p * len(dkets))(*[t.data_ptr() for t in dkets])
    bp = (C.c_void_p * R)(*[b.ci.data_ptr() for b in dbras])
    cnt = (C.c_int * R)(*counts)
    st = torch.cuda.current_stream(dev).cuda_stream

    def single():
        ov, d1, d2 = outs[0]
        off = 0
        for r in range(R):
            rc = lib.evc_fci_trdm_rows(ncas, na, nb, dta.data_ptr(), dtb.data_ptr(), dbras[r].ci.data_ptr(), kp, counts[r],
                                       ov.data_ptr() + 8 * off, d1.data_ptr() + 8 * off * n2,
                                       d2.data_ptr() + 8 * off * n2 * n2, ws.data_ptr(), grant, st)
            assert rc == 0, lib.evc_last_error()
            off += counts[r]

    def block():
        ov, d1, d2 = outs[1]
        rc = lib.evc_fci_trdm_rows_block(ncas, na, nb, dta.data_ptr(), dtb.data_ptr(), bp, R, kp, cnt, ov.data_ptr(),
                                         d1.data_ptr(), d2.data_ptr(), ws.data_ptr(), full, st)
        assert rc == 0, lib.evc_last_error()

    ts, tb = timed(single, repeats), timed(block, repeats)
    torch.cuda.synchronize()
    equal = all(torch.equal(a, b) for a, b in zip(*outs))
    return ts, tb, equal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cas_resident_time.txt"))
    ap.add_argument("--atoms", type=int, default=30)
    ap.add_argument("--ncas", type=int, default=10)
    ap.add_argument("--roots", type=int, default=3)
    ap.add_argument("--geometries", type=int, nargs="*", default=[1, 5])
    ap.add_argument("--single", type=int, default=20, help="stored states of the single-root case (0: skip it)")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    n, ncas, R = args.atoms, args.ncas, args.roots
    solver = DeviceFCI(eigensolver="davidson")
    dev = solver._dev()
    parts, geoms = {}, []
    for k in range(max(args.geometries)):
        geoms.append(solve_split(solver, lambda: hydrogen_chain(n, 1.8 + 0.01 * k, need_grad=False), ncas, R, parts))
    parts1, singles = {}, []
    for k in range(args.single + 1 if args.single else 0):
        singles.append(solve_split(solver, lambda: hydrogen_chain(n, 1.7 + 0.01 * k, need_grad=False), ncas, 1,
                                   parts1)[0])
    prop = torch.cuda.get_device_properties(0)
    lines = [f"# tools/micro/cas_resident_time.py on {prop.name} ({getattr(prop, 'gcnArchName', '?')}, "
             f"{prop.multi_processor_count} CUs, {prop.total_memory >> 30} GiB; torch {torch.__version__}): H{n} "
             f"CAS({ncas},{ncas}), ncore = {geoms[0][0].ncore}, {geoms[0][0].ci.size} active determinants; host clock around "
             f"work that ends in a device synchronise; per route one warm-up call, then the median of {args.repeats} timed "
             "calls (min-max in brackets)",
             "# ms wall per appended geometry, without its RHF + CASCI: host = today's dense block call (row calls through evc_fci_trdm_rows_block) + grow_trdms, resident = "
             "triangular block call into the sym8 matrix, row call = the active-space product alone",
             "#   R   T | host container          of it: block call       resident container      | R single row calls     "
             "one block call         | rows equal bit for bit"]
    cases = [(R, [s for g in geoms[:G - 1] for s in g], list(geoms[G - 1])) for G in args.geometries]
    if singles:
        cases.append((1, singles[:-1], [singles[-1]]))
    for r, stored, bras in cases:
        dall = on_device(stored + bras, dev)
        dstored, dbras = dall[:len(stored)], dall[len(stored):]
        host = host_append(solver, stored, bras)
        th = timed(host, args.repeats)
        tr = timed(resident_append(solver, dstored, dbras, n), args.repeats)
        ts, tb, equal = row_calls(solver, dstored, dbras, args.repeats)
        lines.append(f"  {r:3d} {len(stored):3d} | {med(th)}  {med(host.call[1:])}  {med(tr)} | {med(ts)}  {med(tb)} | "
                     f"{equal}")
    for label, p, nr in (("R = %d roots" % R, parts, R), ("one root", parts1, 1)):
        if p:
            m = {k: 1e3 * float(np.median(v)) for k, v in p.items()}
            lines.append(f"# RHF + CASCI per geometry, {label} (median of {len(p['total'])} geometries, ms): total "
                         f"{m['total']:.1f} = integrals {m['integrals']:.1f} + RHF {m['RHF']:.1f} + active-space transform "
                         f"{m['transform']:.1f} + solver {m['solver']:.1f}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
