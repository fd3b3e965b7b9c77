"""Device time of the S^2 calls of csrc/fci_spin.hip beside the sigma vector they accompany, and what the spin penalty
costs a Davidson run.

Part 1, at (10,(5,5)), (12,(6,6)) and (14,(7,7)): ``evc_fci_spin_apply`` with beta = 0 and beta = 1 and
``evc_fci_spin_diag``, HIP events around the C call, median of 20 after 3 warm-up calls; beside each ``evc_fci_sigma`` of
the same shape in the same process, and the memory floor of the call at 8 TB/s (c read, out written and for beta = 1
read, both tables read; for the diagonal hdiag read and written and the tables).

Part 2: the Davidson runs of tools/micro/fci_solve_time.py for H12, two roots, both orbital bases, with penalty 0 and
0.2: wall time of the second of two ``kernel`` calls and the number of sigma vectors.

usage: python tools/micro/fci_spin_time.py [--out profiles/fci_spin_time.txt] [--sizes 10 12 14] [--solve 12]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from evcont_amd import _lib                                                  # noqa: E402
from evcont_amd._lib import check                                            # noqa: E402
from evcont_amd.electron_integral_utils import get_basis, get_integrals      # noqa: E402
from evcont_amd.fci_device import DeviceFCI                                  # noqa: E402
from evcont_amd.fci_tables import npad_of, packed_table                      # noqa: E402
from evcont_amd.hchain import hydrogen_chain                                 # noqa: E402

HBM = 8.0e12     # bytes per second


def median_ms(call, reps=20, warm=3):
    for _ in range(warm):
        call()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        call()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return float(np.median(times))


def kernels(norb, lines):
    lib = _lib.load()
    dev = torch.device("cuda:0")
    nelec = (norb // 2, norb // 2)
    ta = packed_table(norb, nelec[0])
    na = nb = ta.shape[0]
    dim = na * nb
    dta = torch.from_numpy(ta).to(dev)
    rng = np.random.default_rng(norb)
    c = torch.from_numpy(rng.standard_normal(dim)).to(dev)
    out = torch.zeros(dim, dtype=torch.float64, device=dev)
    h1 = torch.from_numpy(rng.standard_normal((norb, norb))).to(dev)
    h2 = torch.from_numpy(rng.standard_normal(norb ** 4)).to(dev)
    wsb = lib.evc_fci_workspace_bytes(norb, na, nb, 0)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    tp, cp, op = dta.data_ptr(), c.data_ptr(), out.data_ptr()

    def sigma():
        check(lib.evc_fci_sigma(norb, na, nb, tp, tp, h1.data_ptr(), h2.data_ptr(), cp, op, ws.data_ptr(), wsb, st),
              "evc_fci_sigma")

    def apply(beta):
        check(lib.evc_fci_spin_apply(norb, na, nb, tp, tp, cp, 0.2, 0.0, beta, op, st), "evc_fci_spin_apply")

    def diag():
        check(lib.evc_fci_spin_diag(norb, na, nb, tp, tp, 0.2, 0.0, op, st), "evc_fci_spin_diag")

    t_sigma = median_ms(sigma)
    tables = 2 * na * npad_of(norb) * 4
    lines.append(f"\n({norb},{nelec}), {dim} determinants: evc_fci_sigma {t_sigma:.4f} ms")
    for name, call, nbytes in (("evc_fci_spin_apply beta=0", lambda: apply(0.0), 16 * dim + tables),
                               ("evc_fci_spin_apply beta=1", lambda: apply(1.0), 24 * dim + tables),
                               ("evc_fci_spin_diag", diag, 16 * dim + tables)):
        t = median_ms(call)
        rec = lib.evc_profile_kernel(_lib.FCI_PROF_SOLVE).decode()
        floor = 1e3 * nbytes / HBM
        lines.append(f"  {name:26s} {t:8.4f} ms  {100 * t / t_sigma:6.2f} % of sigma  floor {floor:.4f} ms "
                     f"({t / floor:5.1f} x)  [{rec}]")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def solves(norb, lines):
    nelec = (norb // 2, norb // 2)
    for cibasis in ("OAO", "canonical"):
        mol = hydrogen_chain(norb, 1.8, need_grad=False)
        h1, h2 = get_integrals(mol, get_basis(mol, cibasis))
        for penalty in (0.0, 0.2):
            dav = DeviceFCI(eigensolver="davidson", spin_penalty=penalty)
            dav.kernel(h1, h2, norb, nelec, nroots=2)
            t, (e, v) = wall(lambda: dav.kernel(h1, h2, norb, nelec, nroots=2))
            ss = dav.spin_squares if penalty else [dav.spin_square(x, norb, nelec)[0] for x in v]
            inf = dav.davidson_info
            lines.append(f"  H{norb} {nelec} {cibasis:9s} 2 roots, penalty {penalty}: {1e3 * t:8.1f} ms wall, {inf['nsigma']:4d} "
                         f"sigma vectors, {inf['iterations']} iterations, converged={dav.converged}, E = "
                         + ", ".join(f"{x:.8f}" for x in e) + ", <S^2> = " + ", ".join(f"{round(x, 6) + 0.0:.6f}" for x in ss))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fci_spin_time.txt"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[10, 12, 14])
    ap.add_argument("--solve", type=int, nargs="*", default=[12])
    args = ap.parse_args()
    lines = [f"# tools/micro/fci_spin_time.py on {torch.cuda.get_device_name(0)}: HIP events around the C call, median of "
             f"20 after 3; floor = bytes the call must move at 8 TB/s"]
    for norb in args.sizes:
        kernels(norb, lines)
    if args.solve:
        lines.append("\nDavidson (DeviceFCI(eigensolver='davidson')), wall time of the second of two kernel calls:")
    for norb in args.solve:
        solves(norb, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
