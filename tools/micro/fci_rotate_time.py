"""Device time of the CI-vector rotation evc_fci_rotate (csrc/fci_rotate.hip) at H10 (5,5), H12 (6,6) and (14, (7,7)),
next to one sigma vector of the same shape (evc_fci_sigma, as tools/micro/fci_time.py times it): HIP events around the C
call alone, vectors, string masks and tables resident, median of 20 calls after 3 warm-up calls.  u = C^T S C_OAO of the
hydrogen chain at 1.8 Bohr, C from scf_small.rhf: the rotation FCI_EVCont_obj(cibasis="canonical") asks for.  Each shape
is timed with the resident workspace and with the least one (T formed and consumed in panels).

What the figure is for: a state solved in the canonical basis costs one rotation and saves the sigma vectors of
profiles/fci_solve_time.txt; the last column is the rotation in units of one sigma vector.

usage: python tools/micro/fci_rotate_time.py [--out profiles/fci_rotate_time.txt] [--sizes 10 12 14]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from evcont_amd import _lib                                                  # noqa: E402
from evcont_amd.electron_integral_utils import get_basis                     # noqa: E402
from evcont_amd.fci_device import DeviceFCI                                  # noqa: E402
from evcont_amd.hchain import hydrogen_chain                                 # noqa: E402

WARM, REPS = 3, 20


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fci_rotate_time.txt"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[10, 12, 14])
    args = ap.parse_args()
    lib = _lib.load()
    lines = [f"# tools/micro/fci_rotate_time.py on {torch.cuda.get_device_name(0)}: median [min, max] ms of {REPS} calls "
             f"after {WARM}, HIP events around the C call"]
    for norb in args.sizes:
        nelec = (norb // 2, norb // 2)
        mol = hydrogen_chain(norb, 1.8, need_grad=False)
        u = np.ascontiguousarray(np.einsum("ji,jk,kl->il", get_basis(mol, "canonical"), mol.S, get_basis(mol)))
        dev = DeviceFCI()
        _, dta, dtb, na, nb, grant = dev._setup(norb, nelec)
        dsa, dsb = dev._masks[(norb, nelec)]
        d = dev._device
        rng = np.random.default_rng(norb)
        c = rng.standard_normal((na, nb))
        dc = torch.from_numpy(c / np.linalg.norm(c)).to(d)
        out = torch.empty(na * nb, dtype=torch.float64, device=d)
        n2 = norb * norb
        h1 = rng.standard_normal((norb, norb))
        h2 = rng.standard_normal((n2, n2))
        dh1 = torch.from_numpy(0.5 * (h1 + h1.T)).to(d)
        dh2 = torch.from_numpy((0.5 * (h2 + h2.T)).reshape(-1).copy()).to(d)
        st = dev._stream()
        sigma = lambda: _lib.check(lib.evc_fci_sigma(
            norb, na, nb, dta.data_ptr(), dtb.data_ptr(), dh1.data_ptr(), dh2.data_ptr(), dc.data_ptr(), out.data_ptr(),
            dev._ws.data_ptr(), grant, st), "evc_fci_sigma")
        s_ms, s_lo, s_hi = timed(sigma)
        lines.append(f"\n({norb}, {nelec}): {na} x {nb} strings, {na * nb} determinants")
        lines.append(f"  sigma vector        {s_ms:9.3f} ms [{s_lo:.3f}, {s_hi:.3f}]   {lib.evc_profile_kernel(10).decode()}")
        full = lib.evc_fci_rotate_workspace_bytes(norb, nelec[0], nelec[1], na, nb, 0)
        least = lib.evc_fci_rotate_workspace_bytes(norb, nelec[0], nelec[1], na, nb, 1)
        flops = 2.0 * na * nb * (na + nb)
        for name, nbytes in (("resident", full), ("least", least)):
            ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
            rotate = lambda: _lib.check(lib.evc_fci_rotate(
                norb, nelec[0], nelec[1], na, nb, dsa.data_ptr(), dsb.data_ptr(), u.ctypes.data, u.ctypes.data,
                dc.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, st), "evc_fci_rotate")
            r_ms, r_lo, r_hi = timed(rotate)
            lines.append(f"  rotation, {name:8s}  {r_ms:9.3f} ms [{r_lo:.3f}, {r_hi:.3f}]   workspace {nbytes / 2 ** 20:8.1f} MiB, "
                         f"{flops / r_ms / 1e9:6.2f} TFLOP/s over the two products, = {r_ms / s_ms:6.2f} sigma vectors   "
                         f"{lib.evc_profile_kernel(12).decode()}")
            del ws
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
