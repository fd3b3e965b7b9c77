"""``tests/spgto_harness.py`` bound to the route of csrc/spdfgto.hip -- a helper, no test: ``Basis`` with the shells and the
normalisation of ``gto_spdf`` (l <= 3), whose ``run`` / ``run_dipole`` call ``evc_spdfgto_integrals_batch`` /
``evc_spdfgto_dipole_batch``, and ``run_dipole_grad`` for ``evc_spdfgto_dipole_grad_batch``.  The molecules are in
tests/spdfgto_cases.py."""
import ctypes as C

import torch

import spgto_harness
from evcont_amd import _lib
from spgto_harness import (DEV, ENERGY, ENERGY_FIELDS, FENCE, GRAD_FIELDS, GUARD, S2KL, S4, Fenced, pack_eri,  # noqa: F401
                           pack_ip1, run, run_dipole, shapes)


class Basis(spgto_harness.Basis):
    route = "spdfgto"


def run_dipole_grad(R, basis, origin):
    """One call of ``evc_spdfgto_dipole_grad_batch`` on a fresh poisoned buffer -> (rc, host (G,3,3,N,N), fences intact)."""
    lib = _lib.load()
    G, dR = spgto_harness._coords(R, basis.natm)
    n = basis.nao
    buf = Fenced(G * 9 * n * n)
    o = (C.c_double * 3)(*[float(x) for x in origin])
    rc = lib.evc_spdfgto_dipole_grad_batch(basis.natm, basis.nshell, G, dR.data_ptr(), *basis.pointers(),
                                           C.cast(o, C.c_void_p), buf.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, buf.payload((G, 3, 3, n, n)), buf.fences_intact()
