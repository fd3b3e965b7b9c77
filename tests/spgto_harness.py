"""How the GPU tests of csrc/spgto.hip and csrc/spdgto.hip call ``evc_<route>_integrals_batch`` and
``evc_<route>_dipole_batch`` -- a helper, no test, the shell-route counterpart of tests/sgto_harness.py: through ctypes,
with the flattened basis and arbitrary flags, on NaN-poisoned output buffers and workspace between two guards each
(``Fenced``).  The route is the basis's: ``Basis`` is s + p, ``spdgto_harness.Basis`` s + p + d."""
import ctypes as C

import numpy as np
import torch

from evcont_amd import _lib
from evcont_amd.gto_host import contraction_coefficients, flatten_shells
from sgto_harness import DEV, FENCE, GUARD, Fenced                      # noqa: F401 (FENCE, GUARD: for the tests)

S4, S2KL, ENERGY = _lib.FLAG_ERI_S4, _lib.FLAG_IP1_S2KL, _lib.FLAG_ENERGY_ONLY
ENERGY_FIELDS = ("enuc", "S", "hcore", "eri")
GRAD_FIELDS = ("ipovlp", "dhcore", "eri_ip1", "gnuc")


class Basis:
    """The flattened basis of a molecule as the C calls take it: ``charges`` (A,), ``shells`` per atom a list of
    ``Shell`` (an empty list: a nucleus without functions).  The coefficients go through
    ``gto_host.contraction_coefficients``, so the device and the host statement see the same numbers."""
    route = "spgto"                                                          # a subclass names another route

    def __init__(self, charges, shells, renormalize=True):
        self.charges = np.ascontiguousarray(charges, dtype=np.float64).reshape(-1)
        assert len(shells) == self.charges.shape[0]
        (self.shell_atom, self.shell_l, self.shell_prim_offset, self.exponents, self.coefficients, self.aoslices,
         self.nao) = flatten_shells(shells, contraction_coefficients(shells, renormalize))
        self.natm, self.nshell, self.nprim = len(shells), len(self.shell_l), int(self.shell_prim_offset[-1])
        self.shells = shells

    def pointers(self):
        return tuple(a.ctypes.data for a in (self.shell_atom, self.shell_l, self.shell_prim_offset, self.exponents,
                                             self.coefficients))


def shapes(A, n, G, flags):
    ms = n * (n + 1) // 2
    return {"enuc": (G,), "S": (G, n, n), "hcore": (G, n, n), "eri": (G, ms, ms) if flags & S4 else (G, n, n, n, n),
            "ipovlp": (G, 3, n, n), "dhcore": (G, A, 3, n, n), "gnuc": (G, A, 3),
            "eri_ip1": (G, 3, n, n, ms) if flags & S2KL else (G, 3, n, n, n, n)}


def _coords(R, natm):
    R = np.ascontiguousarray(R, dtype=np.float64).reshape(-1, natm, 3)
    return R.shape[0], torch.from_numpy(R).to(DEV)


def run(R, basis, flags, null_grad=False, fetch=None):
    """One call of ``evc_<basis.route>_integrals_batch`` on fresh poisoned buffers -> (rc, {name: host array}, fences
    intact, raw Fenced buffers).  ``null_grad``: null pointers for the gradient arrays (no buffers for them).  ``fetch``: the names
    to read back (default: all); the others stay on the device in their Fenced buffers."""
    lib = _lib.load()
    G, dR = _coords(R, basis.natm)
    shp = shapes(basis.natm, basis.nao, G, flags)
    bufs = {k: Fenced(int(np.prod(s))) for k, s in shp.items() if not (null_grad and k in GRAD_FIELDS)}
    need = getattr(lib, f"evc_{basis.route}_workspace_bytes")(basis.natm, basis.nshell, basis.nprim, basis.nao, G)
    assert need > 0 and need % 8 == 0, lib.evc_last_error()
    ws = Fenced(need // 8)
    dZ = torch.from_numpy(basis.charges).to(DEV)
    out = _lib.SgtoOutputs(**{k: (bufs[k].ptr if k in bufs else None) for k in shp})
    rc = getattr(lib, f"evc_{basis.route}_integrals_batch")(
        basis.natm, basis.nshell, G, dR.data_ptr(), dZ.data_ptr(), *basis.pointers(), C.byref(out), int(flags), ws.ptr,
        need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    arrays = {k: b.payload(shp[k]) for k, b in bufs.items() if fetch is None or k in fetch}
    intact = all(b.fences_intact() for b in bufs.values()) and ws.fences_intact()
    return rc, arrays, intact, bufs


def run_dipole(R, basis, origin):
    """One call of ``evc_<basis.route>_dipole_batch`` on a fresh poisoned buffer -> (rc, host (G,3,N,N), fences intact,
    Fenced)."""
    lib = _lib.load()
    G, dR = _coords(R, basis.natm)
    n = basis.nao
    dip = Fenced(G * 3 * n * n)
    o = (C.c_double * 3)(*[float(x) for x in origin])
    rc = getattr(lib, f"evc_{basis.route}_dipole_batch")(
        basis.natm, basis.nshell, G, dR.data_ptr(), *basis.pointers(), C.cast(o, C.c_void_p), dip.ptr,
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, dip.payload((G, 3, n, n)), dip.fences_intact(), dip


def pack_eri(full):
    """(G,n,n,n,n) -> the s4 form (G,Ms,Ms): the elements mu >= nu, kappa >= lambda."""
    iu, ju = np.tril_indices(full.shape[-1])
    return full[:, iu, ju][:, :, iu, ju]


def pack_ip1(full):
    """(G,3,n,n,n,n) -> the s2kl form (G,3,n,n,Ms)."""
    iu, ju = np.tril_indices(full.shape[-1])
    return full[..., iu, ju]
