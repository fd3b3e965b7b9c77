"""How the GPU tests of csrc/spdgto.hip call ``evc_spdgto_integrals_batch`` and ``evc_spdgto_dipole_batch`` -- a helper,
no test, the s + p + d counterpart of tests/spgto_harness.py: through ctypes, with the flattened basis and arbitrary
flags, on NaN-poisoned output buffers and workspace between two guards each (``Fenced``).  The molecules are in
tests/spdgto_cases.py."""
import ctypes as C

import numpy as np
import torch

from evcont_amd import _lib
from evcont_amd.gto_spd import contraction_coefficients
from sgto_harness import DEV, FENCE, GUARD, Fenced                      # noqa: F401 (FENCE, GUARD: for the tests)
from spgto_harness import (ENERGY, ENERGY_FIELDS, GRAD_FIELDS, S2KL, S4, _coords, pack_eri, pack_ip1,  # noqa: F401
                           shapes)
import spgto_harness


class Basis(spgto_harness.Basis):
    """``spgto_harness.Basis`` with the shells and the normalisation of ``gto_spd`` (l <= 2)."""

    def __init__(self, charges, shells, renormalize=True):
        coef = contraction_coefficients(shells, renormalize)
        atom, l, off, ex, co, slices, n = [], [], [0], [], [], [], 0
        for at, (shs, cs) in enumerate(zip(shells, coef)):
            start = n
            for sh, c in zip(shs, cs):
                atom.append(at)
                l.append(sh.l)
                off.append(off[-1] + len(sh.exponents))
                ex += list(sh.exponents)
                co += list(c)
                n += 2 * sh.l + 1
            slices.append((start, n))
        self.charges = np.ascontiguousarray(charges, dtype=np.float64).reshape(-1)
        assert len(shells) == self.charges.shape[0]
        self.shell_atom = np.array(atom, dtype=np.int32)
        self.shell_l = np.array(l, dtype=np.int32)
        self.shell_prim_offset = np.array(off, dtype=np.int32)
        self.exponents = np.array(ex, dtype=np.float64)
        self.coefficients = np.array(co, dtype=np.float64)
        self.aoslices = np.array(slices, dtype=np.int64).reshape(-1, 2)
        self.natm, self.nshell, self.nprim, self.nao = len(shells), len(atom), off[-1], n
        self.shells = shells


def run(R, basis, flags, null_grad=False, fetch=None):
    """One call of ``evc_spdgto_integrals_batch`` on fresh poisoned buffers -> (rc, {name: host array}, fences intact,
    raw Fenced buffers); the arguments of ``spgto_harness.run``."""
    lib = _lib.load()
    G, dR = _coords(R, basis.natm)
    shp = shapes(basis.natm, basis.nao, G, flags)
    bufs = {k: Fenced(int(np.prod(s))) for k, s in shp.items() if not (null_grad and k in GRAD_FIELDS)}
    need = lib.evc_spdgto_workspace_bytes(basis.natm, basis.nshell, basis.nprim, basis.nao, G)
    assert need > 0 and need % 8 == 0, lib.evc_last_error()
    ws = Fenced(need // 8)
    dZ = torch.from_numpy(basis.charges).to(DEV)
    out = _lib.SgtoOutputs(**{k: (bufs[k].ptr if k in bufs else None) for k in shp})
    rc = lib.evc_spdgto_integrals_batch(basis.natm, basis.nshell, G, dR.data_ptr(), dZ.data_ptr(), *basis.pointers(),
                                        C.byref(out), int(flags), ws.ptr, need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    arrays = {k: b.payload(shp[k]) for k, b in bufs.items() if fetch is None or k in fetch}
    intact = all(b.fences_intact() for b in bufs.values()) and ws.fences_intact()
    return rc, arrays, intact, bufs


def run_dipole(R, basis, origin):
    """One call of ``evc_spdgto_dipole_batch`` on a fresh poisoned buffer -> (rc, host (G,3,N,N), fences intact, Fenced)."""
    lib = _lib.load()
    G, dR = _coords(R, basis.natm)
    n = basis.nao
    dip = Fenced(G * 3 * n * n)
    o = (C.c_double * 3)(*[float(x) for x in origin])
    rc = lib.evc_spdgto_dipole_batch(basis.natm, basis.nshell, G, dR.data_ptr(), *basis.pointers(), C.cast(o, C.c_void_p),
                                     dip.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, dip.payload((G, 3, n, n)), dip.fences_intact(), dip
