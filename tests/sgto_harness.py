"""How the GPU tests of the s-Gaussian device integrals call ``evc_sgto_integrals_batch`` (tests/test_gpu_sgto.py,
tests/test_gpu_sgto_limits.py) -- a helper, no test: through ctypes, on NaN-poisoned output buffers and workspace between
two guards each, read back in full or, for buffers of gigabytes, by slice."""
import ctypes as C

import numpy as np
import torch

from evcont_amd import _lib

DEV = "cuda"
FENCE, GUARD = 12345.678, 64          # guard doubles on either side of every buffer
MODES = {"packed": _lib.FLAG_ERI_S4 | _lib.FLAG_IP1_S2KL, "full": 0, "energy": _lib.FLAG_ENERGY_ONLY}
GRAD_FIELDS = ("ipovlp", "dhcore", "eri_ip1", "gnuc")


def _shapes(A, G, packed):
    n, ms = A, A * (A + 1) // 2
    return {"enuc": (G,), "S": (G, n, n), "hcore": (G, n, n), "eri": (G, ms, ms) if packed else (G, n, n, n, n),
            "ipovlp": (G, 3, n, n), "dhcore": (G, A, 3, n, n), "gnuc": (G, A, 3),
            "eri_ip1": (G, 3, n, n, ms) if packed else (G, 3, n, n, n, n)}


class Fenced:
    """A device buffer of ``count`` doubles filled with NaN between two guards of FENCE."""

    def __init__(self, count):
        self.count = int(count)
        self.buf = torch.full((self.count + 2 * GUARD,), float("nan"), dtype=torch.float64, device=DEV)
        self.buf[:GUARD] = FENCE
        self.buf[GUARD + self.count:] = FENCE

    @property
    def ptr(self):
        return self.buf.data_ptr() + 8 * GUARD

    def fences_intact(self):
        lo, hi = self.buf[:GUARD].cpu().numpy(), self.buf[GUARD + self.count:].cpu().numpy()
        return bool(np.all(lo == FENCE) and np.all(hi == FENCE))

    def payload(self, shape=None):
        h = self.buf[GUARD:GUARD + self.count].cpu().numpy().copy()
        return h if shape is None else h.reshape(shape)

    def device(self, shape=None):
        """The payload as a view on the device (for checks that leave a large buffer where it is)."""
        d = self.buf[GUARD:GUARD + self.count]
        return d if shape is None else d.view(shape)

    def rows(self, shape, index):
        """``payload(shape)[index]`` read back alone; ``index`` a tuple of integers for the leading axes."""
        return self.device(shape)[tuple(index)].cpu().numpy().copy()


def run(R, Z, basis, mode, null_grad=False, ws_bytes=None, flags=None, fetch=None, **override):
    """One call on fresh poisoned buffers -> (rc, {name: host array}, fences intact, raw Fenced buffers).  ``fetch``: the
    names to read back in full (default: all); the others stay on the device in their Fenced buffers."""
    lib = _lib.load()
    R = np.ascontiguousarray(R, dtype=np.float64)
    G, A, K = R.shape[0], R.shape[1], len(basis[0])
    shapes = _shapes(A, G, mode == "packed")
    bufs = {k: Fenced(int(np.prod(s))) for k, s in shapes.items()}
    need = lib.evc_sgto_workspace_bytes(A, K, G)
    assert need > 0 and need % 8 == 0
    ws = Fenced(need // 8)
    dR = torch.from_numpy(R).to(DEV)
    dZ = torch.from_numpy(np.ascontiguousarray(Z, dtype=np.float64)).to(DEV)
    ex, co = (np.ascontiguousarray(b, dtype=np.float64) for b in basis)
    out = _lib.SgtoOutputs(**{k: (None if (null_grad and k in GRAD_FIELDS) else b.ptr) for k, b in bufs.items()})
    args = dict(natm=A, nprim=K, count=G, coords=dR.data_ptr(), charges=dZ.data_ptr(), ex=ex.ctypes.data,
                co=co.ctypes.data, out=C.byref(out), flags=MODES[mode] if flags is None else flags, ws=ws.ptr,
                ws_bytes=need if ws_bytes is None else ws_bytes)
    args.update(override)
    rc = lib.evc_sgto_integrals_batch(args["natm"], args["nprim"], args["count"], args["coords"], args["charges"],
                                      args["ex"], args["co"], args["out"], args["flags"], args["ws"], args["ws_bytes"],
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    arrays = {k: b.payload(shapes[k]) for k, b in bufs.items() if fetch is None or k in fetch}
    intact = all(b.fences_intact() for b in bufs.values()) and ws.fences_intact()
    return rc, arrays, intact, bufs


def unpack(arrays, A):
    """The full forms of packed ``eri`` (G,Ms,Ms) and ``eri_ip1`` (G,3,N,N,Ms)."""
    iu, ju = np.tril_indices(A)
    P = np.zeros((A, A), dtype=np.int64)
    P[iu, ju] = P[ju, iu] = np.arange(len(iu))
    return arrays["eri"][:, P][:, :, :, P], arrays["eri_ip1"][..., P]
