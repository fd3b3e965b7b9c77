"""How the GPU tests of the observables kernels call ``evc_properties_roots_batch`` (tests/test_gpu_properties.py,
tests/test_gpu_properties_limits.py) -- a helper, no test: random inputs of one call through ctypes, a hand-made evaluation
workspace, the numpy statement evcont_amd/properties.py as the reference and, on request, NaN-poisoned outputs and scratch
between two guards each (sgto_harness.Fenced)."""
import ctypes as C
import os
import re

import numpy as np
import torch

DEV = "cuda"
BAR = 1e-10
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("d_oao", "d_ao", "dipole", "mulliken", "loewdin")


def source_constant(name):
    """``constexpr int <name>`` of the code under test."""
    with open(os.path.join(REPO, "evcont_amd", "csrc", "properties.hip")) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


def rows_min():
    """Rows of one_rdm above which the row sum is split over blocks, read from the code under test."""
    return source_constant("kPropRowsMin")


def slices_of(sizes):
    stops = np.cumsum(sizes)
    return np.stack([stops - np.array(sizes), stops], axis=1).astype(np.int64)


class Problem:
    """Random inputs of one evc_properties_roots_batch call and a hand-made evaluation workspace that holds X of every
    geometry where carve() puts it (the head of a geometry's slot).  The kernels do not know physics: X is the Loewdin
    transformation of a random overlap matrix, dip and S are random symmetric matrices.

    ``symmetric=False``: nothing is symmetric -- one_rdm is a plain random (T,T,n,n) tensor (so D is a general matrix), S
    (+ 1 on the diagonal, which keeps its size), dip and X (over sqrt(n); no Loewdin transformation: the kernels only read
    X from the workspace) plain random matrices; an index choice of a kernel then differs from its transpose.
    ``aoslices``: an explicit (A,2) array in place of the one built from ``sizes``; A may exceed n.
    ``fenced``: every output and the scratch (of exactly evc_properties_workspace_bytes bytes) are NaN-poisoned between
    guards, and ``call`` returns (outputs, every fence intact)."""

    def __init__(self, n, T, G, pairs, sizes, seed, symmetric=True, aoslices=None, fenced=False, upload=True):
        """``upload=False``: the host inputs and ``reference()`` alone, for checks of the inputs that need no device."""
        from evcont_amd import _lib
        from oracle import evcont_oracle as orc
        self.lib = _lib.load()
        rng = np.random.default_rng(seed)
        self.n, self.T, self.G, self.fenced = n, T, G, fenced
        self.pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        self.nvec = int(self.pairs.max()) + 1
        assert self.nvec <= T
        if aoslices is None:
            assert sum(sizes) == n
            self.aoslices = slices_of(sizes)
        else:
            self.aoslices = np.ascontiguousarray(np.asarray(aoslices, dtype=np.int64).reshape(-1, 2))
        self.A = len(self.aoslices)
        if symmetric:
            sym = lambda a: a + np.swapaxes(a, -1, -2)
            B = rng.standard_normal((G, n, n))
            self.S = B @ np.swapaxes(B, -1, -2) / n + np.eye(n)
            self.X = np.stack([orc.loewdin_trafo(s) for s in self.S])
            self.dip = sym(rng.standard_normal((G, 3, n, n)))
            one = rng.standard_normal((T, T, n, n)) / n
            self.one = 0.5 * (one + one.transpose(1, 0, 3, 2))
        else:
            self.S = rng.standard_normal((G, n, n)) + np.eye(n)
            self.X = rng.standard_normal((G, n, n)) / np.sqrt(n)
            self.dip = rng.standard_normal((G, 3, n, n))
            self.one = rng.standard_normal((T, T, n, n)) / n
        self.coeffs = rng.standard_normal((G, T, T)) / np.sqrt(T)
        self.charges = rng.uniform(0.5, 3.0, self.A)
        self.coords = rng.uniform(-5.0, 5.0, (G, self.A, 3))       # within 10 Bohr
        self.origin = (0.4, -0.3, 1.2)
        if upload:
            self._upload()

    def single(self, g, p):
        """The call on geometry ``g`` and root pair ``p`` of this problem alone: count = 1, npairs = 1."""
        import copy
        sub = copy.copy(self)
        sub.G, sub.pairs = 1, np.ascontiguousarray(self.pairs[p: p + 1])
        sub.nvec = int(sub.pairs.max()) + 1
        sub.S, sub.X, sub.dip, sub.coeffs, sub.coords = (a[g: g + 1] for a in (self.S, self.X, self.dip, self.coeffs,
                                                                                 self.coords))
        sub._upload()
        return sub

    def _upload(self):
        from evcont_amd import _lib
        n, T, G, fenced = self.n, self.T, self.G, self.fenced
        n2 = n * n
        ld1 = n2 + (n2 & 1)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        one_d = torch.zeros((T * T, ld1), dtype=torch.float64, device=DEV)
        one_d[:, :n2] = up(self.one.reshape(T * T, n2))
        self.dev = dict(one=one_d, S=up(self.S), dip=up(self.dip), coeffs=up(self.coeffs), charges=up(self.charges),
                        coords=up(self.coords), aoslices=up(self.aoslices), dummy=torch.zeros(64, dtype=torch.float64, device=DEV))
        P, M = T * (T + 1) // 2, n2 * (n2 + 1) // 2
        self.t = _lib.TrdmSet(n=n, ntrain=T, layout=2, rows2=P, row_offset=0, rows2_total=P, cols2=M,
                              ld2=(M + 15) // 16 * 16, ld1=ld1, two_rdm=self.dev["dummy"].data_ptr(),
                              one_rdm=one_d.data_ptr(), s_train=self.dev["dummy"].data_ptr())
        self.per_geo = self.lib.evc_workspace_bytes(C.byref(self.t), self.A)
        assert self.per_geo >= n2 * 8
        # nothing but X is read from it
        self.ws = torch.empty(self.per_geo * G, dtype=torch.uint8, device=DEV)
        for g in range(G):
            self.ws[g * self.per_geo: g * self.per_geo + n2 * 8].view(torch.float64).copy_(up(self.X[g]).reshape(-1))
        nbytes = self.lib.evc_properties_workspace_bytes(n, T, self.A, G, len(self.pairs))
        assert nbytes > 0
        self.scratch_bytes = nbytes
        if fenced:
            from sgto_harness import Fenced
            assert nbytes % 8 == 0
            self.scratch = Fenced(nbytes // 8)
        else:
            self.scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

    def call(self, want=OUTPUTS):
        from evcont_amd import _lib
        n, A, G, npairs = self.n, self.A, self.G, len(self.pairs)
        shapes = {"d_oao": (n, n), "d_ao": (n, n), "dipole": (3,), "mulliken": (A,), "loewdin": (A,)}
        if self.fenced:
            from sgto_harness import Fenced
            bufs = {k: Fenced(npairs * G * int(np.prod(shapes[k]))) for k in want}
            out = {k: b.device((npairs, G) + shapes[k]) for k, b in bufs.items()}
            self.scratch.device().fill_(float("nan"))      # poisoned again: a partial sum of an earlier call does not serve
            ptr = {k: b.ptr for k, b in bufs.items()}
            scratch_ptr = self.scratch.ptr
        else:
            # NaN-filled: an element the call leaves out shows
            out = {k: torch.full((npairs, G) + shapes[k], float("nan"), dtype=torch.float64, device=DEV) for k in want}
            ptr = {k: v.data_ptr() for k, v in out.items()}
            scratch_ptr = self.scratch.data_ptr()
        d = self.dev
        pin = _lib.PropertyInputs(natm=A, count=G, S=d["S"].data_ptr(), dip=d["dip"].data_ptr(),
                                  aoslices=d["aoslices"].data_ptr(), charges=d["charges"].data_ptr(),
                                  coords=d["coords"].data_ptr(), origin=(C.c_double * 3)(*self.origin))
        pout = _lib.PropertyOutputs(**{k: ptr.get(k) for k in OUTPUTS})
        rc = self.lib.evc_properties_roots_batch(C.byref(self.t), C.byref(pin), d["coeffs"].data_ptr(), self.nvec,
                                                 self.pairs.ctypes.data, npairs, C.byref(pout), self.ws.data_ptr(),
                                                 int(self.ws.numel()), scratch_ptr, self.scratch_bytes,
                                                 torch.cuda.current_stream().cuda_stream)
        assert rc == 0, self.lib.evc_last_error()
        torch.cuda.synchronize()
        if self.fenced:
            return out, all(b.fences_intact() for b in bufs.values()) and self.scratch.fences_intact()
        return out

    def reference(self):
        from evcont_amd import properties as pr
        per_geo = [pr.properties_host(self.one, self.X[g], self.coeffs[g], self.pairs, self.S[g], self.dip[g],
                                      self.aoslices, self.charges, self.coords[g], self.origin) for g in range(self.G)]
        return {k: np.stack([r[k] for r in per_geo], axis=1) for k in OUTPUTS}      # root-pair-major


def deviations(got, want, what):
    """{output: max |got - want|}, printed; every element finite."""
    worst = {}
    for k in got:
        a = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        assert np.all(np.isfinite(a)), (what, k)
        worst[k] = float(np.abs(a - want[k]).max())
    print(what, " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    return worst


def compare(got, want, what):
    worst = deviations(got, want, what)
    assert max(worst.values()) < BAR, (what, worst)
    return worst
