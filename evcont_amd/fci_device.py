"""``DeviceFCI``: the small determinant full-CI solver of ``fci_small.SmallFCI`` with its two heavy operations on the
GPU (``csrc/fci.hip``): the sigma vector ``H c`` and the transition RDMs.  Same calls, same conventions:

    e, ci = solver.kernel(h1, h2, norb, nelec, nroots=k)
    dm1, dm2 = solver.trans_rdm12(cibra, ciket, norb, nelec)       # dm1[p,q] = <q^+ p>, dm2[p,q,r,s] = <p^+ r^+ s q>

plus ``trans_rdm12_rows(bra, kets, norb, nelec)``: one bra against all kets in one pass, which is what
``FCI_EVCont_obj.append_to_rdms`` needs for a new training state, ``trans_rdm12_rows_packed(..., layout, out_rows)``: the
same call with its two-body rows written on the device in the evaluator's layout (``csrc/fci_pack.hip``; the training
set of ``resident.ResidentFCI_EVCont_obj``), and ``transform_ci(ci, nelec, u)``
(``csrc/fci_rotate.hip``), which rotates a state solved in another orbital basis into the OAO basis, and
``cas_trans_rdm12_rows(bra, kets)``: the t-RDMs between CAS states in different orbital sets, expanded to all N orbitals
on the device (``csrc/cas_expand.hip``; ``CAS_EVCont_obj(ncas, neleca, cisolver=DeviceFCI())``), with
``cas_trans_rdm12_block(bras, kets)`` for the roots of one geometry (one ``evc_fci_rotate_block`` per stored geometry;
``transform_ci_block`` is that rotation on its own; all bras go through one ``evc_fci_trdm_rows_block`` call, and
``triangular=True`` is the ragged form of a training-set append, ``resident.ResidentCAS_EVCont_obj``).  Opt in with
``FCI_EVCont_obj(cisolver=DeviceFCI(), cibasis="OAO")``, or ``cibasis="canonical"`` to solve in the Hartree-Fock basis,
where the Davidson solver's diagonal preconditioner works best near equilibrium.

``DeviceFCI(spin_penalty=0.2)`` holds the roots to one multiplicity (``H + 0.2 (S^2 - S(S+1))``, PySCF's ``fix_spin_``;
``csrc/fci_spin.hip``) and ``spin_square(ci, norb, nelec)`` reports ``<S^2>`` of a state.

Limits: ``norb <= 16``, real CI vectors, any ``(n_alpha, n_beta)``.  By default the eigensolver iteration of ``kernel``
stays on the host (``scipy.sparse.linalg.eigsh``); every matrix-vector product it asks for is a device sigma vector that
is uploaded and downloaded.  ``DeviceFCI(eigensolver="davidson")`` runs a block Davidson (``fci_davidson.py``) whose
CI-length vectors stay on the device (``csrc/fci_solve.hip``); the host sees the projected matrix, the Ritz coefficients
and the residual norms.  There is no host fallback: without the library or a device every call raises
``EvcontHipError``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from scipy.sparse.linalg import LinearOperator, eigsh

from . import _lib
from .fci_davidson import DavidsonOps, davidson
from ._lib import EvcontHipError, check
from .fci_small import _strings, multiplicity_of, resolve_spin_target, unshift_roots
from .fci_tables import MAX_ORB, packed_table

F64 = torch.float64


def _nelec(nelec) -> Tuple[int, int]:
    if isinstance(nelec, (int, np.integer)):
        return (int(nelec) + 1) // 2, int(nelec) // 2
    return int(nelec[0]), int(nelec[1])


class _DeviceOps(DavidsonOps):
    """The vector operations of ``fci_davidson.davidson`` on device storage: ``evc_fci_hdiag``, ``evc_fci_dots``,
    ``evc_fci_combine``, ``evc_fci_davidson_correction`` and ``evc_fci_sigma``.  Coefficients go up and products come
    down as small arrays; no CI-length vector crosses but ``load`` (start vectors) and ``fetch`` (results)."""

    def __init__(self, fci: "DeviceFCI", lib, dta, dtb, na, nb, grant, norb, dh1, dh2):
        self.fci, self.lib, self.dta, self.dtb, self.na, self.nb = fci, lib, dta, dtb, na, nb
        self.grant, self.norb, self.dh1, self.dh2 = grant, norb, dh1, dh2
        self.dim = na * nb
        self.dev = dta.device
        self.nsigma = 0
        self.sets = {}
        self.hd = None
        self.shift, self.target = fci._pen

    def prepare(self, nroots, max_space):
        lib, dim = self.lib, self.dim
        nvec = max(max_space, 2 * nroots)
        wsb = lib.evc_fci_solve_workspace_bytes(self.norb, self.na, self.nb, nvec)
        if wsb == 0:
            check(-1, "evc_fci_solve_workspace_bytes")
        rows = 2 * max_space + 2 * nroots + 1
        small = (nvec * nvec + nvec * 2 * nroots + 4 * nroots) * 8
        need = rows * dim * 8 + wsb + small
        key = (self.norb, self.na, self.nb, max_space, nroots)
        store = self.fci._basis
        if store is None or store[0] != key:
            self.fci._basis = store = None
            free = torch.cuda.mem_get_info(self.dev)[0]
            if need > free:
                raise EvcontHipError(f"DeviceFCI: the Davidson basis of {rows} vectors of {dim} determinants needs "
                                     f"{need} bytes, the device has {free} free (max_space={max_space}, nroots={nroots})")
            store = (key, torch.empty((rows, dim), dtype=F64, device=self.dev),
                     torch.empty(wsb, dtype=torch.uint8, device=self.dev))
            self.fci._basis = store
        _, basis, self.ws = store
        self.wsb = wsb
        self.sets = {"V": basis[:max_space], "W": basis[max_space:2 * max_space],
                     "S": basis[2 * max_space:2 * max_space + 2 * nroots]}
        self.hd = basis[rows - 1]
        self.out = torch.empty(nvec * nvec, dtype=F64, device=self.dev)
        check(lib.evc_fci_hdiag(self.norb, self.na, self.nb, self.dta.data_ptr(), self.dtb.data_ptr(), self.dh1.data_ptr(),
                                self.dh2.data_ptr(), self.hd.data_ptr(), self.ws.data_ptr(), wsb, self.fci._stream()),
              "evc_fci_hdiag")
        if self.shift != 0.0:
            check(lib.evc_fci_spin_diag(self.norb, self.na, self.nb, self.dta.data_ptr(), self.dtb.data_ptr(), self.shift,
                                        self.target, self.hd.data_ptr(), self.fci._stream()), "evc_fci_spin_diag")

    def _row(self, name, row):
        return self.sets[name].data_ptr() + 8 * row * self.dim

    def lowest(self, n):
        return [int(i) for i in torch.sort(self.hd, stable=True).indices[:n].cpu()]

    def load(self, name, row, vec):
        self.sets[name][row].copy_(torch.from_numpy(np.ascontiguousarray(vec, dtype=np.float64).reshape(-1)))

    def fetch(self, name, row):
        return self.sets[name][row].cpu().numpy()

    def copy(self, dst, d0, src, s0, count):
        self.sets[dst][d0:d0 + count].copy_(self.sets[src][s0:s0 + count])

    def sigma(self, row):
        self.nsigma += 1
        check(self.lib.evc_fci_sigma(self.norb, self.na, self.nb, self.dta.data_ptr(), self.dtb.data_ptr(),
                                     self.dh1.data_ptr(), self.dh2.data_ptr(), self._row("V", row), self._row("W", row),
                                     self.fci._ws.data_ptr(), self.grant, self.fci._stream()), "evc_fci_sigma")
        if self.shift != 0.0:
            self.fci._add_penalty(self.lib, self.dta, self.dtb, self.na, self.nb, self.norb, self.shift, self.target,
                                  self._row("V", row), self._row("W", row))

    def dots(self, x, x0, nx, y, y0, ny):
        check(self.lib.evc_fci_dots(self.dim, self._row(x, x0), self.dim, nx, self._row(y, y0), self.dim, ny,
                                    self.out.data_ptr(), self.ws.data_ptr(), self.wsb, self.fci._stream()), "evc_fci_dots")
        return self.out[:nx * ny].cpu().numpy().reshape(nx, ny)

    def _small(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)

    def combine(self, out, o0, src, s0, coef, beta):
        m, k = coef.shape
        dcoef = self._small(coef)
        check(self.lib.evc_fci_combine(self.dim, self._row(src, s0), self.dim, m, dcoef.data_ptr(), k, k, float(beta),
                                       self._row(out, o0), self.dim, self.fci._stream()), "evc_fci_combine")

    def correction(self, m, y, theta):
        k = y.shape[1]
        dy, dth = self._small(y), self._small(theta)
        check(self.lib.evc_fci_davidson_correction(self.dim, self._row("V", 0), self.dim, self._row("W", 0), self.dim, m,
                                                   dy.data_ptr(), k, dth.data_ptr(), k, self.hd.data_ptr(),
                                                   self._row("S", 0), self.dim, self.out.data_ptr(), self.ws.data_ptr(),
                                                   self.wsb, self.fci._stream()), "evc_fci_davidson_correction")
        return self.out[:k].cpu().numpy()


EIGENSOLVERS = ("host", "davidson")
ROTATE_RESIDENT_BYTES = 1 << 28     # transform_ci: largest workspace granted without being asked (256 MiB)


class DeviceFCI:
    """``workspace_bytes=None`` grants what keeps every intermediate resident (``evc_fci_workspace_bytes``: two
    ``dim x npad`` excitation arrays and the split-K partials; 2.1 GB at (12, (6, 6))); a smaller grant makes the
    library work in chunks of determinants, with the same results bit for bit.

    ``eigensolver="host"`` (the default): ``kernel`` diagonalises densely up to ``dense_limit`` determinants and runs
    ``eigsh`` on the host beyond.  ``eigensolver="davidson"``: block Davidson with resident vectors at every size, a root
    converged when its residual 2-norm is at most ``conv_tol``; the basis holds at most ``max_space`` vectors (default
    ``8 nroots + 12``) and ``2 max_space + 2 nroots + 1`` vectors are allocated, once per shape; ``converged`` is False,
    with a warning, when ``max_cycle`` iterations did not suffice.

    ``spin_penalty`` / ``spin_target`` as in ``SmallFCI``: with a non-zero penalty every sigma vector, on all three
    routes, is ``H c + spin_penalty (S^2 c - spin_target c)`` (``evc_fci_spin_apply`` on the row ``evc_fci_sigma`` just
    wrote, csrc/fci_spin.hip), the Davidson diagonal carries the same penalty, and ``kernel`` returns energies of H with
    the measured ``<S^2>`` of its roots in ``spin_squares``.  With the default 0 no such kernel is launched."""

    def __init__(self, device=None, tol: float = 1e-13, workspace_bytes: Optional[int] = None, dense_limit: int = 1500,
                 eigensolver: str = "host", conv_tol: float = 1e-10, max_space: Optional[int] = None,
                 max_cycle: int = 300, spin_penalty: float = 0.0, spin_target: Optional[float] = None):
        if eigensolver not in EIGENSOLVERS:
            raise ValueError(f"DeviceFCI: eigensolver={eigensolver!r}, expected one of {EIGENSOLVERS}")
        self.eigensolver = eigensolver
        self.conv_tol, self.max_space, self.max_cycle = conv_tol, max_space, max_cycle
        self.davidson_info = None
        self.spin_penalty, self.spin_target, self.spin_squares = float(spin_penalty), spin_target, None
        self._pen = (0.0, 0.0)  # (penalty, S(S+1) target) of the shape last set up
        self._basis = None
        self.tol = tol
        self.dense_limit = dense_limit
        self.workspace_bytes = workspace_bytes
        self.converged = True
        self._device_arg = device
        self._device = None
        self._tables = {}
        self._masks = {}    # (norb, nelec) -> occupation masks of the alpha / beta strings on the device (transform_ci)
        self._ws = None
        self._cas_ws = None  # workspace of evc_cas_expand_rows (cas_trans_rdm12_rows)
        # id(host array) -> (host array, host copy of what was uploaded, device tensor): CI vectors already uploaded
        self._vecs = {}

    # ---- plumbing ----------------------------------------------------------------
    def _dev(self) -> torch.device:
        if self._device is None:
            _lib.load()
            if not torch.cuda.is_available():
                raise EvcontHipError("DeviceFCI needs a HIP device (evcont_amd has no CPU fallback; "
                                     "fci_small.SmallFCI is the host solver)")
            self._device = torch.device(self._device_arg if self._device_arg is not None else "cuda:0")
        return self._device

    def _check_shape(self, norb: int, nelec: Tuple[int, int]) -> None:
        if not 1 <= norb <= MAX_ORB:
            raise EvcontHipError(f"DeviceFCI: norb={norb}, supported 1 ... {MAX_ORB}")
        if not (0 <= nelec[0] <= norb and 0 <= nelec[1] <= norb):
            raise EvcontHipError(f"DeviceFCI: nelec={nelec} for {norb} orbitals")

    def _setup(self, norb: int, nelec: Tuple[int, int]):
        """Tables on the device and a workspace the library accepts; every limit is checked before any launch."""
        self._check_shape(norb, nelec)
        lib = _lib.load()
        key = (norb, nelec)
        if key not in self._tables:
            ta = packed_table(norb, nelec[0])
            tb = ta if nelec[1] == nelec[0] else packed_table(norb, nelec[1])
            na, nb = ta.shape[0], tb.shape[0]
            least = lib.evc_fci_workspace_bytes(norb, na, nb, 1)
            full = lib.evc_fci_workspace_bytes(norb, na, nb, 0)
            if least == 0 or full == 0:
                check(-1, "evc_fci_workspace_bytes")
            grant = full if self.workspace_bytes is None else int(self.workspace_bytes)
            if grant < least:
                raise EvcontHipError(f"DeviceFCI: workspace_bytes={grant}, but {na * nb} determinants of {norb} orbitals "
                                     f"need at least {least} bytes ({full} to keep everything resident)")
            dev = self._dev()
            dta = torch.from_numpy(ta).to(dev)
            dtb = dta if tb is ta else torch.from_numpy(tb).to(dev)
            self._tables[key] = (dta, dtb, na, nb, min(grant, full))
            dsa = torch.tensor(_strings(norb, nelec[0]), dtype=torch.int32, device=dev)
            dsb = dsa if nelec[1] == nelec[0] else torch.tensor(_strings(norb, nelec[1]), dtype=torch.int32, device=dev)
            self._masks[key] = (dsa, dsb)
        dta, dtb, na, nb, grant = self._tables[key]
        self._pen = self._penalty(nelec)            # a spin_target that is no S(S+1) is refused here (ValueError)
        if self._ws is None or self._ws.numel() < grant:
            self._ws = None
            self._ws = torch.empty(grant, dtype=torch.uint8, device=self._dev())
        return lib, dta, dtb, na, nb, grant

    def _stream(self) -> int:
        return torch.cuda.current_stream(self._dev()).cuda_stream

    def _upload(self, v, na: int, nb: int, cache: bool) -> torch.Tensor:
        if torch.is_tensor(v):
            t = v.to(self._dev(), F64).contiguous()
        else:
            if np.iscomplexobj(v):
                raise EvcontHipError("DeviceFCI: complex CI vectors are not supported")
            # A cached copy is used only while the host array still holds what was uploaded: the array may have been
            # changed in place since (one pass over the host data per vector; a NaN anywhere compares unequal and
            # uploads again).
            hit = self._vecs.get(id(v))
            if hit is not None and hit[0] is v and np.array_equal(hit[1], v):
                return hit[2]
            t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(self._dev())
            if cache:
                self._vecs[id(v)] = (v, np.array(v, copy=True), t)
        if t.numel() != na * nb:
            raise EvcontHipError(f"DeviceFCI: CI vector of {t.numel()} elements, expected {na} x {nb}")
        return t

    def forget(self, keep: Sequence = ()) -> None:
        """Drop the device copies of CI vectors, except those of the host arrays in ``keep`` (after pruning a
        container: ``solver.forget(cont.fcivecs)``)."""
        ids = {id(v) for v in keep}
        self._vecs = {k: hv for k, hv in self._vecs.items() if k in ids}

    # ---- the SmallFCI interface --------------------------------------------------
    def contract(self, h1, h2, c, norb, nelec):
        """sigma = H c, shape ``(na, nb)`` (``SmallFCI.contract``)."""
        nelec = _nelec(nelec)
        lib, dta, dtb, na, nb, grant = self._setup(norb, nelec)
        dev = self._dev()
        dh1 = torch.from_numpy(np.ascontiguousarray(h1, dtype=np.float64).reshape(norb, norb)).to(dev)
        dh2 = torch.from_numpy(np.ascontiguousarray(h2, dtype=np.float64).reshape(norb ** 4)).to(dev)
        return self._sigma(lib, dta, dtb, na, nb, grant, norb, dh1, dh2,
                           self._upload(c, na, nb, cache=False)).cpu().numpy().reshape(na, nb)

    def _sigma(self, lib, dta, dtb, na, nb, grant, norb, dh1, dh2, dc) -> torch.Tensor:
        out = torch.empty(na * nb, dtype=F64, device=dc.device)
        check(lib.evc_fci_sigma(norb, na, nb, dta.data_ptr(), dtb.data_ptr(), dh1.data_ptr(), dh2.data_ptr(),
                                dc.data_ptr(), out.data_ptr(), self._ws.data_ptr(), grant, self._stream()),
              "evc_fci_sigma")
        shift, target = self._pen
        if shift != 0.0:
            self._add_penalty(lib, dta, dtb, na, nb, norb, shift, target, dc.data_ptr(), out.data_ptr())
        return out

    def _penalty(self, nelec) -> Tuple[float, float]:
        """``(spin_penalty, S(S+1) target)``; the target is resolved, and a wrong one refused, only with a penalty."""
        shift = float(self.spin_penalty)
        return (shift, resolve_spin_target(self.spin_target, nelec)) if shift != 0.0 else (0.0, 0.0)

    def _add_penalty(self, lib, dta, dtb, na, nb, norb, shift, target, c_ptr, out_ptr) -> None:
        """``out += shift (S^2 c - target c)`` on the device."""
        check(lib.evc_fci_spin_apply(norb, na, nb, dta.data_ptr(), dtb.data_ptr(), c_ptr, shift, target, 1.0, out_ptr,
                                     self._stream()), "evc_fci_spin_apply")

    def spin_square(self, ci, norb, nelec):
        """``(<S^2>, multiplicity)`` of a normalised CI vector, a host array or a device tensor
        (``SmallFCI.spin_square``): one ``evc_fci_spin_apply`` and one ``evc_fci_dots``."""
        nelec = _nelec(nelec)
        lib, dta, dtb, na, nb, _ = self._setup(norb, nelec)
        dc = self._upload(ci, na, nb, cache=False).reshape(-1)
        dim = na * nb
        wsb = lib.evc_fci_solve_workspace_bytes(norb, na, nb, 1)
        if wsb == 0:
            check(-1, "evc_fci_solve_workspace_bytes")
        if self._ws.numel() < wsb:
            self._ws = None
            self._ws = torch.empty(wsb, dtype=torch.uint8, device=self._dev())
        s2c = torch.empty(dim, dtype=F64, device=dc.device)
        one = torch.empty(1, dtype=F64, device=dc.device)
        check(lib.evc_fci_spin_apply(norb, na, nb, dta.data_ptr(), dtb.data_ptr(), dc.data_ptr(), 1.0, 0.0, 0.0,
                                     s2c.data_ptr(), self._stream()), "evc_fci_spin_apply")
        check(lib.evc_fci_dots(dim, dc.data_ptr(), dim, 1, s2c.data_ptr(), dim, 1, one.data_ptr(), self._ws.data_ptr(),
                               wsb, self._stream()), "evc_fci_dots")
        ss = float(one.item())
        return ss, float(multiplicity_of(ss))

    def _finish(self, w, vecs, norb, nelec, nroots):
        """What ``kernel`` returns: with a penalty, the energies of H from the shifted values and the measured <S^2>."""
        w = [float(x) for x in w[:nroots]]
        self.spin_squares = None
        shift, target = self._penalty(nelec)
        if shift != 0.0:
            self.spin_squares = [self.spin_square(x, norb, nelec)[0] for x in vecs]
            w = unshift_roots(w, self.spin_squares, shift, target)
        if nroots == 1:
            return w[0], vecs[0]
        return w, vecs

    def kernel(self, h1, h2, norb, nelec, nroots: int = 1, ci0=None, **_):
        """Lowest ``nroots`` eigenpairs; scalars/array for ``nroots == 1``, lists otherwise; sign convention of
        ``SmallFCI.kernel`` (largest-magnitude coefficient positive).  Up to ``dense_limit`` determinants H is built
        column by column from device sigma vectors and diagonalised densely, beyond that Lanczos (eigsh) runs over
        them -- the same split as ``SmallFCI``.  With ``eigensolver="davidson"`` the iteration runs on the device at
        every size and ``ci0`` (one array or a list, as PySCF takes it) replaces the first start vectors; the host
        route ignores ``ci0``."""
        nelec = _nelec(nelec)
        lib, dta, dtb, na, nb, grant = self._setup(norb, nelec)
        dev = self._dev()
        dim = na * nb
        dh1 = torch.from_numpy(np.ascontiguousarray(h1, dtype=np.float64).reshape(norb, norb)).to(dev)
        dh2 = torch.from_numpy(np.ascontiguousarray(h2, dtype=np.float64).reshape(norb ** 4)).to(dev)

        if self.eigensolver == "davidson":
            return self._davidson(lib, dta, dtb, na, nb, grant, norb, dh1, dh2, nroots, ci0, nelec)

        def mv(v):
            dc = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64).reshape(-1)).to(dev)
            return self._sigma(lib, dta, dtb, na, nb, grant, norb, dh1, dh2, dc).cpu().numpy()

        if dim <= self.dense_limit:
            H = torch.empty((dim, dim), dtype=F64, device=dev)
            eye = torch.zeros(dim, dtype=F64, device=dev)
            for k in range(dim):
                eye[k] = 1.0
                H[k] = self._sigma(lib, dta, dtb, na, nb, grant, norb, dh1, dh2, eye)     # column k of H
                eye[k] = 0.0
            H = H.cpu().numpy()
            w, v = np.linalg.eigh(0.5 * (H + H.T))
        else:
            op = LinearOperator((dim, dim), matvec=mv, dtype=np.float64)
            rng = np.random.default_rng(0)
            w, v = eigsh(op, k=max(nroots, 1), which="SA", tol=self.tol, v0=rng.standard_normal(dim),
                         ncv=max(20, 2 * nroots + 10))
            order = np.argsort(w)
            w, v = w[order], v[:, order]
        vecs = []
        for k in range(nroots):
            x = v[:, k].copy()
            x *= np.sign(x[np.argmax(np.abs(x))])
            vecs.append(x.reshape(na, nb))
        return self._finish(w, vecs, norb, nelec, nroots)

    def _davidson(self, lib, dta, dtb, na, nb, grant, norb, dh1, dh2, nroots, ci0, nelec):
        ops = _DeviceOps(self, lib, dta, dtb, na, nb, grant, norb, dh1, dh2)
        try:
            w, v, self.converged, self.davidson_info = davidson(
                ops, nroots=nroots, conv_tol=self.conv_tol, max_space=self.max_space, max_cycle=self.max_cycle, ci0=ci0)
        except ValueError as e:
            raise EvcontHipError(f"DeviceFCI: {e}") from e
        vecs = []
        for k in range(nroots):
            x = v[k] / np.linalg.norm(v[k])
            x *= np.sign(x[np.argmax(np.abs(x))])
            vecs.append(x.reshape(na, nb))
        return self._finish(w, vecs, norb, nelec, nroots)

    def trans_rdm12_rows(self, bra, kets, norb, nelec):
        """One bra against all ``kets`` in one pass: ``(ovlp (K,), dm1 (K,N,N), dm2 (K,N,N,N,N))``.  The host arrays are
        uploaded once and remembered by identity and content, so the next training state does not upload the old vectors
        again, and a vector changed in place since its upload is uploaded anew."""
        nelec = _nelec(nelec)
        kets = list(kets)
        if not kets:
            raise EvcontHipError("DeviceFCI.trans_rdm12_rows: no kets")
        lib, dta, dtb, na, nb, grant = self._setup(norb, nelec)
        dev = self._dev()
        dbra = self._upload(bra, na, nb, cache=True)
        dkets = [self._upload(k, na, nb, cache=True) for k in kets]
        K = len(dkets)
        ovlp = torch.empty(K, dtype=F64, device=dev)
        dm1 = torch.empty((K, norb, norb), dtype=F64, device=dev)
        dm2 = torch.empty((K, norb, norb, norb, norb), dtype=F64, device=dev)
        ptrs = (C.c_void_p * K)(*[t.data_ptr() for t in dkets])
        check(lib.evc_fci_trdm_rows(norb, na, nb, dta.data_ptr(), dtb.data_ptr(), dbra.data_ptr(), ptrs, K,
                                    ovlp.data_ptr(), dm1.data_ptr(), dm2.data_ptr(), self._ws.data_ptr(), grant,
                                    self._stream()), "evc_fci_trdm_rows")
        return ovlp.cpu().numpy(), dm1.cpu().numpy(), dm2.cpu().numpy()

    def trans_rdm12_rows_packed(self, bra, kets, norb, nelec, layout, out_rows: torch.Tensor):
        """``trans_rdm12_rows`` with the two-body results left on the device, in the layout the evaluator streams
        (``evc_fci_trdm_rows_packed``): row ``i`` of ``out_rows``, a ``(K, ld)`` float64 device view into the caller's
        matrix, receives ``<bra|.|kets[i]>`` in ``layout`` ("pack2" / "sym8", or the ``_lib.LAYOUT_*`` integer), its
        columns beyond the layout's as zeros.  Returns ``(ovlp (K,), dm1 (K,N,N))`` as numpy.  Vectors are uploaded by
        the rules of ``trans_rdm12_rows``; device tensors are used as they are.  A view whose rows are wider apart than
        ``ld`` is filled through a contiguous ``(K, ld)`` device buffer, so that nothing between its rows is written."""
        nelec = _nelec(nelec)
        kets = list(kets)
        if not kets:
            raise EvcontHipError("DeviceFCI.trans_rdm12_rows_packed: no kets")
        lay = {"pack2": _lib.LAYOUT_PACK2, "sym8": _lib.LAYOUT_SYM8}.get(layout, layout)
        if lay not in (_lib.LAYOUT_PACK2, _lib.LAYOUT_SYM8):
            raise EvcontHipError(f"DeviceFCI.trans_rdm12_rows_packed: layout={layout!r}, expected 'pack2' or 'sym8'")
        lib, dta, dtb, na, nb, grant = self._setup(norb, nelec)
        dev = self._dev()
        K = len(kets)
        on_dev = torch.is_tensor(out_rows) and out_rows.device.type == dev.type and dev.index in (None, out_rows.device.index)
        if not (on_dev and out_rows.dtype == F64 and out_rows.dim() == 2 and out_rows.shape[0] == K
                and out_rows.stride(1) == 1):
            raise EvcontHipError(f"DeviceFCI.trans_rdm12_rows_packed: out_rows must be a ({K}, ld) float64 view with "
                                 f"unit column stride on {dev}")
        ld = int(out_rows.shape[1])
        direct = K == 1 or int(out_rows.stride(0)) == ld
        target = out_rows if direct else torch.empty((K, ld), dtype=F64, device=dev)
        # the scratch slot of the packed call on top of what the dense call is granted
        slot = (lib.evc_fci_rows_packed_workspace_bytes(norb, na, nb, 0) - lib.evc_fci_workspace_bytes(norb, na, nb, 0))
        if slot <= 0:
            check(-1, "evc_fci_rows_packed_workspace_bytes")
        if self._ws.numel() < grant + slot:
            self._ws = None
            self._ws = torch.empty(grant + slot, dtype=torch.uint8, device=dev)
        dbra = self._upload(bra, na, nb, cache=True)
        dkets = [self._upload(k, na, nb, cache=True) for k in kets]
        ovlp = torch.empty(K, dtype=F64, device=dev)
        dm1 = torch.empty((K, norb, norb), dtype=F64, device=dev)
        ptrs = (C.c_void_p * K)(*[t.data_ptr() for t in dkets])
        check(lib.evc_fci_trdm_rows_packed(norb, na, nb, dta.data_ptr(), dtb.data_ptr(), dbra.data_ptr(), ptrs, K,
                                           ovlp.data_ptr(), dm1.data_ptr(), lay, target.data_ptr(), ld,
                                           self._ws.data_ptr(), grant + slot, self._stream()), "evc_fci_trdm_rows_packed")
        if not direct:
            out_rows.copy_(target)
        return ovlp.cpu().numpy(), dm1.cpu().numpy()

    def trans_rdm12(self, cibra, ciket, norb, nelec):
        nelec = _nelec(nelec)
        lib, dta, dtb, na, nb, grant = self._setup(norb, nelec)
        dev = self._dev()
        dbra = self._upload(cibra, na, nb, cache=False)
        dket = dbra if ciket is cibra else self._upload(ciket, na, nb, cache=False)
        ovlp = torch.empty(1, dtype=F64, device=dev)
        dm1 = torch.empty((norb, norb), dtype=F64, device=dev)
        dm2 = torch.empty((norb, norb, norb, norb), dtype=F64, device=dev)
        ptrs = (C.c_void_p * 1)(dket.data_ptr())
        check(lib.evc_fci_trdm_rows(norb, na, nb, dta.data_ptr(), dtb.data_ptr(), dbra.data_ptr(), ptrs, 1,
                                    ovlp.data_ptr(), dm1.data_ptr(), dm2.data_ptr(), self._ws.data_ptr(), grant,
                                    self._stream()), "evc_fci_trdm_rows")
        return dm1.cpu().numpy(), dm2.cpu().numpy()

    def make_rdm12(self, ci, norb, nelec):
        return self.trans_rdm12(ci, ci, norb, nelec)

    def transform_ci(self, ci, nelec, u):
        """The CI vector in the orbitals ``new_q = sum_p old_p u[p, q]`` (``fci_small.transform_ci``; ``u`` square, or a
        pair ``(u_a, u_b)``), numpy ``(na, nb)``: the minors of ``u`` and the two products ``T_a^T c T_b`` on the device
        (``csrc/fci_rotate.hip``).  ``workspace_bytes`` bounds the workspace of this call as it does the others'; the
        result has the same bits for every accepted value.  Without it the workspace keeps both matrices of minors
        resident where that takes at most ``ROTATE_RESIDENT_BYTES`` (up to about (14, (6, 6))) and is the least one
        beyond (7 MB instead of 2.7 GB at (16, (8, 8)))."""
        out, na, nb = self._rotate(ci, _nelec(nelec), u)
        return out.cpu().numpy().reshape(na, nb)

    def _rotate(self, ci, nelec, u):
        """``transform_ci`` with the result left on the device: ``(na * nb doubles, na, nb)``."""
        if isinstance(u, (tuple, list)):
            ua, ub = (np.ascontiguousarray(x, dtype=np.float64) for x in u)
        else:
            ua = ub = np.ascontiguousarray(u, dtype=np.float64)
        norb = ua.shape[0]
        if ua.shape != (norb, norb) or ub.shape != (norb, norb):
            raise EvcontHipError(f"DeviceFCI.transform_ci: u of shape {ua.shape} / {ub.shape} (square matrices of one size)")
        lib, _, _, na, nb, _ = self._setup(norb, nelec)
        dsa, dsb = self._masks[(norb, nelec)]
        least = lib.evc_fci_rotate_workspace_bytes(norb, nelec[0], nelec[1], na, nb, 1)
        full = lib.evc_fci_rotate_workspace_bytes(norb, nelec[0], nelec[1], na, nb, 0)
        if least == 0 or full == 0:
            check(-1, "evc_fci_rotate_workspace_bytes")
        # by default both matrices of minors stay resident up to ROTATE_RESIDENT_BYTES, beyond that T is formed and
        # consumed in panels (the same bits, one T formed twice when both spins share it)
        grant = ((full if full <= ROTATE_RESIDENT_BYTES else least) if self.workspace_bytes is None
                 else min(int(self.workspace_bytes), full))
        if grant < least:
            raise EvcontHipError(f"DeviceFCI.transform_ci: workspace_bytes={grant}, but {na} x {nb} strings need at least "
                                 f"{least} bytes ({full} to keep both matrices of minors resident)")
        if self._ws.numel() < grant:
            self._ws = None
            self._ws = torch.empty(grant, dtype=torch.uint8, device=self._dev())
        dc = self._upload(ci, na, nb, cache=False)
        out = torch.empty(na * nb, dtype=F64, device=dc.device)
        check(lib.evc_fci_rotate(norb, nelec[0], nelec[1], na, nb, dsa.data_ptr(), dsb.data_ptr(), ua.ctypes.data,
                                 ub.ctypes.data, dc.data_ptr(), out.data_ptr(), self._ws.data_ptr(), grant,
                                 self._stream()), "evc_fci_rotate")
        return out, na, nb

    def transform_ci_block(self, cis, nelec, u):
        """``transform_ci`` of several vectors under one ``u`` (or pair): a list of numpy ``(na, nb)`` arrays, each with
        the bits ``transform_ci`` gives on it.  One ``evc_fci_rotate_block`` call: the minors of ``u`` are formed once."""
        outs, na, nb = self._rotate_block(cis, _nelec(nelec), u)
        return [o.cpu().numpy().reshape(na, nb) for o in outs]

    def _rotate_block(self, cis, nelec, u):
        """``transform_ci_block`` with the results left on the device: ``([na * nb doubles] per vector, na, nb)``."""
        cis = list(cis)
        if not cis:
            raise EvcontHipError("DeviceFCI.transform_ci_block: no vectors")
        if isinstance(u, (tuple, list)):
            ua, ub = (np.ascontiguousarray(x, dtype=np.float64) for x in u)
        else:
            ua = ub = np.ascontiguousarray(u, dtype=np.float64)
        norb, nvec = ua.shape[0], len(cis)
        if ua.shape != (norb, norb) or ub.shape != (norb, norb):
            raise EvcontHipError(f"DeviceFCI.transform_ci_block: u of shape {ua.shape} / {ub.shape} (square matrices of "
                                 "one size)")
        lib, _, _, na, nb, _ = self._setup(norb, nelec)
        dsa, dsb = self._masks[(norb, nelec)]
        least = lib.evc_fci_rotate_block_workspace_bytes(norb, nelec[0], nelec[1], na, nb, nvec, 1)
        full = lib.evc_fci_rotate_block_workspace_bytes(norb, nelec[0], nelec[1], na, nb, nvec, 0)
        if least == 0 or full == 0:
            check(-1, "evc_fci_rotate_block_workspace_bytes")
        # the rule of _rotate, with one intermediate per vector
        grant = ((full if full <= ROTATE_RESIDENT_BYTES else least) if self.workspace_bytes is None
                 else min(int(self.workspace_bytes), full))
        if grant < least:
            raise EvcontHipError(f"DeviceFCI.transform_ci_block: workspace_bytes={grant}, but {nvec} vectors of {na} x {nb} "
                                 f"strings need at least {least} bytes ({full} to keep both matrices of minors resident)")
        if self._ws.numel() < grant:
            self._ws = None
            self._ws = torch.empty(grant, dtype=torch.uint8, device=self._dev())
        dcs = [self._upload(ci, na, nb, cache=False) for ci in cis]
        outs = [torch.empty(na * nb, dtype=F64, device=self._dev()) for _ in cis]
        cp = (C.c_void_p * nvec)(*[t.data_ptr() for t in dcs])
        op = (C.c_void_p * nvec)(*[t.data_ptr() for t in outs])
        check(lib.evc_fci_rotate_block(norb, nelec[0], nelec[1], na, nb, dsa.data_ptr(), dsb.data_ptr(), ua.ctypes.data,
                                       ub.ctypes.data, nvec, cp, op, self._ws.data_ptr(), grant, self._stream()),
              "evc_fci_rotate_block")
        return outs, na, nb

    def _block_grant(self, lib, norb, na, nb, nbras):
        """``(bras per evc_fci_trdm_rows_block call, workspace bytes)``: all ``nbras`` in one call with everything
        resident by default; under ``workspace_bytes`` as many bras per call as its least workspace allows (one bra
        always fits: ``_setup`` checked that), so that the bound on the workspace holds here as in every other call."""
        full = lib.evc_fci_rows_block_workspace_bytes(norb, na, nb, nbras, 0)
        if full == 0:
            check(-1, "evc_fci_rows_block_workspace_bytes")
        if self.workspace_bytes is None:
            return nbras, full
        cap = int(self.workspace_bytes)
        per = nbras
        while per > 1 and lib.evc_fci_rows_block_workspace_bytes(norb, na, nb, per, 1) > cap:
            per -= 1
        return per, min(cap, lib.evc_fci_rows_block_workspace_bytes(norb, na, nb, per, 0))

    def cas_trans_rdm12_block(self, bras, kets, layout=None, out_rows: Optional[torch.Tensor] = None,
                              triangular: bool = False):
        """``cas_trans_rdm12_rows`` for several bras that share their orbitals (the roots of one geometry; the statement
        is ``cas_small.trans_rdm12_block``), with a leading bra axis: ``(ovlp (R,K), dm1 (R,K,N,N), dm2 (R,K,N,N,N,N))``
        without a layout; with one, ``out_rows`` is a contiguous ``(R K, ld)`` float64 device tensor, bra-major, and
        ``(ovlp, dm1)`` is returned.  Row ``(r, k)`` has the bits of ``cas_trans_rdm12_rows(bras[r], kets)`` row ``k``.

        ``triangular=True`` is the form of a training-set append: the last ``R`` kets must be the bras themselves (by
        identity, ``ValueError`` otherwise) and bra ``r`` is taken against ``kets[:K - R + r + 1]`` only.  The results are
        ragged: lists of ``R`` arrays ``(K - R + r + 1, ...)``; with a layout ``out_rows`` is one contiguous
        ``(sum_r (K - R + r + 1), ld)`` tensor, bra after bra -- the row order of ``resident.ResidentTRDMs`` for the
        states ``T ... T + R - 1``.  Every row has the bits of the rectangular call's row ``(r, k)``.

        The pair intermediates depend on the two orbital sets alone: they are formed once per group of consecutive kets
        that share a ``U``, the group's kets are rotated by one ``evc_fci_rotate_block`` call and scaled by ``fac`` on the
        device, and ``A_a / B_a / Qc`` are uploaded once for all bras.  One ``evc_fci_trdm_rows_block`` call takes all
        bras against the rotated kets (the ket-side excitations of a determinant chunk formed once for all of them),
        then per bra one ``evc_cas_expand_rows`` call on the prefix it sees.  ``CASState.ci`` may be a float64 tensor
        on the solver's device: the rotation and the bra side then read it as it is.  A pair beyond the conditioning
        guard raises ``ValueError`` before anything is launched."""
        from . import cas_small
        bras, kets = list(bras), list(kets)
        if not bras or not kets:
            raise EvcontHipError("DeviceFCI.cas_trans_rdm12_block: no bras or no kets")
        cas_small.check_block("DeviceFCI.cas_trans_rdm12_block", bras, kets)
        bra0 = bras[0]
        R, K, n, ncas, nelec = len(bras), len(kets), int(bra0.U.shape[0]), int(bra0.ncas), _nelec(bra0.nelecas)
        if triangular:
            if K < R or any(kets[K - R + r] is not bras[r] for r in range(R)):
                raise ValueError(f"DeviceFCI.cas_trans_rdm12_block: triangular=True takes kets whose last {R} entries are "
                                 "the bras themselves, in order")
            counts = [K - R + r + 1 for r in range(R)]
        else:
            counts = [K] * R
        offs = [sum(counts[:r]) for r in range(R)]
        total = sum(counts)
        lay = {None: _lib.LAYOUT_FULL6, "pack2": _lib.LAYOUT_PACK2, "sym8": _lib.LAYOUT_SYM8}.get(layout, layout)
        if lay not in (_lib.LAYOUT_FULL6, _lib.LAYOUT_PACK2, _lib.LAYOUT_SYM8):
            raise EvcontHipError(f"DeviceFCI.cas_trans_rdm12_block: layout={layout!r}, expected None, 'pack2' or 'sym8'")
        groups = cas_small.ket_groups(kets)
        for ket in kets:
            cas_small._same_shape(bra0, ket)
        inter = [cas_small.pair_intermediates(bra0, kets[first], f"(bras, ket {first})") for first, _ in groups]
        lib, dta, dtb, na, nb, grant = self._setup(ncas, nelec)
        dev = self._dev()
        if lay != _lib.LAYOUT_FULL6:
            rows_all = out_rows
            on_dev = (torch.is_tensor(rows_all) and rows_all.device.type == dev.type
                      and dev.index in (None, rows_all.device.index))
            if not (on_dev and rows_all.dtype == F64 and rows_all.dim() == 2 and rows_all.shape[0] == total
                    and rows_all.stride(1) == 1 and (total == 1 or rows_all.stride(0) == rows_all.shape[1])):
                raise EvcontHipError(f"DeviceFCI.cas_trans_rdm12_block: out_rows must be a contiguous ({total}, ld) float64 "
                                     f"tensor on {dev}")
        else:
            # (one tensor per bra: evc_cas_expand_rows wants 16-byte aligned rows, which n^4 doubles do not keep)
            rows_all = [torch.empty((counts[r], n ** 4), dtype=F64, device=dev) for r in range(R)]
        dkets = []
        for (first, count), (fac, s_eff, _, _, _) in zip(groups, inter):
            rotated, _, _ = self._rotate_block([k.ci for k in kets[first:first + count]], nelec,
                                               np.ascontiguousarray(s_eff.T))
            dkets.extend(t.mul_(fac) for t in rotated)
        lib, dta, dtb, na, nb, grant = self._setup(ncas, nelec)      # (the rotation may have replaced the workspace)
        per_call, grant = self._block_grant(lib, ncas, na, nb, R)
        if self._ws.numel() < grant:
            self._ws = None
            self._ws = torch.empty(grant, dtype=torch.uint8, device=dev)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        per_ket = [x for (_, count), x in zip(groups, inter) for _ in range(count)]
        A_act = up(np.stack([x[2] for x in per_ket]))                  # (K, n, ncas), the same for every bra
        B_act = up(np.stack([x[3] for x in per_ket]))
        Qc = up(np.stack([x[4] for x in per_ket])) if bra0.ncore else None
        need = lib.evc_cas_expand_workspace_bytes(n, ncas, K)
        if need == 0:
            check(-1, "evc_cas_expand_workspace_bytes")
        if self._cas_ws is None or self._cas_ws.numel() < need:
            self._cas_ws = None
            self._cas_ws = torch.empty(need, dtype=torch.uint8, device=dev)
        # the active-space results of all bras, ragged and consecutive: bra r holds rows offs[r] ... + counts[r] - 1
        ovlp = torch.empty(total, dtype=F64, device=dev)
        d1 = torch.empty((total, ncas * ncas), dtype=F64, device=dev)
        d2 = torch.empty((total, ncas ** 4), dtype=F64, device=dev)
        dm1 = [torch.empty((counts[r], n, n), dtype=F64, device=dev) for r in range(R)]
        dbras = [self._upload(bra.ci, na, nb, cache=False) for bra in bras]
        for r0 in range(0, R, per_call):
            nr = min(per_call, R - r0)
            nk = counts[r0 + nr - 1]
            bp = (C.c_void_p * nr)(*[t.data_ptr() for t in dbras[r0:r0 + nr]])
            kp = (C.c_void_p * nk)(*[t.data_ptr() for t in dkets[:nk]])
            cnt = (C.c_int * nr)(*counts[r0:r0 + nr])
            check(lib.evc_fci_trdm_rows_block(ncas, na, nb, dta.data_ptr(), dtb.data_ptr(), bp, nr, kp, cnt,
                                              ovlp[offs[r0]:].data_ptr(), d1[offs[r0]:].data_ptr(),
                                              d2[offs[r0]:].data_ptr(), self._ws.data_ptr(), grant, self._stream()),
                  "evc_fci_trdm_rows_block")
        # (evc_cas_expand_rows wants 16-byte aligned inputs and the block call's rows are consecutive, so a bra whose
        # rows start at an odd double gets a copy: on the append path of every odd T, (1 + ncas^2 + ncas^4) doubles per
        # row, small beside the n^4 the expansion writes)
        aligned = lambda t: t if t.data_ptr() % 16 == 0 else t.clone()
        for r in range(R):
            o, c = offs[r], counts[r]
            rows = rows_all[r] if lay == _lib.LAYOUT_FULL6 else rows_all[o:o + c]
            so, s1, s2 = aligned(ovlp[o:o + c]), aligned(d1[o:o + c]), aligned(d2[o:o + c])
            check(lib.evc_cas_expand_rows(n, ncas, c, A_act.data_ptr(), B_act.data_ptr(),
                                          None if Qc is None else Qc.data_ptr(), so.data_ptr(), s1.data_ptr(),
                                          s2.data_ptr(), dm1[r].data_ptr(), lay, rows.data_ptr(), int(rows.shape[1]),
                                          self._cas_ws.data_ptr(), need, self._stream()), "evc_cas_expand_rows")
        # (each bra's results straight into their place on the host: no stacked copy on the device)
        if triangular:
            h_ovlp = [ovlp[offs[r]:offs[r] + counts[r]].cpu().numpy() for r in range(R)]
            h_dm1 = [dm1[r].cpu().numpy() for r in range(R)]
            if lay != _lib.LAYOUT_FULL6:
                return h_ovlp, h_dm1
            return h_ovlp, h_dm1, [rows_all[r].cpu().numpy().reshape(counts[r], n, n, n, n) for r in range(R)]
        h_ovlp, h_dm1 = np.empty((R, K)), np.empty((R, K, n, n))
        for r in range(R):
            torch.from_numpy(h_ovlp[r]).copy_(ovlp[offs[r]:offs[r] + K])
            torch.from_numpy(h_dm1[r]).copy_(dm1[r])
        if lay != _lib.LAYOUT_FULL6:
            return h_ovlp, h_dm1
        h_dm2 = np.empty((R, K, n ** 4))
        for r in range(R):
            torch.from_numpy(h_dm2[r]).copy_(rows_all[r])
        return h_ovlp, h_dm1, h_dm2.reshape(R, K, n, n, n, n)

    def cas_trans_rdm12_rows(self, bra, kets, layout=None, out_rows: Optional[torch.Tensor] = None):
        """Overlaps and transition RDMs, in the OAO basis, of one CAS state against ``kets`` whose orbitals differ from
        its own (``cas_small.CASState``; the statement is ``cas_small.trans_rdm12_rows``): the ``R = 1`` case of
        ``cas_trans_rdm12_block``.  The pair intermediates on the host (m x m and N x m matrices, once per group of
        consecutive kets that share their orbitals), the kets rotated with ``u = s_eff^T`` and scaled by ``fac`` on the
        device, one active-space row call for all kets, and one ``evc_cas_expand_rows`` call (``csrc/cas_expand.hip``)
        that expands its results to N orbitals with the core terms.  Nothing but the overlaps, ``dm1`` and, without a
        layout, ``dm2`` comes back to the host.

        ``layout=None`` returns ``(ovlp (K,), dm1 (K,N,N), dm2 (K,N,N,N,N))`` as numpy.  With ``layout`` ("pack2" /
        "sym8") the two-body rows go into ``out_rows``, a contiguous ``(K, ld)`` float64 device tensor, in the format of
        ``trans_rdm12_rows_packed``, and ``(ovlp, dm1)`` is returned.  A pair beyond the conditioning guard raises
        ``ValueError`` before anything is launched."""
        kets = list(kets)
        if not kets:
            raise EvcontHipError("DeviceFCI.cas_trans_rdm12_rows: no kets")
        return tuple(x[0] for x in self.cas_trans_rdm12_block([bra], kets, layout=layout, out_rows=out_rows))

    def energy(self, h1, h2, ci, norb, nelec) -> float:
        dm1, dm2 = self.make_rdm12(ci, norb, nelec)
        return float(np.sum(np.asarray(h1) * dm1.T) + 0.5 * np.sum(np.asarray(h2).reshape(dm2.shape) * dm2))
