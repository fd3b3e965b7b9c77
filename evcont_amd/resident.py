"""Training data that grows on the device: the two-body t-RDM rows of a new training state are written by the full-CI row
call straight into the ``(P, ld)`` matrix the evaluator streams (``fci_device.DeviceFCI.trans_rdm12_rows_packed``,
``csrc/fci_pack.hip``), in its layout ("sym8" or "pack2"), and never reach the host.

The matrix has one row per training pair ``a >= b`` at ``p = a(a+1)/2 + b``: the rows of state ``T`` are rows
``T(T+1)/2 ... T(T+1)/2 + T``, behind every row already there, so an append writes ``T + 1`` rows and moves nothing;
the first ``k(k+1)/2`` rows are the training set of the first ``k`` states (``trdm_io.prefix``).  Only the overlap row
and the one-body rows of a new state come back to the host, where ``overlap (T,T)`` and ``one_rdm (T,T,N,N)`` stay as
the record.

``ResidentTRDMs`` is the matrix with its capacity; ``ResidentFCI_EVCont_obj`` the ``FCI_EVCont_obj`` on top of it and
``ResidentCAS_EVCont_obj`` the ``CAS_EVCont_obj``: the ``R`` roots of a new geometry are appended by one triangular block
call (``DeviceFCI.cas_trans_rdm12_block(..., triangular=True)``, ``evc_fci_trdm_rows_block``) that writes the rows of all
of them, and the CI vectors of the stored states stay on the device between appends.
The "sym8" form is for the Hermitian continuation with symmetric integrals, like ``compress="sym8"`` everywhere else.
"""
from __future__ import annotations

import inspect
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import EvcontHipError
from .evaluator import DeviceTRDMs, F64, _dev, layout_shape
from .CASCI_EVCont import CAS_EVCont_obj
from .FCI_EVCont import FCI_EVCont_obj

LAYOUTS = {"pack2": _lib.LAYOUT_PACK2, "sym8": _lib.LAYOUT_SYM8}


def pair_row(a: int, b: int) -> int:
    """Row of the training pair ``a >= b``."""
    return a * (a + 1) // 2 + b


def check_keep_ids(keep_ids: Sequence[int], T: int) -> list:
    """``keep_ids`` as a list of ints; ``ValueError`` unless they are strictly increasing and within ``0 ... T - 1``.
    (Any other order needs the bra<->ket partner rows ``(b, a)``, ``a > b``, which a pair layout does not store.)"""
    keep = [int(k) for k in keep_ids]
    if any(k < 0 or k >= T for k in keep):
        raise ValueError(f"prune: keep_ids={keep} outside 0 ... {T - 1}")
    if any(y <= x for x, y in zip(keep, keep[1:])):
        raise ValueError(f"prune: keep_ids={keep} must be strictly increasing (the rows hold the pairs a >= b only)")
    return keep


def prune_row_map(keep_ids: Sequence[int]) -> np.ndarray:
    """Source rows of the pruned matrix: new row ``pair_row(i, j)`` is old row ``pair_row(keep[i], keep[j])``
    (``keep`` strictly increasing) -- ``np.ix_`` slicing of the ``(T,T,...)`` array followed by ``np.tril_indices``."""
    keep = np.asarray(list(keep_ids), dtype=np.int64)
    i, j = np.tril_indices(len(keep))
    a, b = keep[i], keep[j]
    return a * (a + 1) // 2 + b


class ResidentTRDMs:
    """One zero-initialised ``(capacity (capacity + 1) / 2, ld)`` device matrix of two-body rows, with the one-body
    blocks ``(cap, cap, n^2)`` and the overlap ``(cap, cap)`` beside it on the host.  Beyond ``capacity`` states the
    capacity doubles and the rows are copied once, on the device; a row once written is never written again."""

    def __init__(self, n: int, layout: str = "sym8", capacity: int = 16, device=None):
        if layout not in LAYOUTS:
            raise ValueError(f"ResidentTRDMs: layout={layout!r}, expected 'sym8' or 'pack2'")
        if capacity < 1:
            raise ValueError(f"ResidentTRDMs: capacity={capacity}")
        self.n, self.layout, self.layout_id = int(n), layout, LAYOUTS[layout]
        self.device = _dev(device)
        self.cols = layout_shape(self.layout_id, 1, self.n)[1]
        self.ld = (self.cols + 15) // 16 * 16
        self.T = 0
        self.capacity = int(capacity)
        self.two = torch.zeros((pair_row(self.capacity, 0), self.ld), dtype=F64, device=self.device)
        self.one = np.zeros((self.capacity, self.capacity, self.n * self.n))
        self.S = np.zeros((self.capacity, self.capacity))

    # -- the host record ---------------------------------------------------------------------------
    @property
    def overlap(self) -> np.ndarray:
        return np.ascontiguousarray(self.S[:self.T, :self.T])

    @property
    def one_rdm(self) -> np.ndarray:
        return np.ascontiguousarray(self.one[:self.T, :self.T]).reshape(self.T, self.T, self.n, self.n)

    def _reserve(self, T: int) -> None:
        if T <= self.capacity:
            return
        cap = self.capacity
        while cap < T:
            cap *= 2
        two = torch.zeros((pair_row(cap, 0), self.ld), dtype=F64, device=self.device)
        used = pair_row(self.T, 0)
        two[:used].copy_(self.two[:used])          # the one device copy of a growth; views keep the old matrix
        one, S = np.zeros((cap, cap, self.n * self.n)), np.zeros((cap, cap))
        one[:self.T, :self.T], S[:self.T, :self.T] = self.one[:self.T, :self.T], self.S[:self.T, :self.T]
        self.two, self.one, self.S, self.capacity = two, one, S, cap

    # -- growth / pruning --------------------------------------------------------------------------
    def append(self, solver, bra, kets, norb, nelec):
        """State ``T`` from the row call of ``solver`` (``trans_rdm12_rows_packed``): ``kets`` are the ``T`` stored
        vectors followed by ``bra`` itself.  Writes rows ``T(T+1)/2 ... + T`` in place, fills the one-body blocks and
        overlap entries ``[T, i]`` and ``[i, T]`` with the same untransposed matrix (``containers.grow_trdms``) and
        synchronises the stream.  Returns the host ``(ovlp_row (T+1,), one_rows (T+1, N, N))``."""
        kets = list(kets)
        T = self.T
        if len(kets) != T + 1:
            raise ValueError(f"ResidentTRDMs.append: {len(kets)} kets for state {T} (the {T} stored states and the new one)")
        if int(norb) != self.n:
            raise ValueError(f"ResidentTRDMs.append: norb={norb}, the matrix was made for {self.n} orbitals")
        self._reserve(T + 1)
        r0 = pair_row(T, 0)
        with torch.cuda.device(self.device):
            ovlp, one = solver.trans_rdm12_rows_packed(bra, kets, norb, nelec, self.layout, self.two[r0:r0 + T + 1])
            torch.cuda.current_stream(self.device).synchronize()
        ovlp = np.asarray(ovlp, dtype=np.float64)
        one = np.asarray(one, dtype=np.float64)
        flat = one.reshape(T + 1, self.n * self.n)
        self.S[T, :T + 1] = ovlp
        self.S[:T + 1, T] = ovlp
        self.one[T, :T + 1] = flat
        self.one[:T + 1, T] = flat
        self.T = T + 1
        return ovlp, one

    def append_block(self, solver, bras, kets):
        """States ``T ... T + R - 1`` from the triangular block call of ``solver`` (``cas_trans_rdm12_block``): ``bras``
        are ``R`` CAS states of one geometry, ``kets`` the ``T`` stored states followed by the bras themselves.  Capacity
        for ``T + R`` states is reserved before the call (a growth never falls inside a block), then the one call writes
        rows ``T(T+1)/2 ... (T+R)(T+R+1)/2 - 1`` in place: bra ``r`` against ``kets[:T + r + 1]``, bra after bra.  The
        host record is filled as ``R`` appends would fill it and the stream is synchronised.  A call that raises
        leaves ``T``, the record and every view as they were; a growth it needed has then happened already (the
        capacity is larger and ``two`` / ``one`` / ``S`` are the new arrays with the same contents).  Returns the ragged host ``(ovlp, one)`` lists."""
        bras, kets = list(bras), list(kets)
        T, R = self.T, len(bras)
        if R < 1 or len(kets) != T + R:
            raise ValueError(f"ResidentTRDMs.append_block: {len(kets)} kets for {R} new states behind {T} (the {T} stored "
                             "states and the new ones)")
        if int(bras[0].U.shape[0]) != self.n:
            raise ValueError(f"ResidentTRDMs.append_block: states of {bras[0].U.shape[0]} orbitals, the matrix was made "
                             f"for {self.n}")
        self._reserve(T + R)
        r0, r1 = pair_row(T, 0), pair_row(T + R, 0)
        with torch.cuda.device(self.device):
            ovlp, one = solver.cas_trans_rdm12_block(bras, kets, self.layout, self.two[r0:r1], triangular=True)
            torch.cuda.current_stream(self.device).synchronize()
        for r in range(R):
            t = T + r
            row = np.asarray(ovlp[r], dtype=np.float64)
            flat = np.asarray(one[r], dtype=np.float64).reshape(t + 1, self.n * self.n)
            self.S[t, :t + 1] = row
            self.S[:t + 1, t] = row
            self.one[t, :t + 1] = flat
            self.one[:t + 1, t] = flat
        self.T = T + R
        return ovlp, one

    def prune(self, keep_ids: Sequence[int]) -> None:
        """Keep the listed states (strictly increasing ids, ``ValueError`` otherwise): rows ``(keep[i], keep[j])`` are
        gathered into a new matrix on the device."""
        keep = check_keep_ids(keep_ids, self.T)
        k = len(keep)
        two = torch.zeros((pair_row(self.capacity, 0), self.ld), dtype=F64, device=self.device)
        if k:
            src = torch.from_numpy(prune_row_map(keep)).to(self.device)
            two[:pair_row(k, 0)] = self.two.index_select(0, src)
        one, S = np.zeros_like(self.one), np.zeros_like(self.S)
        one[:k, :k], S[:k, :k] = self.one[np.ix_(keep, keep)], self.S[np.ix_(keep, keep)]
        self.two, self.one, self.S, self.T = two, one, S, k

    # -- what the evaluator and the checkpoints read --------------------------------------------------
    def view(self) -> DeviceTRDMs:
        """``DeviceTRDMs`` of the current ``T`` states on the rows themselves (no copy of the two-body data), a
        snapshot: later appends write behind its rows, a capacity growth and a prune make a new matrix."""
        if self.T == 0:
            raise ValueError("the container holds no training data yet")
        return DeviceTRDMs.from_padded_rows(self.one_rdm, self.two[:pair_row(self.T, 0)], self.overlap, self.layout_id)

    def rows_host(self) -> np.ndarray:
        """The ``(P, cols)`` matrix on the host; for "pack2" the reference's own two-index ``two_RDM``."""
        return self.two[:pair_row(self.T, 0), :self.cols].cpu().numpy()


class ResidentFCI_EVCont_obj(FCI_EVCont_obj):
    """``FCI_EVCont_obj`` whose two-body t-RDMs exist on the device alone (``ResidentTRDMs``): same constructor plus
    ``layout`` ("sym8" / "pack2"), ``capacity`` and ``device`` (where the rows live: it must be the device of the solver,
    whose row call writes them; ``None`` = the current device); ``cisolver`` must have ``trans_rdm12_rows_packed``
    (``fci_device.DeviceFCI``).  ``overlap``, ``one_rdm``, ``fcivecs``, ``ens``, ``mol_index``, ``ntrain``,
    ``append_to_rdms`` and ``prune_datapoints`` behave as in the host container; ``two_rdm`` is ``None`` while empty and
    raises afterwards: read ``device_trdms()`` (the evaluator's view) or ``rows_host()``.  Every training vector is
    uploaded once, at its append, and the row call gets those device tensors; ``fcivecs`` stays the list of host
    arrays."""

    resident_rows = True     # what active_learning.converge_EVCont_MD asks: the two-body rows are on the device alone

    def __init__(self, cisolver=None, cibasis="canonical", nroots=1, roots_train=None, layout: str = "sym8",
                 capacity: int = 16, device=None):
        if layout not in LAYOUTS:
            raise ValueError(f"ResidentFCI_EVCont_obj: layout={layout!r}, expected 'sym8' or 'pack2'")
        self._res: Optional[ResidentTRDMs] = None
        super().__init__(cisolver=cisolver, cibasis=cibasis, nroots=nroots, roots_train=roots_train)
        if not hasattr(self.cisolver, "trans_rdm12_rows_packed"):
            raise EvcontHipError("ResidentFCI_EVCont_obj needs a solver with trans_rdm12_rows_packed "
                                 "(fci_device.DeviceFCI); FCI_EVCont_obj is the container for host solvers")
        self.layout, self.capacity, self._device_arg = layout, int(capacity), device
        self._dvecs = []         # the training vectors on the device, in the order of fcivecs

    @property
    def two_rdm(self):
        if self._res is None or self._res.T == 0:
            return None
        # (never None once states exist: get_scanner(mol, one, None, S) would silently take the nuclear-only branch)
        raise EvcontHipError("ResidentFCI_EVCont_obj keeps the two-body t-RDMs on the device: use device_trdms() (the "
                             "evaluator's view, e.g. get_scanner(..., device_trdms=)) or rows_host() (the packed rows)")

    @two_rdm.setter
    def two_rdm(self, value):
        if value is not None:
            raise EvcontHipError("ResidentFCI_EVCont_obj: two_rdm cannot be assigned (the rows live on the device)")

    def _append_root(self, fcivec, energy, mindex, n, nelec):
        if np.iscomplexobj(fcivec):
            raise EvcontHipError("ResidentFCI_EVCont_obj: complex CI vectors are not supported")
        if self._res is None:
            self._res = ResidentTRDMs(n, self.layout, self.capacity, self._device_arg)
        dvec = torch.from_numpy(np.ascontiguousarray(fcivec, dtype=np.float64)).to(self._res.device)
        self._res.append(self.cisolver, dvec, self._dvecs + [dvec], n, nelec)
        # the lists grow only once the rows are written: a failed row call leaves the container as it was
        self._dvecs.append(dvec)
        self.fcivecs.append(fcivec)
        self.ens.append(energy)
        self.mol_index.append(mindex)
        self._sync_record()

    def _sync_record(self) -> None:
        """The training set changed: refresh the host record and drop the cached view (nothing of this container is in
        the upload cache of the mol-level API, so that cache is left alone)."""
        self.overlap, self.one_rdm = self._res.overlap, self._res.one_rdm
        self._device, self._device_key = None, None

    def prune_datapoints(self, keep_ids):
        keep = check_keep_ids(keep_ids, self.ntrain)
        if self._res is not None:
            self._res.prune(keep)
            self._sync_record()
        self.fcivecs = [self.fcivecs[i] for i in keep]
        self.ens = [self.ens[i] for i in keep]
        self._dvecs = [self._dvecs[i] for i in keep]

    def device_trdms(self, layout: Optional[str] = None, device=None) -> DeviceTRDMs:
        """The view of the current training set, cached until the next append or prune.  ``layout`` other than the
        container's own is refused (the rows exist in one form only)."""
        if layout is not None and layout != self.layout:
            raise EvcontHipError(f"ResidentFCI_EVCont_obj holds its rows as {self.layout!r}; device_trdms({layout!r}) "
                                 "would need the dense two-body t-RDMs, which are not kept")
        if self._res is None or self._res.T == 0:
            raise ValueError("the container holds no training data yet")
        if device is not None and _dev(device).index not in (None, self._res.device.index):
            raise EvcontHipError(f"ResidentFCI_EVCont_obj: the rows are on {self._res.device}, not on {_dev(device)}")
        if self._device is None:
            self._device = self._res.view()
        return self._device

    def rows_host(self) -> np.ndarray:
        if self._res is None:
            raise ValueError("the container holds no training data yet")
        return self._res.rows_host()


class ResidentCAS_EVCont_obj(CAS_EVCont_obj):
    """``CAS_EVCont_obj`` (built-in route: ``cisolver=DeviceFCI(...)``) whose two-body t-RDMs exist on the device alone
    (``ResidentTRDMs``).  ``layout`` ("sym8" / "pack2"), ``capacity`` and ``device`` as in ``ResidentFCI_EVCont_obj``;
    ``cisolver`` must have the triangular block call (``DeviceFCI.cas_trans_rdm12_block(..., triangular=True)``).

    ``append_to_rdms(mol)`` solves the geometry as the host container does (``cas_small.casci`` / ``casci_roots``),
    uploads each new CI vector once and keeps it, and one triangular block call writes the rows of all ``R`` new states
    behind those already there.  Only overlaps and one-body rows come back.  ``overlap``, ``one_rdm``, ``ens``,
    ``mol_index``, ``cascis`` (the host states, for the record) and ``ntrain`` are as in the host container; ``two_rdm``
    is ``None`` while empty and raises afterwards: read ``device_trdms()`` or ``rows_host()``.  A pair beyond the
    conditioning guard raises before any launch and leaves the container as it was."""

    resident_rows = True
    single_root_loop_only = True   # converge_EVCont_MD takes this container with roots_train == [0] alone

    def __init__(self, ncas, neleca, cisolver=None, nroots=1, roots_train=None, layout: str = "sym8",
                 capacity: int = 16, device=None):
        if layout not in LAYOUTS:
            raise ValueError(f"ResidentCAS_EVCont_obj: layout={layout!r}, expected 'sym8' or 'pack2'")
        self._res: Optional[ResidentTRDMs] = None
        super().__init__(ncas, neleca, cisolver=cisolver, nroots=nroots, roots_train=roots_train)
        call = getattr(self.cisolver, "cas_trans_rdm12_block", None)
        if call is None or "triangular" not in inspect.signature(call).parameters:
            raise EvcontHipError("ResidentCAS_EVCont_obj needs a solver with cas_trans_rdm12_block(..., triangular=True) "
                                 "(fci_device.DeviceFCI); CAS_EVCont_obj is the container for host solvers")
        self.layout, self.capacity, self._device_arg = layout, int(capacity), device
        self._dstates = []       # the stored states with their CI vectors on the device, in the order of cascis

    @property
    def two_rdm(self):
        if self._res is None or self._res.T == 0:
            return None
        raise EvcontHipError("ResidentCAS_EVCont_obj keeps the two-body t-RDMs on the device: use device_trdms() (the "
                             "evaluator's view, e.g. get_scanner(..., device_trdms=)) or rows_host() (the packed rows)")

    @two_rdm.setter
    def two_rdm(self, value):
        if value is not None:
            raise EvcontHipError("ResidentCAS_EVCont_obj: two_rdm cannot be assigned (the rows live on the device)")

    def append_to_rdms(self, mol):
        from . import cas_small
        mindex = 0 if len(self.mol_index) == 0 else max(self.mol_index) + 1
        if self.roots_train == [0]:
            states = [cas_small.casci(mol, self.ncas, self.neleca, self.cisolver)]
        else:
            roots = cas_small.casci_roots(mol, self.ncas, self.neleca, self.cisolver, max(self.roots_train) + 1)
            states = [roots[k] for k in self.roots_train]
        n = int(states[0].U.shape[0])
        if self._res is None:
            self._res = ResidentTRDMs(n, self.layout, self.capacity, self._device_arg)
        dev = self._res.device
        bras = []
        for st in states:
            if np.iscomplexobj(st.ci):
                raise EvcontHipError("ResidentCAS_EVCont_obj: complex CI vectors are not supported")
            dci = torch.from_numpy(np.ascontiguousarray(st.ci, dtype=np.float64)).to(dev)     # the one upload
            bras.append(cas_small.CASState(U=st.U, ncore=st.ncore, ncas=st.ncas, nelecas=st.nelecas, ci=dci,
                                           e_tot=st.e_tot))
        # (a pair beyond the conditioning guard raises here, before any launch: the container is then as it was)
        self._res.append_block(self.cisolver, bras, self._dstates + bras)
        self._dstates.extend(bras)
        for st in states:
            self.cascis.append(st)
            self.ens.append(st.e_tot)
            self.mol_index.append(mindex)
        self._sync_record()

    def _sync_record(self) -> None:
        self.overlap, self.one_rdm = self._res.overlap, self._res.one_rdm
        self._device, self._device_key = None, None

    def prune_datapoints(self, keep_ids):
        keep = check_keep_ids(keep_ids, self.ntrain)
        if self._res is not None:
            self._res.prune(keep)
            self._sync_record()
        self.cascis = [self.cascis[i] for i in keep]
        self._dstates = [self._dstates[i] for i in keep]
        self.ens = [self.ens[i] for i in keep]
        self.mol_index = [self.mol_index[i] for i in keep]

    def device_trdms(self, layout: Optional[str] = None, device=None) -> DeviceTRDMs:
        """The view of the current training set, cached until the next append or prune.  ``layout`` other than the
        container's own is refused (the rows exist in one form only)."""
        if layout is not None and layout != self.layout:
            raise EvcontHipError(f"ResidentCAS_EVCont_obj holds its rows as {self.layout!r}; device_trdms({layout!r}) "
                                 "would need the dense two-body t-RDMs, which are not kept")
        if self._res is None or self._res.T == 0:
            raise ValueError("the container holds no training data yet")
        if device is not None and _dev(device).index not in (None, self._res.device.index):
            raise EvcontHipError(f"ResidentCAS_EVCont_obj: the rows are on {self._res.device}, not on {_dev(device)}")
        if self._device is None:
            self._device = self._res.view()
        return self._device

    def rows_host(self) -> np.ndarray:
        if self._res is None:
            raise ValueError("the container holds no training data yet")
        return self._res.rows_host()
