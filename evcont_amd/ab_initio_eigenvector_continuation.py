"""Device-backed mirror of ``evcont/ab_initio_eigenvector_continuation.py``."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import cache, ops
from .electron_integral_utils import (  # re-exported, scripts import them from here (04_Zundel...py:13-15)
    get_basis,
    get_integrals,
    compress_electron_exchange_symmetry,
)
from .evaluator import DeviceTRDMs, DeviceAO, ContinuationEvaluator, _dev, _eig_nonhermitian, _select
from .integrals import ao_arrays, energy_nuc, is_array_mol


# How the resident copy of the training data is stored by the mol-level entry points (``*_OAO``,
# ``get_energy_with_grad``, ``MD_utils.get_scanner``):
#   "auto" (default)  8-fold compressed (``evaluator.DeviceTRDMs.compress_sym8_``: 3.7x fewer streamed bytes and the
#                     symmetric AO-side pipeline, the configuration ``bench.py`` measures) whenever that is exact AND
#                     indistinguishable from the reference for the caller: ``hermitian=True``, no predicted RDMs asked
#                     for, a training set whose bra<->ket partner blocks compress alike (checked on the device when the
#                     compressed copy of a training set held as (T,T,...) is made, ``DeviceTRDMs.compress_sym8_``;
#                     ``_trdms_auto`` then keeps the caller's layout for it), and AO integrals with the index
#                     symmetries of real two-electron integrals -- a PySCF ``Mole`` has them by construction, an
#                     array-level molecule is checked completely at the first call for a training set
#                     (``integrals_have_symmetry``) and, unless it declares ``integral_symmetry``, by a random sample on
#                     every later call (``spot_check_integral_symmetry``).  Everything else (``hermitian=False``,
#                     ``return_density_matrices=True``, ``predicted_two_rdm`` of a scanner, general tensors) runs on the
#                     layout the caller passed, from a second resident copy made on first use;
#   None / "none"     always the layout the caller passed;
#   "sym8"            always compressed (``predicted_two_rdm`` then is the 8-fold symmetrised 2-RDM; integrals without
#                     the symmetries raise ``EvcontHipError``).
def _mode_from_env():
    m = os.environ.get("EVCONT_AMD_COMPRESS", "auto").strip().lower()
    if m in ("", "none", "0", "off"):
        return None
    if m not in ("auto", "sym8"):
        raise ValueError(f"EVCONT_AMD_COMPRESS={m!r} (known: auto, sym8, none)")
    return m


_COMPRESS = _mode_from_env()
_auto_decisions = {}   # training-set key -> bool: its first geometry's integrals had the symmetries (False as well once
                       # the compressed layout refused the training set itself, _trdms_auto)


def set_trdm_compression(mode) -> None:
    """``"auto"`` (default), ``"sym8"`` or ``None``; applies to training data uploaded from now on."""
    global _COMPRESS
    if mode not in (None, "sym8", "auto"):
        raise ValueError(f"unknown t-RDM compression {mode!r} (known: None, 'sym8', 'auto')")
    _COMPRESS = mode


def get_trdm_compression():
    return _COMPRESS


def integrals_have_symmetry(mol_or_ao, tol: float = 1.0e-9) -> bool:
    """Whether the AO integrals of a molecule have the index symmetries the compressed layout relies on (``eri``
    8-fold, ``eri_ip1[x,p,q,r,s] = eri_ip1[x,p,q,s,r]``).  A PySCF ``Mole`` (anything with ``intor``): yes, libcint
    integrals have them.  Array-level molecule: what it declares (``integral_symmetry``), else checked numerically (arrays handed over packed -- s4 / s2kl -- carry
    the symmetries of their packing; the pair exchange of a packed ``eri`` is still checked)."""
    declared = getattr(mol_or_ao, "integral_symmetry", None)
    if declared is not None:
        return bool(declared)
    if not is_array_mol(mol_or_ao):
        return True
    from .evaluator import check_integral_symmetry
    from ._lib import EvcontHipError
    n = int(np.asarray(mol_or_ao.S).shape[0])
    ip1 = getattr(mol_or_ao, "eri_ip1", None)
    if ip1 is not None and np.asarray(ip1).size == 0:
        ip1 = None
    try:
        check_integral_symmetry(np.asarray(mol_or_ao.eri), None if ip1 is None else np.asarray(ip1), n, tol)
    except EvcontHipError:
        return False
    return True


def _integrals_fit_this_call(mol, need_grad: bool) -> bool:
    """Per-call part of the "auto" decision: a molecule that declares ``integral_symmetry`` is taken at its word, a
    PySCF ``Mole`` has the symmetries, any other array-level molecule is spot-checked (``eri_ip1`` only when the call
    reads it)."""
    declared = getattr(mol, "integral_symmetry", None)
    if declared is not None:
        return bool(declared)
    if not is_array_mol(mol):
        return True
    from .evaluator import _CHECK_SYM, spot_check_integral_symmetry
    from ._lib import EvcontHipError
    if _CHECK_SYM == "0":
        return True
    ip1 = getattr(mol, "eri_ip1", None) if need_grad else None
    try:
        spot_check_integral_symmetry(mol.eri, ip1, int(np.asarray(mol.S).shape[0]))
    except EvcontHipError:
        return False
    return True


def resolve_compression(mode, one_RDM, two_RDM, S, mol, hermitian=True, want_rdms=False, n=None, need_grad=True):
    """The storage (``None`` or ``"sym8"``) one call of a mol-level entry point uses under ``mode``
    (``"default"`` = ``get_trdm_compression()``).  ``need_grad=False``: the call reads no ``eri_ip1``."""
    if mode == "default":
        mode = _COMPRESS
    if mode is None:
        return None
    if not hermitian:
        return None              # the eig branch works on the subspace matrix of the caller's layout
    if mode == "sym8":
        return "sym8"
    if want_rdms:
        return None              # the reference returns the un-symmetrised predicted 2-RDM
    key = cache.key_of(one_RDM, two_RDM, S, ("auto",))
    ok = _auto_decisions.get(key)
    if ok is None:
        ok = integrals_have_symmetry(mol)
        if len(_auto_decisions) > 64:
            _auto_decisions.clear()
        _auto_decisions[key] = ok
    # (the decision above was made on the first molecule; every later one must have the symmetries as well)
    return "sym8" if ok and _integrals_fit_this_call(mol, need_grad) else None


def _trdms(one_RDM, two_RDM, S, compress=None) -> DeviceTRDMs:
    key = cache.key_of(one_RDM, two_RDM, S, ("trdms", compress))
    arrays = (one_RDM, two_RDM, S)
    t = cache.get(key, arrays)       # (block checksums of the host arrays are verified: cache.py)
    if t is None:
        t = cache.put(key, DeviceTRDMs(one_RDM, two_RDM, S, _dev(), compress=compress), arrays)
    return t


def _trdms_auto(one_RDM, two_RDM, S, compress) -> DeviceTRDMs:
    """``_trdms`` for a storage that mode "auto" chose: a training set the compressed layout cannot represent (its
    bra<->ket partner blocks differ, ``Sym8NotExact``) is kept in the caller's layout instead, and "auto" remembers
    that for the training set.  (An explicit "sym8" raises.)"""
    from .evaluator import Sym8NotExact
    if compress == "sym8":
        try:
            return _trdms(one_RDM, two_RDM, S, "sym8")
        except Sym8NotExact:
            _auto_decisions[cache.key_of(one_RDM, two_RDM, S, ("auto",))] = False
            compress = None
    return _trdms(one_RDM, two_RDM, S, compress)


def _resident_trdms(one_RDM, two_RDM, S, compress, auto=None) -> DeviceTRDMs:
    """The resident training data in the storage ``compress`` (None or "sym8", what ``resolve_compression`` returned
    for this call), verified against the host arrays or uploaded again.  ``auto``: the storage was chosen by mode
    "auto" (``_trdms_auto``); None: whether the current mode is "auto"."""
    if auto is None:
        auto = _COMPRESS == "auto"
    return _trdms_auto(one_RDM, two_RDM, S, compress) if auto else _trdms(one_RDM, two_RDM, S, compress)


def _evaluator(one_RDM, two_RDM, S, natm: int, compress=None, auto: bool = False) -> ContinuationEvaluator:
    """``compress``, ``auto``: as for ``_resident_trdms``."""
    assert compress in (None, "sym8")
    t = _resident_trdms(one_RDM, two_RDM, S, compress, auto)
    key = ("evaluator", id(t), int(natm))
    ev = cache.get(key)
    if ev is None or ev.t is not t:
        ev = cache.put(key, ContinuationEvaluator(t, natm))
    return ev


def _solve_from_integrals(h1, h2, one_RDM, two_RDM, S, nroots, hermitian=True, ground_state=False):
    """H_ab from given OAO integrals (reference :38-68) + eigh(H, S) (:73-88), all on the device."""
    two_RDM = np.asarray(two_RDM) if not torch.is_tensor(two_RDM) else two_RDM
    assert two_RDM.ndim in (6, 5, 3, 2)          # reference: `assert False` otherwise (:70-71)
    t = _trdms(one_RDM, two_RDM, S)
    d = t.device
    h2d = ops.to_device(np.asarray(h2, dtype=np.float64).reshape((t.n,) * 4), d)
    h1d = ops.to_device(np.asarray(h1, dtype=np.float64), d).reshape(-1)
    if t.layout in (3, 2):
        v, alpha = ops.pack_pair_sym(h2d, 0.5, pad_to=t.ld), 1.0
    else:
        v, alpha = h2d.reshape(-1), 0.5
    rows2 = ops.gemv_rows(t.two, t.cols, v, alpha)[: t.rows_total]
    rows1 = ops.gemv_rows(t.one, t.n * t.n, h1d)          # t.one rows are padded to an even length
    ev, vec, _, _, Hd = ops.subspace_solve(rows1, rows2.contiguous(), t.S, t.layout, nroots)
    if not hermitian:
        return _select(*_eig_nonhermitian(Hd.cpu().numpy(), t.S.cpu().numpy(), t.layout), nroots, ground_state)
    e = ev.cpu().numpy()
    if not np.all(np.isfinite(e)):
        raise np.linalg.LinAlgError("generalised eigenproblem failed (overlap not positive definite?)")
    return e, vec.cpu().numpy()


def approximate_ground_state(h1, h2, one_RDM, two_RDM, S, hermitian=True):
    """(E, c) of the lowest generalised eigenpair (reference :12-90)."""
    if not hermitian:
        return _solve_from_integrals(h1, h2, one_RDM, two_RDM, S, 1, hermitian=False, ground_state=True)
    e, c = _solve_from_integrals(h1, h2, one_RDM, two_RDM, S, 1)
    return float(e[0]), c[0].copy()


def approximate_multistate(h1, h2, one_RDM, two_RDM, S, nroots=1, hermitian=True):
    """(E[nroots], C[nroots,T]) lowest eigenpairs, rows S-orthonormal (reference :93-175)."""
    T = np.asarray(S).shape[0]
    assert T >= nroots                               # reference :166
    return _solve_from_integrals(h1, h2, one_RDM, two_RDM, S, int(nroots), hermitian=bool(hermitian))


def _oao(mol, one_RDM, two_RDM, S, nroots, hermitian=True, ground_state=False):
    ao = ao_arrays(mol, need_grad=False)
    # (the non-Hermitian branch works on the subspace matrix of the layout the caller passed)
    ev = _evaluator(one_RDM, two_RDM, S, int(np.asarray(ao.aoslices).shape[0]),
                    compress=resolve_compression("default", one_RDM, two_RDM, S, ao if is_array_mol(mol) else mol,
                                                 hermitian=hermitian, need_grad=False),
                    auto=_COMPRESS == "auto")
    dao = DeviceAO.from_arrays(ao, ev.t.device, energy_only=True)
    res = ev.energies(dao, nroots)
    if hermitian:
        return res
    # same device pipeline (Loewdin, rotation, H build); only the T x T eigensolve differs
    e, c = _select(*_eig_nonhermitian(ev.hmat.cpu().numpy(), ev.t.S.cpu().numpy(), ev.t.layout), nroots, ground_state)
    return e + float(ao.enuc), c


def approximate_ground_state_OAO(mol, one_RDM, two_RDM, S, hermitian=True):
    """Total energy (incl. nuclear repulsion) and coefficients at the geometry of ``mol``
    (reference :178-211); Loewdin trafo, integral rotation, H build and eigensolve fused on the GPU."""
    if not hermitian:
        return _oao(mol, one_RDM, two_RDM, S, 1, hermitian=False, ground_state=True)
    e, c = _oao(mol, one_RDM, two_RDM, S, 1)
    return float(e[0]), c[0].copy()


def approximate_multistate_OAO(mol, one_RDM, two_RDM, S, nroots=1, hermitian=True):
    """Reference :214-250."""
    return _oao(mol, one_RDM, two_RDM, S, int(nroots), hermitian=bool(hermitian))


def _dipole_inputs(mol, origin):
    """``(dip (3,N,N), charges (A,), coords (A,3))`` of one molecule for the origin: an array-level molecule computes its
    own dipole integrals (``dipole_integrals(origin)``, e.g. ``hchain.HChainMol``), a PySCF ``Mole`` gives
    ``int1e_r`` under ``with_common_orig``."""
    if is_array_mol(mol):
        if not hasattr(mol, "dipole_integrals"):
            raise ValueError("array-level molecule without dipole_integrals(origin): no AO dipole integrals")
        return (np.asarray(mol.dipole_integrals(origin), dtype=np.float64), np.asarray(mol.charges, dtype=np.float64),
                np.asarray(mol.coords, dtype=np.float64).reshape(-1, 3))
    with mol.with_common_orig(origin):
        dip = np.asarray(mol.intor("int1e_r", comp=3), dtype=np.float64)
    return dip, np.asarray(mol.atom_charges(), dtype=np.float64), np.asarray(mol.atom_coords(), dtype=np.float64)


def get_multistate_properties(mols, one_rdm, two_rdm, overlap, nroots=1, pairs=None, origin=None, hermitian=True,
                              return_forces=False, device_trdms=None):
    """Dipole moments, transition dipole moments and atomic charges of the lowest ``nroots`` continuation states at
    every geometry of ``mols`` (geometries of ONE molecule), on the device in batches
    (``BatchedEvaluator.multistate_properties``): what the reference computes per geometry on the host at the end of
    its workflow (``scripts/MD/H2O-H3O+/evaluate_dipole_moment_charges_continuation.py:72-90``), for every root pair.

    ``pairs``: (P,2) root pairs k <= l < nroots, default the diagonal; ``origin``: of the dipole operator, default
    (0,0,0) (the dipole of a neutral molecule and every transition dipole between orthogonal states do not depend on
    it).  Returns ``E (G,nroots)`` and a dict of ``dipole (G,P,3)`` in atomic units (diagonal slots: total dipole;
    slot (k,l): the electronic transition dipole), ``mulliken_charges`` and ``loewdin_charges (G,P,A)``, ``C
    (G,nroots,T)``; with ``return_forces`` also ``grads (G,P,A,3)`` of the same slots from the same solve.
    ``device_trdms``: training data already on the device (``get_scanner``'s keyword), used instead of the host arrays.

    The populations are PLAIN Mulliken (PySCF's ``mulliken_pop``) and Loewdin; the reference script's
    ``mulliken_meta`` (meta-Loewdin, orthogonalised against PySCF's tabulated atomic reference orbitals) is not
    provided.  For array-level molecules the dipole integrals come from the molecule (``dipole_integrals(origin)``);
    for a PySCF ``Mole`` from ``mol.intor("int1e_r")`` under ``with_common_orig`` -- that branch is written against
    PySCF's documented interface and has NOT been run: PySCF was not available where this was developed."""
    from .ab_initio_gradients_loewdin import BATCH_WORKSPACE_BUDGET, _batched_evaluator
    from .evaluator import DeviceAOBatch
    import ctypes as C
    from . import _lib
    mols = list(mols)
    if not mols:
        raise ValueError("no geometries")
    nroots = int(nroots)
    origin = (0.0, 0.0, 0.0) if origin is None else tuple(float(x) for x in origin)
    need_grad = bool(return_forces)
    aos = [ao_arrays(m, need_grad=need_grad) for m in mols]
    natm = int(np.asarray(aos[0].aoslices).shape[0])
    if any(int(np.asarray(a.aoslices).shape[0]) != natm or a.S.shape != aos[0].S.shape for a in aos):
        raise ValueError("get_multistate_properties: the geometries must be of one molecule")
    t = device_trdms if device_trdms is not None else _resident_trdms(
        one_rdm, two_rdm, overlap, resolve_compression("default", one_rdm, two_rdm, overlap,
                                                       mols[0] if not is_array_mol(mols[0]) else aos[0],
                                                       hermitian=hermitian, need_grad=need_grad))
    if pairs is None:
        pairs = [(k, k) for k in range(nroots)]
    pairs = [tuple(int(x) for x in p) for p in np.asarray(pairs).reshape(-1, 2)]
    npairs = len(pairs)
    lib = _lib.load()
    per_slot = (lib.evc_workspace_bytes_roots_batch(C.byref(t.cstruct), natm, 1, 1) if need_grad
                else lib.evc_workspace_bytes_batch(C.byref(t.cstruct), natm, 1))
    if per_slot == 0:
        raise _lib.EvcontHipError("workspace size: " + lib.evc_last_error().decode())
    per_geo = per_slot * (npairs if need_grad else 1)
    chunk = max(1, min(len(mols), 4096 // npairs, BATCH_WORKSPACE_BUDGET // per_geo))
    if chunk * npairs > 4096:
        raise ValueError(f"{npairs} root pairs exceed the 4096 slots of one call")
    slices = torch.from_numpy(np.ascontiguousarray(aos[0].aoslices, dtype=np.int64)).to(t.device)
    E, Cs, grads, props = [], [], [], {}
    for c0 in range(0, len(mols), chunk):
        part = aos[c0: c0 + chunk]
        ev = _batched_evaluator(t, natm, len(part))
        aob = DeviceAOBatch.from_arrays(part, t.device, energy_only=not need_grad)
        aob.aoslices = slices
        dz = [_dipole_inputs(m, origin) for m in mols[c0: c0 + chunk]]
        res = ev.multistate_properties(aob, nroots, pairs, dip=np.stack([d[0] for d in dz]), charges=dz[0][1],
                                       coords=np.stack([d[2] for d in dz]), origin=origin, hermitian=hermitian,
                                       return_forces=need_grad)
        E.append(res[0])
        Cs.append(res[1])
        for k, v in res[2].items():
            props.setdefault(k, []).append(v)
        if need_grad:
            grads.append(res[3])
    out = {k: np.concatenate(v) for k, v in props.items()}
    out["C"] = np.concatenate(Cs)
    if need_grad:
        out["grads"] = np.concatenate(grads)
    return np.concatenate(E), out


def field_points(step) -> np.ndarray:
    """The seven fields of ``get_multistate_field_response``: 0, then ``+step`` and ``-step`` along x, y and z."""
    F = np.zeros((7, 3))
    for c in range(3):
        F[1 + 2 * c, c], F[2 + 2 * c, c] = float(step), -float(step)
    return F


def field_response_from_points(E, dip, grads, step) -> dict:
    """The result of ``get_multistate_field_response`` from the energies (7,R), dipoles (7,R,3) and gradients (7,R,A,3)
    at ``field_points(step)``: first central differences of the dipoles and of the forces."""
    E, dip, grads, h = np.asarray(E), np.asarray(dip), np.asarray(grads), float(step)
    alpha = np.stack([(dip[1 + 2 * c] - dip[2 + 2 * c]) / (2.0 * h) for c in range(3)], axis=-1)       # (R,3 mu,3 F)
    apt = np.stack([-(grads[1 + 2 * c] - grads[2 + 2 * c]) / (2.0 * h) for c in range(3)], axis=-1)    # (R,A,3 x,3 c)
    return {"energies": np.array(E[0]), "dipole": np.array(dip[0]), "polarizability": alpha, "apt": apt}


def get_multistate_field_response(mol, one_rdm, two_rdm, S, nroots, step, origin=(0.0, 0.0, 0.0), integrals="host",
                                  device_trdms=None):
    """Dipole, polarisability and atomic polar tensor of the lowest ``nroots`` continuation states of ``mol`` (an
    array-level molecule with ``with_field``: ``hchain.HChainMol``, ``gto_small.GaussianMol``,
    ``gto_spd.SpdGaussianMol``) by finite uniform fields: ONE batched ``multistate_properties(..., return_forces=True)``
    call over seven field points, ``F = 0`` and ``+-step e_x, +-step e_y, +-step e_z`` (atomic units) at the same
    coordinates.  Returns a dict, ``R = nroots``, ``A`` atoms:

        energies        (R,)       at zero field
        dipole          (R,3)      the zero-field dipole, taken directly (atomic units, ``origin``)
        polarizability  (R,3,3)    alpha[i,j] = d mu_i / dF_j, central differences of the DIPOLES
        apt             (R,A,3,3)  P[A,x,c] = d mu_c / dR_Ax = - d(grad_Ax) / dF_c, central differences of the FORCES

    Both are first differences of quantities the chain gives to ~1e-13; second differences of the energy would lose
    ``step``^-2 of that and are not used.  ``integrals``: "host" builds the seven molecules with ``with_field`` (numpy);
    "device" computes the integrals from the coordinates on the device and folds the fields there
    (``integrals(..., field=)`` of the device producers, ``csrc/field.hip``).  ``device_trdms``: as for
    ``get_multistate_properties``.

    Degeneracy warning (as for every several-roots call): the seven field points are seven independent solves; at
    (near-)degenerate roots they need not return the same state, or the same mixture within a degenerate space, and the
    differences between them are then meaningless for those roots."""
    nroots, h = int(nroots), float(step)
    if not h > 0.0:
        raise ValueError(f"step={step} must be positive")
    if integrals not in ("host", "device"):
        raise ValueError(f"unknown integrals={integrals!r} (known: 'host', 'device')")
    origin = tuple(float(x) for x in origin)
    F = field_points(h)
    pairs = [(k, k) for k in range(nroots)]
    if integrals == "host":
        base = mol if getattr(mol, "field", None) is None else mol.with_field((0.0, 0.0, 0.0))
        mols = [base] + [base.with_field(f, origin) for f in F[1:]]
        E, out = get_multistate_properties(mols, one_rdm, two_rdm, S, nroots, pairs, origin=origin, return_forces=True,
                                           device_trdms=device_trdms)
        dip, grads = out["dipole"], out["grads"]
    else:
        from . import _lib
        from .ab_initio_gradients_loewdin import _batched_evaluator
        from .MD_utils import _device_producer
        if 7 * nroots > 4096:
            raise ValueError(f"{nroots} roots at seven field points exceed the 4096 slots of one call")
        t = device_trdms if device_trdms is not None else _resident_trdms(
            one_rdm, two_rdm, S, resolve_compression("default", one_rdm, two_rdm, S, ao_arrays(mol, need_grad=True)))
        natm = int(np.asarray(mol.charges).shape[0])
        sg = _device_producer(mol).from_mol(mol, device=t.device)
        R = np.repeat(np.asarray(mol.coords, dtype=np.float64).reshape(1, natm, 3), 7, axis=0)
        aob = sg.integrals(R, packed=t.layout == _lib.LAYOUT_SYM8 and t.n <= 64, field=F, origin=origin)
        Rd = sg.staged_coords(7)
        E, _, props, grads = _batched_evaluator(t, natm, 7).multistate_properties(
            aob, nroots, pairs, dip=sg.dipole_integrals(Rd, origin), charges=sg.charges, coords=Rd, origin=origin,
            return_forces=True, observables=("dipole",))
        dip = props["dipole"]
    return field_response_from_points(E, dip, grads, h)
