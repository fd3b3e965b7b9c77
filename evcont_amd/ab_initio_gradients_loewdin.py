"""Device-backed mirror of ``evcont/ab_initio_gradients_loewdin.py`` (same public names,
signatures and array layouts)."""
from __future__ import annotations

import numpy as np
import torch

from . import gradients as G
from . import ops
from .ab_initio_eigenvector_continuation import (_evaluator, approximate_ground_state,  # noqa: F401
                                                 get_trdm_compression, resolve_compression)
from .electron_integral_utils import get_loewdin_trafo, restore_electron_exchange_symmetry  # noqa: F401
from .evaluator import DeviceAO, _dev
from .integrals import ao_arrays, grad_nuc, is_array_mol


def _dao(mol) -> DeviceAO:
    return DeviceAO.from_arrays(ao_arrays(mol, need_grad=True), _dev())


def get_overlap_grad(mol):
    """dS[mu,nu,A,x] (reference :13-38).  Pure index bookkeeping of int1e_ipovlp: done on the host."""
    ao = ao_arrays(mol, need_grad=True)
    n, A = ao.S.shape[0], len(ao.aoslices)
    d = np.zeros((3, A, n, n))
    for a, (p0, p1) in enumerate(np.asarray(ao.aoslices)):
        d[:, a, p0:p1, :] -= ao.ipovlp[:, p0:p1, :]
    d = d + d.transpose(0, 1, 3, 2)
    return np.ascontiguousarray(d.transpose(2, 3, 1, 0))


def loewdin_trafo_grad(overlap_mat):
    """d X / d S for all symmetrised unit perturbations, (N,N,N,N) (reference :41-112).

    Evaluated in closed (Daleckii-Krein divided-difference) form, which equals the reference's
    degenerate perturbation theory for non-degenerate and exactly degenerate spectra."""
    S = ops.to_device(np.asarray(overlap_mat, dtype=np.float64), _dev())
    return G.loewdin_trafo_grad_device(S).cpu().numpy()


def get_derivative_ao_mo_trafo(mol):
    """dX[k,l,A,x] (reference :115-134)."""
    return G.derivative_ao_mo_trafo_device(_dao(mol)).cpu().numpy()


def get_one_el_grad_ao(mol):
    """(N,N,A,3) AO derivative of hcore (reference :137-152): a transposition of PySCF's output."""
    ao = ao_arrays(mol, need_grad=True)
    return np.ascontiguousarray(np.asarray(ao.dhcore).transpose(2, 3, 0, 1))


def get_one_el_grad(mol, ao_mo_trafo=None, ao_mo_trafo_grad=None):
    """d h1^OAO / dR, (N,N,A,3) (reference :155-187)."""
    dao = _dao(mol)
    d = dao.S.device
    X = ops.loewdin(dao.S)[0] if ao_mo_trafo is None else ops.to_device(ao_mo_trafo, d)
    dX = G.derivative_ao_mo_trafo_device(dao) if ao_mo_trafo_grad is None else ops.to_device(ao_mo_trafo_grad, d)
    return G.one_el_grad_device(dao, X, dX).cpu().numpy()


def two_el_grad(h2_ao, two_rdm, ao_mo_trafo, ao_mo_trafo_grad, h2_ao_deriv, atm_slices):
    """Two-electron gradient (A,3) (reference :190-252)."""
    d = _dev()
    sl = torch.from_numpy(np.ascontiguousarray(np.asarray(atm_slices, dtype=np.int64).reshape(-1, 2))).to(d)
    up = lambda x: ops.to_device(np.asarray(x, dtype=np.float64), d)
    n = np.asarray(ao_mo_trafo).shape[0]
    return G.two_el_grad_device(up(h2_ao).reshape((n,) * 4), up(two_rdm), up(ao_mo_trafo), up(ao_mo_trafo_grad),
                                up(h2_ao_deriv).reshape((3,) + (n,) * 4), sl).cpu().numpy()


def get_grad_elec_OAO(mol, one_rdm, two_rdm, ao_mo_trafo=None, ao_mo_trafo_grad=None):
    """Electronic gradient of given OAO RDMs, (A,3) (reference :255-305)."""
    dao = _dao(mol)
    d = dao.S.device
    D = ops.to_device(np.asarray(one_rdm, dtype=np.float64), d)
    Gm = ops.to_device(np.asarray(two_rdm, dtype=np.float64), d)
    if ao_mo_trafo_grad is None:
        X = None if ao_mo_trafo is None else ops.to_device(ao_mo_trafo, d)
        return G.grad_elec_oao_device(dao, D, Gm, X).cpu().numpy()
    # explicit trafo derivative supplied: assemble from the tensor-valued pieces (reference :279-303)
    X = ops.loewdin(dao.S)[0] if ao_mo_trafo is None else ops.to_device(ao_mo_trafo, d)
    dX = ops.to_device(ao_mo_trafo_grad, d)
    h1_jac = G.one_el_grad_device(dao, X, dX)
    g2 = G.two_el_grad_device(dao.eri, Gm, X, dX, dao.eri_ip1, dao.aoslices)
    return (G.contract_nnA3_device(h1_jac, D) + 0.5 * g2).cpu().numpy()


def get_energy_with_grad(mol, one_RDM, two_RDM, S, hermitian=True, return_density_matrices=False):
    """Total energy and nuclear gradient of the continuation at ``mol``'s geometry (reference :308-379).

    The t-RDMs are uploaded once (``evcont_amd.cache``) and stay resident; each call ships only
    the AO integrals of the new geometry and enqueues one fused device pipeline."""
    ao = ao_arrays(mol, need_grad=True)
    natm = int(np.asarray(ao.aoslices).shape[0])
    if not hermitian:
        # the eig branch works on the subspace matrix of the layout the caller passed (no sym8 compression)
        ev = _evaluator(one_RDM, two_RDM, S, natm, compress=None)
        return ev.energy_with_grad_nonhermitian(DeviceAO.from_arrays(ao, ev.t.device),
                                                return_density_matrices=return_density_matrices)
    # default ("auto"): the compressed resident copy + symmetric pipeline when the call only wants (E, grad) and the
    # integrals have the symmetries of real ones; the caller's layout otherwise (predicted RDMs as the reference
    # returns them)
    ev = _evaluator(one_RDM, two_RDM, S, natm,
                    compress=resolve_compression("default", one_RDM, two_RDM, S, mol if not is_array_mol(mol) else ao,
                                                 hermitian=True, want_rdms=return_density_matrices),
                    auto=get_trdm_compression() == "auto")
    dao = DeviceAO.from_arrays(ao, ev.t.device)
    return ev.energy_with_grad(dao, return_density_matrices=return_density_matrices)


def _evaluator_of(t, natm: int):
    """The single-geometry evaluator on training data already on the device (``device_trdms=``), cached like the
    others."""
    from . import cache
    from .evaluator import ContinuationEvaluator
    key = ("evaluator", id(t), int(natm))
    ev = cache.get(key)
    if ev is None or ev.t is not t:
        ev = cache.put(key, ContinuationEvaluator(t, natm))
    return ev


def get_multistate_energy_with_grad(mol, one_RDM, two_RDM, S, nroots=1, hermitian=True, return_couplings=False,
                                    return_density_matrices=False, device_trdms=None):
    """Total energies ``E[nroots]`` and nuclear gradients ``grad[nroots,A,3]`` of the lowest ``nroots`` continuation
    states at ``mol``'s geometry: ``get_energy_with_grad`` with the eigenvector c_k of root k in place of c_0
    (S_train does not depend on the geometry, so dE_k/dR = c_k^T dH/dR c_k), all roots in one device pass.

    ``return_couplings``: also ``h[nroots,nroots,A,3]``, the interstate coupling vectors c_k^T dH/dR c_l (symmetric in
    k, l; the diagonal is the electronic gradient of root k; the derivative coupling is h_kl / (E_l - E_k)).
    ``return_density_matrices``: also the predicted RDMs of every root, ``D[nroots,N,N]`` and ``G[nroots,N,N,N,N]``,
    as ``get_energy_with_grad`` returns them.  Storage of the resident training data as for ``get_energy_with_grad``.
    ``device_trdms``: training data already on the device (``get_scanner``'s keyword, e.g. a resident container's
    ``device_trdms()``), used instead of the host arrays, which may then be ``None``.
    At (near-)degenerate roots the forces follow whichever eigenvectors the solver returned."""
    nroots = int(nroots)
    ao = ao_arrays(mol, need_grad=True)
    natm = int(np.asarray(ao.aoslices).shape[0])
    if device_trdms is not None:
        ev = _evaluator_of(device_trdms, natm)
    else:
        ev = _evaluator(one_RDM, two_RDM, S, natm,
                        compress=resolve_compression("default", one_RDM, two_RDM, S,
                                                     mol if not is_array_mol(mol) else ao, hermitian=hermitian,
                                                     want_rdms=return_density_matrices),
                        auto=get_trdm_compression() == "auto")
    pairs = _root_pairs(nroots, return_couplings)
    res = ev.energies_with_grads(DeviceAO.from_arrays(ao, ev.t.device), nroots, pairs,
                                 return_density_matrices=return_density_matrices, hermitian=hermitian)
    e, grads = res[0], res[2]
    out = (e, grads[:nroots].copy())
    if return_couplings:
        out += (_fold_couplings(grads, pairs, nroots, np.asarray(ao.gnuc, dtype=np.float64)),)
    if return_density_matrices:
        out += (res[3][:nroots], res[4][:nroots])
    return out


def _root_pairs(nroots: int, couplings: bool):
    """The slots of a multistate call: (k, k) for every root, then with ``couplings`` every (k, l), k < l."""
    pairs = [(k, k) for k in range(nroots)]
    if couplings:
        pairs += [(k, l) for k in range(nroots) for l in range(k + 1, nroots)]
    return pairs


def _fold_couplings(grads, pairs, nroots: int, gnuc):
    """``h[..., k, l] = h[..., l, k]`` from the slots ``grads[..., p, :, :]`` of ``pairs`` (any leading geometry axes),
    with the nuclear term ``gnuc (..., A, 3)`` taken off the diagonal: the electronic gradients."""
    h = np.zeros(grads.shape[:-3] + (nroots, nroots) + grads.shape[-2:])
    for p, (k, l) in enumerate(pairs):
        h[..., k, l, :, :] = h[..., l, k, :, :] = grads[..., p, :, :]
    for k in range(nroots):
        h[..., k, k, :, :] -= gnuc
    return h


# Workspace bytes one call of get_multistate_energies_with_grads may hold (the list is split into chunks below this and
# below 4096 slots of geometries x root pairs).
BATCH_WORKSPACE_BUDGET = 8 << 30


def _batched_evaluator(t, natm: int, count: int):
    from . import cache
    from .evaluator import BatchedEvaluator
    key = ("batched_evaluator", id(t), int(natm), int(count))
    ev = cache.get(key)
    if ev is None or ev.t is not t:
        ev = cache.put(key, BatchedEvaluator(t, natm, count))
    return ev


def get_multistate_energies_with_grads(mols, one_RDM, two_RDM, S, nroots=1, hermitian=True, return_couplings=False,
                                       device_trdms=None):
    """``get_multistate_energy_with_grad`` for a list of geometries of ONE molecule, evaluated in batches (every
    geometry of a batch and all its roots in one pass of the gradient chain, ``evc_phase_gradient_roots_batch``).

    Returns stacked arrays ``E[G,nroots]`` and ``grad[G,nroots,A,3]``, with ``return_couplings`` also
    ``h[G,nroots,nroots,A,3]`` (symmetric in k, l; the diagonal is the electronic gradient of root k), with the storage
    of the training data and the coupling conventions of ``get_multistate_energy_with_grad``.  The list is split so
    that a batch holds at most 4096 (geometry, root pair) slots and ``BATCH_WORKSPACE_BUDGET`` bytes of workspace.
    ``device_trdms``: as for ``get_multistate_energy_with_grad``."""
    import ctypes as C
    from . import _lib
    from .ab_initio_eigenvector_continuation import _resident_trdms
    from .evaluator import DeviceAOBatch
    mols = list(mols)
    if not mols:
        raise ValueError("no geometries")
    nroots = int(nroots)
    aos = [ao_arrays(m, need_grad=True) for m in mols]
    natm = int(np.asarray(aos[0].aoslices).shape[0])
    if any(int(np.asarray(a.aoslices).shape[0]) != natm or a.S.shape != aos[0].S.shape for a in aos):
        raise ValueError("get_multistate_energies_with_grads: the geometries must be of one molecule")
    t = device_trdms if device_trdms is not None else _resident_trdms(
        one_RDM, two_RDM, S, resolve_compression("default", one_RDM, two_RDM, S,
                                                 mols[0] if not is_array_mol(mols[0]) else aos[0], hermitian=hermitian))
    pairs = _root_pairs(nroots, return_couplings)
    npairs = len(pairs)
    lib = _lib.load()
    per_slot = lib.evc_workspace_bytes_roots_batch(C.byref(t.cstruct), natm, 1, 1)
    if per_slot == 0:
        raise _lib.EvcontHipError("evc_workspace_bytes_roots_batch: " + lib.evc_last_error().decode())
    chunk = max(1, min(len(mols), 4096 // npairs, BATCH_WORKSPACE_BUDGET // (per_slot * npairs)))
    if chunk * npairs > 4096:
        raise ValueError(f"nroots={nroots}: {npairs} root pairs exceed the 4096 slots of one call")
    E, grads = [], []
    for c0 in range(0, len(mols), chunk):
        part = aos[c0: c0 + chunk]
        ev = _batched_evaluator(t, natm, len(part))
        aob = DeviceAOBatch.from_arrays(part, t.device)
        e, _, g = ev.multistate_energies_with_grads(aob, nroots, pairs, hermitian=hermitian)
        E.append(e)
        grads.append(g)
    E, grads = np.concatenate(E), np.concatenate(grads)
    out = (E, grads[:, :nroots].copy())
    if return_couplings:
        out += (_fold_couplings(grads, pairs, nroots, np.stack([np.asarray(a.gnuc, dtype=np.float64) for a in aos])),)
    return out
