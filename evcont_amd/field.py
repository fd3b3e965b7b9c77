"""A molecule in a uniform electric field: the host statement (numpy) of ``csrc/field.hip``.

For a field ``F`` and an origin ``O`` of the dipole operator, ``H(F) = H0 - mu . F`` with
``mu = sum_A Z_A (R_A - O) - sum_i (r_i - O)``, so four of the arrays a geometry hands to the evaluators change:

    hcore  += sum_c F_c <mu| r_c - O_c |nu>
    dhcore += sum_c F_c d<mu| r_c - O_c |nu> / dR_A
    enuc   -= sum_A Z_A F . (R_A - O)
    gnuc[A] -= Z_A F

and everything behind them (the Loewdin basis, the rotations, the subspace problem, the gradient) runs unchanged.  The
nuclear derivative of the dipole integrals comes from ``ipdip[x,c,mu,nu] = <d_x mu| r_c - O_c |nu>`` (the
electron-coordinate gradient on the bra, the convention of ``ipovlp``; ``dipole_grad_integrals`` of the molecule classes):

    d dip_c[mu,nu] / dR_Ax = - ipdip[x,c,mu,nu] [mu in A] - ipdip[x,c,nu,mu] [nu in A]

The molecule classes (``hchain.HChainMol``, ``gto_small.GaussianMol``, ``gto_spd.SpdGaussianMol``) delegate their
``with_field`` to ``with_field`` here; the device route is ``evc_field_fold_batch`` behind ``integrals(..., field=)`` of
the three device producers, and these functions are the oracle of its tests.

Derived quantities (``ab_initio_eigenvector_continuation.get_multistate_field_response``): the polarisability
``alpha = d mu / dF`` and the atomic polar tensor ``P[A,x,c] = d mu_c / dR_Ax = - d(grad_Ax) / dF_c``.
"""
from __future__ import annotations

import dataclasses

import numpy as np


def dipole_derivative(ipdip, aoslices) -> np.ndarray:
    """``d dip_c[mu,nu] / dR_Ax`` as (A,3,3,N,N) (atom, x, c) from ``ipdip`` (3,3,N,N) (x, c)."""
    ipdip = np.asarray(ipdip, dtype=np.float64)
    sl = np.asarray(aoslices).reshape(-1, 2)
    n = ipdip.shape[-1]
    out = np.zeros((sl.shape[0], 3, 3, n, n))
    for at, (s0, s1) in enumerate(sl):
        out[at, :, :, s0:s1, :] -= ipdip[:, :, s0:s1, :]
        out[at, :, :, :, s0:s1] -= ipdip[:, :, s0:s1, :].transpose(0, 1, 3, 2)
    return out


def field_terms(F, origin, dip, ipdip, aoslices, charges, coords):
    """The four additions of a field ``F`` (3,): ``(dhcore_0 (N,N), ddhcore (A,3,N,N) or None, denuc, dgnuc (A,3))``;
    ``ipdip`` None: no gradient terms."""
    F = np.asarray(F, dtype=np.float64).reshape(3)
    O = np.asarray(origin, dtype=np.float64).reshape(3)
    Z = np.asarray(charges, dtype=np.float64).reshape(-1)
    R = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
    dh = np.einsum("c,cij->ij", F, np.asarray(dip, dtype=np.float64))
    ddh = None if ipdip is None else np.einsum("c,axcij->axij", F, dipole_derivative(ipdip, aoslices))
    return dh, ddh, -float(Z @ ((R - O) @ F)), -Z[:, None] * F[None, :]


def has_gradients(mol) -> bool:
    """Whether an array-level molecule carries its derivative arrays (built with ``need_grad``)."""
    return int(np.asarray(mol.eri_ip1).size) > 0


def _add(mol, F, origin, sign=1.0):
    grad = has_gradients(mol)
    dh, ddh, de, dg = field_terms(sign * np.asarray(F, dtype=np.float64), origin, mol.dipole_integrals(origin),
                                  mol.dipole_grad_integrals(origin) if grad else None, mol.aoslices, mol.charges,
                                  mol.coords)
    new = dict(hcore=mol.hcore + dh, enuc=float(mol.enuc) + de)
    if grad:
        new.update(dhcore=mol.dhcore + ddh, gnuc=mol.gnuc + dg)
    return dataclasses.replace(mol, **new)


def with_field(mol, F, origin=(0.0, 0.0, 0.0)):
    """A copy of the array-level molecule ``mol`` in the uniform field ``F`` (3,) (atomic units) with the dipole
    operator's origin ``origin``: ``hcore`` and ``enuc``, and with gradients ``dhcore`` and ``gnuc``, carry the field
    terms; ``field`` / ``field_origin`` record it.  The copy is in the field ``F``, not in ``F`` on top of a field
    ``mol`` already is in (that one is taken out first)."""
    F = np.array(F, dtype=np.float64).reshape(3)
    origin = tuple(float(x) for x in np.asarray(origin, dtype=np.float64).reshape(3))
    if getattr(mol, "field", None) is not None:
        mol = dataclasses.replace(_add(mol, mol.field, mol.field_origin, -1.0), field=None)
    return dataclasses.replace(_add(mol, F, origin), field=F, field_origin=origin)


def keep_field(old, new):
    """``new`` (the molecule of ``old`` at other coordinates, field-free) in the field ``old`` is in."""
    if getattr(old, "field", None) is None:
        return new
    return with_field(new, old.field, old.field_origin)
