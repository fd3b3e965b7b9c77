"""``CAS_EVCont_obj``: container for continuation training data from CASCI states (mirror of the
class in ``evcont/CASCI_EVCont.py:93-361``: constructor, attributes, ``prune_datapoints``).

Generating CASCI training states needs PySCF (RHF + CASCI) and pygnme (non-orthogonal Wick's theorem
for the transition RDMs between different orbital sets); that is training-time host work outside the
accelerated path (out of scope).  ``append_to_rdms`` therefore delegates the per-pair
overlap / transition-RDM evaluation to a user-supplied ``pair_rdm_fun(casci_bra, casci_ket) ->
(ovlp, rdm1, rdm2)`` in the OAO basis (what ``CASCI_EVCont.py:204-335`` computes with pygnme) and
raises ImportError when neither that nor PySCF is available.  Everything downstream — array growth,
pruning, the device-resident packed copy — is shared with the other containers.

With a ``cisolver`` (``fci_small.SmallFCI()`` or ``fci_device.DeviceFCI()``) nothing third-party is needed:
``append_to_rdms(mol)`` runs ``cas_small.casci`` on the molecule's RHF orbitals and reduces each pair of CAS states in
different orbital sets to a non-orthogonal ``transform_ci`` and an active-space t-RDM (``cas_small``),
on the device when the solver has ``cas_trans_rdm12_rows``.

``nroots`` / ``roots_train`` mean what they mean in ``FCI_EVCont_obj``: ``max(roots_train) + 1`` CASCI roots are solved per
geometry (``cas_small.casci_roots``) and the listed ones appended in root order, with one ``mol_index`` per geometry.  The
roots of a geometry share their orbitals, so their rows against the stored states come from one block call
(``cas_small.trans_rdm12_block`` / ``DeviceFCI.cas_trans_rdm12_block``).  Built-in route only.
"""
from __future__ import annotations

import numpy as np

from .containers import TRDMContainer


class CAS_EVCont_obj(TRDMContainer):
    def __init__(self, ncas, neleca, casci_solver=None, pair_rdm_fun=None, cisolver=None, nroots=1, roots_train=None):
        super().__init__()
        self.nroots = nroots
        if roots_train is None:
            self.roots_train = list(range(nroots))
        else:
            assert isinstance(roots_train, list) and roots_train and min(roots_train) >= 0
            self.roots_train = sorted(roots_train)
        self.mol_index = []
        self.ncas = ncas
        self.neleca = neleca
        self.cascis = []
        self.ens = []
        self.casci_solver = casci_solver
        self.pair_rdm_fun = pair_rdm_fun
        self.cisolver = cisolver

    def _append_own(self, mol):
        """The built-in route: ``cas_small.casci`` and the pair reduction of ``cas_small`` (host or device)."""
        from . import cas_small
        mindex = 0 if len(self.mol_index) == 0 else max(self.mol_index) + 1
        if self.roots_train != [0]:
            return self._append_own_roots(mol, mindex)
        state = cas_small.casci(mol, self.ncas, self.neleca, self.cisolver)
        kets = self.cascis + [state]
        # (a pair beyond the conditioning guard raises here: the container is then as it was)
        if hasattr(self.cisolver, "cas_trans_rdm12_rows"):
            ovlp, one, two = self.cisolver.cas_trans_rdm12_rows(state, kets)
        else:
            ovlp, one, two = cas_small.trans_rdm12_rows(state, kets, self.cisolver)
        self.cascis.append(state)
        self.ens.append(state.e_tot)
        self.mol_index.append(mindex)
        self._append_state(ovlp, one, two)

    def _append_own_roots(self, mol, mindex):
        """Several roots of one geometry: one block call gives the rows of all of them, the new corner included."""
        from . import cas_small
        roots = cas_small.casci_roots(mol, self.ncas, self.neleca, self.cisolver, max(self.roots_train) + 1)
        bras = [roots[k] for k in self.roots_train]
        kets = self.cascis + bras
        # (a pair beyond the conditioning guard raises here: the container is then as it was)
        if hasattr(self.cisolver, "cas_trans_rdm12_block"):
            ovlp, one, two = self.cisolver.cas_trans_rdm12_block(bras, kets)
        else:
            ovlp, one, two = cas_small.trans_rdm12_block(bras, kets, self.cisolver)
        T = len(self.cascis)
        for r, state in enumerate(bras):
            # root r as the bra against everything before it and itself: the arrays a one-by-one append would give
            self.cascis.append(state)
            self.ens.append(state.e_tot)
            self.mol_index.append(mindex)
            self._append_state(ovlp[r, :T + r + 1], one[r, :T + r + 1], two[r, :T + r + 1])

    def append_to_rdms(self, mol):
        if self.cisolver is not None:
            return self._append_own(mol)
        if self.roots_train != [0]:
            raise NotImplementedError("CAS_EVCont_obj: several roots per geometry need the built-in route (cisolver=...); "
                                      "the PySCF / pair_rdm_fun route is ground state only")
        if self.casci_solver is None:
            try:
                from pyscf.mcscf import CASCI
            except ImportError as e:
                raise ImportError("CAS_EVCont_obj.append_to_rdms needs PySCF (RHF/CASCI training states are "
                                  "generated on the host) or an explicit casci_solver") from e
            self.casci_solver = CASCI
        if self.pair_rdm_fun is None:
            raise ImportError("CAS_EVCont_obj.append_to_rdms needs pair_rdm_fun(casci_bra, casci_ket) -> "
                              "(overlap, rdm1, rdm2) in the OAO basis (the reference evaluates it with pygnme, "
                              "CASCI_EVCont.py:204-335)")
        mf = mol.copy().RHF()
        mf.kernel()
        assert mf.converged
        casci_bra = self.casci_solver(mf, self.ncas, self.neleca)
        casci_bra.kernel()
        assert casci_bra.fcisolver.converged
        self.cascis.append(casci_bra)
        T1 = len(self.cascis)
        n = casci_bra.mo_coeff.shape[0]
        ovlp, one, two = np.empty(T1), np.empty((T1, n, n)), np.empty((T1, n, n, n, n))
        for i, ket in enumerate(self.cascis):
            ovlp[i], one[i], two[i] = self.pair_rdm_fun(casci_bra, ket)
        self._append_state(ovlp, one, two)

    def prune_datapoints(self, keep_ids):
        """``CASCI_EVCont.py:345-361``."""
        self._prune_arrays(keep_ids)
        self.cascis = [self.cascis[i] for i in keep_ids]
        if self.mol_index:
            self.mol_index = [self.mol_index[i] for i in keep_ids]
        if self.ens:
            self.ens = [self.ens[i] for i in keep_ids]
