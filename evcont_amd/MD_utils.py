"""Device-backed mirror of the evaluator-facing part of ``evcont/MD_utils.py``.

``get_scanner`` (reference :20-57) is the harness PySCF's MD integrators call once per step;
``get_trajectory`` (:60-125) is a thin wrapper around ``pyscf.md.NVE`` (or the velocity-Verlet
driver below for array-level molecules).  The active-learning driver ``converge_EVCont_MD``
(:128-502) lives in ``evcont_amd/active_learning.py``.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .ab_initio_gradients_loewdin import get_energy_with_grad
from .ab_initio_eigenvector_continuation import (approximate_ground_state_OAO, _trdms,  # noqa: F401 (re-export)
                                                 _resident_trdms, _trdms_auto, get_trdm_compression,
                                                 integrals_have_symmetry)
from .electron_integral_utils import get_basis, get_integrals  # noqa: F401 (re-export)
from .evaluator import ContinuationEvaluator, DeviceAO
from .hosted import HostedEvaluator
from .integrals import ao_arrays, aoslices_of, energy_nuc, grad_nuc, is_array_mol, stage_mol


def _grad_scanner_base():
    try:
        from pyscf import lib
        return lib.GradScanner
    except Exception:  # PySCF absent: the scanner is still a plain callable (tests, array-level mols)
        return object


def get_scanner(mol, one_rdm, two_rdm, overlap, hermitian=True, compress="default", device_trdms=None):
    """Fake PySCF gradient scanner driven by the continuation (reference :20-57): ``scanner(mol)``
    returns ``(E_tot, grad)`` and stores the predicted RDMs on ``scanner.base``.

    ``compress``: storage of the resident training data, ``None``, ``"sym8"``, ``"auto"`` or ``"default"``
    (= ``set_trdm_compression``, "auto" unless changed).  "auto": the 8-fold compressed copy and the packed s4 / s2kl
    integrals for the per-step ``(E, grad)`` when ``hermitian``, the training set's bra<->ket partner blocks compress
    alike and the first molecule's integrals have the symmetries of real ones (a PySCF ``Mole`` always; array-level
    molecules are checked completely once; the packed staging spot-checks every later one and raises), with
    ``predicted_two_rdm`` still the reference's un-symmetrised 2-RDM (evaluated on the caller's layout when it is
    read); with ``"sym8"`` the stored predicted 2-RDM is the 8-fold symmetrised one.
    ``device_trdms``: training data already resident on the device (``trdm_io.load_pair_directories`` /
    ``load_checkpoint``, a container's ``device_trdms()``): used instead of uploading the host arrays."""
    if compress == "default":
        compress = get_trdm_compression()
    if compress not in (None, "sym8", "auto"):
        raise ValueError(f"unknown t-RDM compression {compress!r} (known: None, 'sym8', 'auto', 'default')")
    auto = compress == "auto"

    have_data = device_trdms is not None or (one_rdm is not None and two_rdm is not None and overlap is not None)

    class Base:
        """``scanner.base`` of the reference (:26-32).  The predicted RDMs are fetched from the device when they are
        read: integrator callbacks use ``predicted_one_rdm`` (``04_Zundel_continuation_MD.py:145``); nothing in the
        reference reads the N^4 ``predicted_two_rdm`` during a run, so it is produced on first access (a second
        evaluation of the current geometry with the unpacked 2-RDM as an output) instead of being shipped every step."""
        converged = True
        ovlp = overlap
        one_trdm = one_rdm
        two_trdm = two_rdm

        def __init__(self, owner):
            self._owner = owner

        @property
        def predicted_one_rdm(self):
            return self._owner._one()

        @property
        def predicted_two_rdm(self):
            return self._owner._two()

    class Scanner(_grad_scanner_base()):
        def __init__(self):
            self.mol = mol
            self.base = Base(self)
            self._compress = None if auto else compress   # "auto": decided at the first call (needs integrals)
            self._decided = not auto
            self._hev = None          # HostedEvaluator (Hermitian path)
            self._full = None         # ContinuationEvaluator with every output (lazy 2-RDM, hermitian=False)
            self._last = None         # (mol, D, G) of the last call as far as known

        # -- lazily fetched outputs -----------------------------------------------------------------
        def _one(self):
            if self._last is None:
                return None
            if self._last[1] is None and self._hev is not None:
                self._last[1] = self._hev.predicted_one_rdm()
            return self._last[1]

        def _two(self):
            if self._last is None:
                return None
            if self._last[2] is None:
                self._last[2] = self._full_eval(self._last[0])[3]
            return self._last[2]

        def _full_eval(self, m):
            ao = ao_arrays(m, need_grad=True)
            if self._full is None:
                # "auto": the predicted 2-RDM as the reference returns it -- from the layout the caller passed
                t = device_trdms if device_trdms is not None else \
                    _trdms(one_rdm, two_rdm, overlap, None if auto else self._compress)
                self._full = ContinuationEvaluator(t, int(np.asarray(ao.aoslices).shape[0]))
            return self._full.energy_with_grad(DeviceAO.from_arrays(ao, self._full.t.device), True)

        def __call__(self, mol):
            self.mol = mol
            if not have_data:
                return energy_nuc(mol), grad_nuc(mol)
            if not hermitian:
                if device_trdms is not None and (one_rdm is None or two_rdm is None or overlap is None):
                    # training data resident on the device only: the eig branch on ITS layout (not the compressed one)
                    if self._full is None:
                        self._full = ContinuationEvaluator(device_trdms, len(aoslices_of(mol)))
                    ao = ao_arrays(mol, need_grad=True)
                    en, grad, rdm_o, rdm_t = self._full.energy_with_grad_nonhermitian(
                        DeviceAO.from_arrays(ao, device_trdms.device), True)
                else:
                    en, grad, rdm_o, rdm_t = get_energy_with_grad(
                        mol, one_rdm, two_rdm, overlap, hermitian=hermitian, return_density_matrices=True)
                self._last = [mol, rdm_o, rdm_t]
                return en, grad
            # called once per MD step on slowly moving geometries: the scanner owns a hosted evaluator (pinned
            # staging, eager two-stream enqueue of uploads + kernels + download -- replaying the step as one HIP graph
            # is an opt-in, EVCONT_AMD_HOSTED_GRAPH=1, measured slower --, eigensolvers warm-started from the previous
            # step; with the compressed layout the two large integral arrays are requested / staged packed: 12 instead
            # of 26.6 MB at H30)
            if self._hev is None:
                if not self._decided:
                    self._compress = "sym8" if integrals_have_symmetry(mol) else None
                    self._decided = True
                if device_trdms is not None:
                    t = device_trdms
                elif auto:      # (the caller's layout for a training set the compressed one cannot represent)
                    t = _trdms_auto(one_rdm, two_rdm, overlap, self._compress)
                    self._compress = "sym8" if t.layout == _lib.LAYOUT_SYM8 else None
                else:
                    t = _trdms(one_rdm, two_rdm, overlap, self._compress)
                sl = aoslices_of(mol)
                self._hev = HostedEvaluator(t, len(sl), sl, warm_start=True)
            stage_mol(mol, self._hev)
            en, grad = self._hev.run()
            self._last = [mol, None, None]
            return en, grad

    return Scanner()


def get_state_scanner(mol, one_rdm, two_rdm, overlap, root, hermitian=True):
    """``get_scanner`` for the continuation eigenstate ``root`` (0 = ground state): ``scanner(mol)`` returns
    ``(E_root, grad_root)`` and ``scanner.base.predicted_one_rdm`` / ``predicted_two_rdm`` are that root's predicted
    RDMs.  Each call evaluates the lowest ``root + 1`` energies and the gradient of ``root`` alone (one slot of
    ``evc_phase_gradient_roots``); consecutive calls warm-start the eigensolvers.  Drives excited-state NVE through
    ``nve_velocity_verlet(scanner, mol, ...)``.  At (near-)degenerate roots the forces follow whichever eigenvector
    the solver returned: a trajectory through a crossing does not follow a diabatic state."""
    from .ab_initio_eigenvector_continuation import resolve_compression
    from .ab_initio_gradients_loewdin import get_multistate_energy_with_grad
    root = int(root)
    if root < 0:
        raise ValueError(f"root={root} must be >= 0")

    class Base:
        converged = True
        ovlp = overlap
        one_trdm = one_rdm
        two_trdm = two_rdm

        def __init__(self, owner):
            self._owner = owner

        @property
        def predicted_one_rdm(self):
            return None if self._owner._last is None else self._owner._last[1]

        @property
        def predicted_two_rdm(self):
            return self._owner._two()

    class Scanner(_grad_scanner_base()):
        def __init__(self):
            self.mol = mol
            self.root = root
            self.base = Base(self)
            self._ev = None
            self._last = None         # (mol, D, G) of the last call; G on first access

        def _two(self):
            if self._last is None:
                return None
            if self._last[2] is None:
                r = get_multistate_energy_with_grad(self._last[0], one_rdm, two_rdm, overlap, root + 1,
                                                    hermitian=hermitian, return_density_matrices=True)
                self._last[2] = r[-1][root]
            return self._last[2]

        def __call__(self, mol):
            self.mol = mol
            ao = ao_arrays(mol, need_grad=True)
            if self._ev is None:
                compress = resolve_compression("default", one_rdm, two_rdm, overlap,
                                               ao if is_array_mol(mol) else mol, hermitian=hermitian)
                t = _resident_trdms(one_rdm, two_rdm, overlap, compress)
                self._ev = ContinuationEvaluator(t, int(np.asarray(ao.aoslices).shape[0]), warm_start=True,
                                                 want_two_rdm=False)
            ev = self._ev
            e, _, grads, D, _ = ev._roots(DeviceAO.from_arrays(ao, ev.t.device), root + 1, [(root, root)], True,
                                          False, hermitian)
            self._last = [mol, D[0].cpu().numpy(), None]
            return float(e[root]), grads[0, : ev.natm].cpu().numpy()

    return Scanner()


def get_trajectory(init_mol, overlap, one_rdm, two_rdm, dt=10.0, steps=10, init_veloc=None, hermitian=True,
                   trajectory_output=None, energy_output=None, compress="default", device_trdms=None,
                   integrals="host"):
    """NVE trajectory from the continuation (reference :60-125).  Single process: the reference's
    rank-0-computes / Bcast split exists only to coexist with MPI-parallel training code.

    PySCF molecules are propagated by ``pyscf.md.NVE`` exactly as in the reference; array-level molecules
    that can be rebuilt at new coordinates (``with_coords``, e.g. ``evcont_amd.hchain.HChainMol``) by the
    velocity-Verlet integrator below, with the same conventions (Bohr, atomic time units, frame 0 = the
    initial geometry, ``steps`` frames).  ``device_trdms``: as for ``get_scanner`` (training data already on the
    device, e.g. ``resident.ResidentFCI_EVCont_obj.device_trdms()``; ``two_rdm`` may then be ``None``).
    ``integrals="device"`` (s-Gaussian ``with_coords`` molecules, Hermitian branch, host training arrays, no output
    files): the one-trajectory case of ``state_swarm(..., integrals="device")`` -- the AO integrals of every step are
    computed on the device from the coordinates."""
    if integrals == "device":
        if not (hermitian and device_trdms is None and compress == "default" and trajectory_output is None
                and energy_output is None):
            raise ValueError('get_trajectory(integrals="device") takes the Hermitian branch on host training arrays with '
                             "the default compression and writes no output files")
        v0 = None if init_veloc is None else np.asarray(init_veloc, dtype=np.float64)[None]
        frames = state_swarm([init_mol], one_rdm, two_rdm, overlap, 0, dt=dt, steps=steps, init_veloc=v0,
                             integrals="device")
        return np.array([f["coord"][0] for f in frames])
    if integrals != "host":
        raise ValueError(f"unknown integrals={integrals!r} (known: 'host', 'device')")
    scanner_fun = get_scanner(init_mol, one_rdm, two_rdm, overlap, hermitian=hermitian, compress=compress,
                              device_trdms=device_trdms)
    if hasattr(init_mol, "with_coords"):
        frames = nve_velocity_verlet(scanner_fun, init_mol, dt=dt, steps=steps, veloc=init_veloc,
                                     trajectory_output=trajectory_output, energy_output=energy_output)
        return np.array([f["coord"] for f in frames])
    from pyscf import md  # needs PySCF's integrator
    frames = []
    integ = md.NVE(scanner_fun, dt=dt, steps=steps, veloc=init_veloc, incore_anyway=True, frames=frames,
                   trajectory_output=trajectory_output, energy_output=energy_output, verbose=0)
    integ.run()
    return np.array([frame.coord for frame in frames])


AMU2AU = 1822.888486209      # atomic mass unit in electron masses (CODATA 2018)


KB_HARTREE = 3.166811563e-6   # Boltzmann constant in Hartree / K


def _vv_drift(R, v, a, dt):
    """Velocity-Verlet position update (any leading axes: one or many trajectories)."""
    return R + dt * v + 0.5 * dt * dt * a


def _vv_kick(v, a, g, m, dt):
    """Velocity-Verlet velocity update from the start acceleration ``a`` and the end-point gradient ``g``."""
    return v + 0.5 * dt * (a - np.asarray(g) / m)


def nve_velocity_verlet(scanner, init_mol, dt=10.0, steps=10, veloc=None, trajectory_output=None,
                        energy_output=None, callback=None, thermostat=None):
    """Velocity-Verlet NVE propagation of an array-level molecule with ``scanner(mol) -> (E, grad)``.
    Returns one frame per step: ``{"coord", "veloc", "epot", "ekin", "time"}`` (frame 0 = initial geometry);
    the force of a step's end point is reused as the next step's start, so there is exactly one
    energy+force evaluation per step.

    ``callback(locals())`` is called after every frame with ``mol`` and ``scanner`` among the keys, as PySCF's
    integrators do (``04_Zundel_continuation_MD.py:140-177`` reads ``locals["scanner"].base.predicted_one_rdm``);
    ``thermostat=(T_kelvin, taut)`` rescales the velocities after every step like ``md.integrators.NVTBerendson``."""
    R = np.array(init_mol.atom_coords(), dtype=np.float64)
    m = (np.asarray(init_mol.atom_mass_list(), dtype=np.float64) * AMU2AU)[:, None]
    v = np.zeros_like(R) if veloc is None else np.array(veloc, dtype=np.float64)
    mol = init_mol
    e, g = scanner(mol)
    frames = []
    fe = open(energy_output, "w") if isinstance(energy_output, str) else energy_output
    ft = open(trajectory_output, "w") if isinstance(trajectory_output, str) else trajectory_output
    for k in range(steps):
        ekin = 0.5 * float(np.sum(m * v * v))
        frames.append({"coord": R.copy(), "veloc": v.copy(), "epot": float(e), "ekin": ekin, "time": k * dt})
        if callable(callback):
            frame, iteration = frames[-1], k   # noqa: F841 (exposed to the callback through locals())
            callback(locals())
        if fe is not None:
            fe.write(f"{k * dt:14.6f} {e:18.10f} {ekin:18.10f} {e + ekin:18.10f}\n")
        if ft is not None:
            ft.write(f"{R.shape[0]}\nMD time {k * dt:.6f} a.u., coordinates in Bohr\n")
            for xyz in R:
                ft.write("H %18.10f %18.10f %18.10f\n" % tuple(xyz))
        if k == steps - 1:
            break
        a = -np.asarray(g) / m
        R = _vv_drift(R, v, a, dt)
        mol = init_mol.with_coords(R)
        e, g = scanner(mol)
        v = _vv_kick(v, a, g, m, dt)
        if thermostat is not None:
            T_target, taut = thermostat
            T_now = float(np.sum(m * v * v)) / (3 * R.shape[0] * KB_HARTREE)
            if T_now > 0.0:
                v = v * np.sqrt(1.0 + (T_target / T_now - 1.0) * dt / taut)
    for f, given in ((fe, energy_output), (ft, trajectory_output)):
        if f is not None and isinstance(given, str):
            f.close()
    return frames


def converge_EVCont_MD(EVCont_obj, init_mol, steps=100, dt=1, convergence_thresh=1.0e-3,
                       prune_irrelevant_data=False, trn_times=[], data_addition="farthest_point_ham", **kwargs):
    """Active-learning driver (reference :128-502): see ``evcont_amd.active_learning.converge_EVCont_MD``,
    which evaluates the loop's re-evaluation and selection steps as batched device calls."""
    from .active_learning import converge_EVCont_MD as _impl
    return _impl(EVCont_obj, init_mol, steps=steps, dt=dt, convergence_thresh=convergence_thresh,
                 prune_irrelevant_data=prune_irrelevant_data, trn_times=list(trn_times),
                 data_addition=data_addition, **kwargs)


def _device_producer(mol0):
    """The device integral producer class of an array-level molecule: molecules of s and p shells
    (gto_small.GaussianMol), of s, p and d shells (gto_spd.SpdGaussianMol), of shells up to f
    (gto_spdf.SpdfGaussianMol) and of one s function per centre (hchain.HChainMol)."""
    if getattr(mol0, "shells", None) is not None and hasattr(mol0, "charges"):
        if any(sh.l == 3 for atom in mol0.shells for sh in atom):
            # f shells (gto_spdf.SpdfGaussianMol): csrc/spdfgto.hip
            from .gto_spdf_device import DeviceSpdfGaussians as producer
        elif any(sh.l == 2 for atom in mol0.shells for sh in atom):
            # d shells (gto_spd.SpdGaussianMol): the general route, csrc/spdgto.hip
            from .gto_spd_device import DeviceSpdGaussians as producer
        else:
            from .gto_device import DeviceGaussians as producer
    elif all(hasattr(mol0, k) for k in ("charges", "exponents", "coefficients")):
        from .hchain_device import DeviceSGaussians as producer
    else:
        raise ValueError('integrals="device" needs s-Gaussian molecules (evcont_amd.hchain.HChainMol)')
    return producer


def _device_surfaces(mols, one_rdm, two_rdm, overlap, nroots, observables=(), device_trdms=None,
                     field_origin=(0.0, 0.0, 0.0)):
    """``evaluate(R (G,A,3)) -> (E (G,nroots), grads (G,nroots,A,3))`` for geometries of the s-Gaussian molecule of
    ``mols``, device-resident from the coordinates on: the training set and the batched evaluator are built once, every
    call uploads the coordinates, computes the AO integrals there (``hchain_device.DeviceSGaussians``, or
    ``gto_device.DeviceGaussians`` for a molecule with ``shells``, ``gto_spd_device.DeviceSpdGaussians`` when the
    shells contain l = 2, ``gto_spdf_device.DeviceSpdfGaussians`` when they contain l = 3) and runs the
    batched several-roots call on them.  With ``observables``: ``(E, grads (G,1,A,3), props)`` of the highest root alone,
    forces and observables from one solve (``BatchedEvaluator.multistate_properties``).  ``evaluate(R, field)``: the
    geometries in the uniform electric fields ``field`` ((3,) or (G,3)) with the origin ``field_origin``, folded into the
    integrals on the device (``integrals(..., field=)`` of the producer)."""
    from .ab_initio_eigenvector_continuation import resolve_compression
    from .ab_initio_gradients_loewdin import _batched_evaluator
    mol0, G = mols[0], len(mols)
    producer = _device_producer(mol0)
    if G * nroots > 4096:
        raise ValueError(f"{G} trajectories x {nroots} roots exceed the 4096 slots of one call")
    t = device_trdms if device_trdms is not None else _resident_trdms(
        one_rdm, two_rdm, overlap,
        resolve_compression("default", one_rdm, two_rdm, overlap, ao_arrays(mol0, need_grad=True)))
    natm = int(np.asarray(mol0.charges).shape[0])
    ev = _batched_evaluator(t, natm, G)
    sg = producer.from_mol(mol0, device=t.device)
    packed = t.layout == _lib.LAYOUT_SYM8 and t.n <= 64

    def evaluate(R, field=None):
        aob = sg.integrals(R, packed=packed) if field is None else \
            sg.integrals(R, packed=packed, field=field, origin=field_origin)
        if not observables:
            E, _, grads = ev.multistate_energies_with_grads(aob, nroots)
            return E, grads
        # the dipole integrals from the coordinates the call above left on the device: no second upload, and the step's
        # download grows by the observables of the propagated root alone
        Rd = sg.staged_coords(G)
        root = nroots - 1
        E, _, props, grads = ev.multistate_properties(
            aob, nroots, [(root, root)], dip=sg.dipole_integrals(Rd) if "dipole" in observables else None,
            charges=sg.charges, coords=Rd, return_forces=True, observables=observables)
        return E, grads, props

    return evaluate


_OBSERVABLES = {"dipole": "dipole", "mulliken": "mulliken_charges", "loewdin": "loewdin_charges"}


def state_swarm(mols, one_rdm, two_rdm, overlap, root, dt=10.0, steps=10, init_veloc=None, integrals="host",
                observables=None, device_trdms=None, field=None, field_origin=(0.0, 0.0, 0.0)):
    """Velocity-Verlet NVE of G trajectories on the continuation surface ``root`` (0 = ground state), advanced in lock
    step: every step is ONE batched call for all G geometries (``get_multistate_energies_with_grads``, all trajectories'
    roots 0 .. root in one pass).  ``mols``: the G initial geometries of one array-level molecule that can be rebuilt at
    new coordinates (``with_coords``, as ``get_trajectory``'s native path takes); ``init_veloc``: (G,A,3) or None.
    Conventions of ``nve_velocity_verlet`` (Bohr, atomic time units, frame 0 = the initial geometries); returns one
    frame per step with ``coord``/``veloc`` (G,A,3), ``epot``/``ekin`` (G,) and ``time``.  Plain adiabatic dynamics:
    no surface hopping, and at (near-)degenerate roots the forces follow whichever eigenvector the solver returned.
    ``integrals``: "host" rebuilds every molecule with ``with_coords`` (numpy) at every step; "device" (s-Gaussian
    molecules, ``evcont_amd.hchain``, molecules of s and p shells, ``evcont_amd.gto_small``, or of s, p and d shells,
    ``evcont_amd.gto_spd``) uploads the (G,A,3)
    coordinates and computes the AO integrals on the device.
    ``observables``: None (the frames above, nothing else) or a selection of "dipole", "mulliken", "loewdin": every frame
    gains ``dipole`` (G,3) (atomic units, origin (0,0,0)) and ``mulliken_charges`` / ``loewdin_charges`` (G,A) of the
    propagated root (plain Mulliken, not meta-Loewdin), from the solve that gives the forces; with
    ``integrals="device"`` that adds the observables' G (3 + A) doubles per kind of charge to the step's download and
    no upload.
    ``device_trdms``: as for ``get_scanner`` (training data already on the device, e.g. a resident container's
    ``device_trdms()``; the host arrays may then be ``None``).
    ``field``: None, or a uniform electric field in atomic units, (3,) for all trajectories or (G,3), or a callable
    ``time -> `` either (a pulse); ``field_origin``: the origin of the dipole operator.  ``mols`` are then the field-free
    molecules; every step's geometries are put into the field of the step's time (``with_field`` on the host route,
    ``integrals(..., field=)`` of the device producer on the device route), ``epot`` of a frame includes the field
    terms, and a static field conserves ``epot + ekin``."""
    from .ab_initio_gradients_loewdin import get_multistate_energies_with_grads
    mols = list(mols)
    root = int(root)
    if root < 0:
        raise ValueError(f"root={root} must be >= 0")
    if integrals not in ("host", "device"):
        raise ValueError(f"unknown integrals={integrals!r} (known: 'host', 'device')")
    R = np.array([m_.atom_coords() for m_ in mols], dtype=np.float64)
    m = (np.asarray(mols[0].atom_mass_list(), dtype=np.float64) * AMU2AU)[:, None]
    v = np.zeros_like(R) if init_veloc is None else np.array(init_veloc, dtype=np.float64).reshape(R.shape)

    observables = tuple(observables or ())
    if set(observables) - set(_OBSERVABLES):
        raise ValueError(f"unknown observables {observables!r} (known: {sorted(_OBSERVABLES)})")
    # frame key -> (G, ...) array of the propagated root
    observed = lambda props: {_OBSERVABLES[k]: props[_OBSERVABLES[k]][:, 0] for k in observables}

    def field_at(time):
        """(G,3) fields of the step at ``time``, or None."""
        if field is None:
            return None
        F = np.asarray(field(time) if callable(field) else field, dtype=np.float64)
        return np.ascontiguousarray(np.broadcast_to(F.reshape(1, 3), (len(mols), 3)) if F.size == 3
                                    else F.reshape(len(mols), 3))

    if integrals == "device":
        surfaces = _device_surfaces(mols, one_rdm, two_rdm, overlap, root + 1, observables, device_trdms, field_origin)

        def evaluate(ms, time):
            F = field_at(time)
            if observables:
                E, grads, props = surfaces(R, F)
                return E[:, root], grads[:, 0], observed(props)
            E, grads = surfaces(R, F)
            return E[:, root], grads[:, root], {}

        rebuild = lambda ms, R: ms
    else:
        def evaluate(ms, time):
            F = field_at(time)
            if F is not None:
                ms = [m_.with_field(f, field_origin) for m_, f in zip(ms, F)]
            if observables:
                from .ab_initio_eigenvector_continuation import get_multistate_properties
                E, props = get_multistate_properties(ms, one_rdm, two_rdm, overlap, root + 1, [(root, root)],
                                                     return_forces=True, device_trdms=device_trdms)
                return E[:, root], props["grads"][:, 0], observed(props)
            E, grads = get_multistate_energies_with_grads(ms, one_rdm, two_rdm, overlap, root + 1,
                                                          device_trdms=device_trdms)
            return E[:, root], grads[:, root], {}

        rebuild = lambda ms, R: [m_.with_coords(r) for m_, r in zip(ms, R)]

    e, g, obs = evaluate(mols, 0.0)
    frames = []
    for k in range(steps):
        frames.append({"coord": R.copy(), "veloc": v.copy(), "epot": e.copy(),
                       "ekin": 0.5 * np.sum(m * v * v, axis=(1, 2)), "time": k * dt, **obs})
        if k == steps - 1:
            break
        a = -g / m
        R = _vv_drift(R, v, a, dt)
        mols = rebuild(mols, R)
        e, g, obs = evaluate(mols, (k + 1) * dt)
        v = _vv_kick(v, a, g, m, dt)
    return frames
