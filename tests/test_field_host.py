"""Host statements of a molecule in a uniform electric field (evcont_amd/field.py, ``dipole_grad_integrals`` and
``with_field`` of HChainMol / GaussianMol / SpdGaussianMol) and the host side of csrc/field.hip.  No device.

* ``ipdip[x,c] + ipdip[x,c]^T = -delta_xc S`` and the translation rule, to 1e-12 of the array's scale: sign, index order
  and d normalisation tied to arrays that are pinned to exact values elsewhere.
* ``ipdip`` against Richardson-combined central differences of the independent ``dipole_integrals`` over one moved atom.
* ``with_field`` through the numpy oracle (H4, three SmallFCI training states): dE/dF = -dipole (Hellmann-Feynman),
  forces in a field = -dE/dR.
* the sum rule of the atomic polar tensor and the symmetry of the polarisability, with the field points and the assembly
  of ``get_multistate_field_response`` (``field_points``, ``field_response_from_points``) on oracle energies, dipoles
  and forces.  The function itself runs the device evaluator on both of its routes; tests/test_gpu_field.py holds it to
  the same rule.
* closure of csrc/field.hip in the style of tests/test_properties_closure.py.

Tolerances of the finite-difference checks: the rule is |FD(h) - FD(h/2)| measured here on the CPU, times 10 (the
truncation error falls 4x per halving, so the Richardson value is far inside).  Measured (``python
tests/test_field_host.py``), worst over the elements and the moved coordinates:

    check                                      h      |FD(h) - FD(h/2)|   tolerance   |Richardson - analytic|
    ipdip, bent H3 (STO-3G s)                  2e-3   2.23e-7             2.3e-6      1.4e-13
    ipdip, s + p (moderate exponents)          2e-3   1.96e-7             2.0e-6      1.3e-13
    ipdip, s + p + d (O-H, d exponent 0.8)     2e-3   1.12e-6             1.2e-5      5.1e-13
    dE/dF against -dipole, roots 0 and 1       2e-3   4.31e-8             4.4e-7      1.7e-10
    forces in a field against -dE/dR           2e-3   2.82e-7             2.9e-6      3.7e-12
    alpha - alpha^T (truncation, no limit 0)   1e-3   |alpha(h) - alpha(h/2)| = 7.0e-9 -> 7.1e-8; asymmetry 2.4e-9

The sum rule is linear in F, so the central difference has no truncation error: it holds to the rounding of the forces
divided by h.  The forces are good to 1e-13 (the accuracy the response function's docstring states for the chain), so the
bound is 1e-13 / h = 1e-10 at h = 1e-3; measured 4e-13.
"""
import os
import re

import numpy as np
import pytest

from evcont_amd import gto_small, gto_spd, hchain
from evcont_amd import properties as pr
from evcont_amd.ab_initio_eigenvector_continuation import field_points, field_response_from_points
from evcont_amd.field import dipole_derivative
from oracle import evcont_oracle as orc
from test_hchain_physics import bundle, chain, train

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "evcont_amd", "csrc")
CALLS = ("evc_sgto_dipole_grad_batch", "evc_gto_dipole_grad_batch", "evc_field_fold_batch")
KERNELS = {"field_sgrad_kernel", "field_grad_kernel", "field_fold_kernel"}
ORIGIN = (0.3, -0.2, 0.1)
H4_COORDS = np.array([[0.0, 0.0, 0.0], [1.7, 0.3, 0.0], [2.9, 1.6, 0.4], [4.4, 1.9, -0.7]])
H4_ORIGIN = (0.2, -0.1, 0.3)
OH_COORDS = np.array([[0.0, 0.0, 0.0], [0.4, 1.5, 0.7]])


def bent_h3():
    return hchain.s_gaussian_mol(np.array([[0.0, 0.0, 0.0], [1.7, 0.2, 0.0], [2.5, 1.5, 0.4]]), need_grad=False)


def sp_molecule():
    """O-H of s and p shells with moderate exponents (a tight core function makes finite differences meaningless)."""
    sh = gto_small.Shell
    return gto_small.sp_gaussian_mol(OH_COORDS, [8, 1], [[sh(0, (1.1, 0.4), (0.5, 0.6)), sh(1, (0.9, 0.3), (0.6, 0.5))],
                                                         [sh(0, (0.7, 0.25), (0.5, 0.6))]], need_grad=False)


def spd_molecule():
    """O-H with one d shell of moderate exponent."""
    sh = gto_spd.Shell
    return gto_spd.spd_gaussian_mol(OH_COORDS, [8, 1], [[sh(0, (1.1, 0.4), (0.5, 0.6)), sh(1, (0.9,), (1.0,)),
                                                         sh(2, (0.8,), (1.0,))],
                                                        [sh(0, (0.7, 0.25), (0.5, 0.6)), sh(1, (0.6,), (1.0,))]],
                                    need_grad=False)


MOLECULES = {"h3": bent_h3, "water_sto3g": lambda: gto_small.water("sto-3g", need_grad=False), "spd": spd_molecule}
# name -> (molecule, h, tolerance = 10 x the measured |FD(h) - FD(h/2)| of the header)
FD_CASES = {"h3": (bent_h3, 2e-3, 2.3e-6), "sp": (sp_molecule, 2e-3, 2.0e-6), "spd": (spd_molecule, 2e-3, 1.2e-5)}


@pytest.mark.parametrize("name", sorted(MOLECULES))
def test_exact_identity_and_translation(name):
    mol = MOLECULES[name]()
    ip = mol.dipole_grad_integrals(ORIGIN)
    n = mol.nao
    assert ip.shape == (3, 3, n, n)
    scale = np.abs(ip).max()
    assert scale > 0.1
    # <d_x mu| r_c |nu> + <mu| r_c |d_x nu> = -<mu| d_x r_c |nu> = -delta_xc S
    for x in range(3):
        for c in range(3):
            want = -mol.S if x == c else np.zeros((n, n))
            assert np.abs(ip[x, c] + ip[x, c].T - want).max() < 1e-12 * scale, (x, c)
    # all atoms moved together: d dip_c / dt_x = delta_xc S, and the finite translation changes dip_c by t_c S exactly
    total = dipole_derivative(ip, mol.aoslices).sum(axis=0)
    for x in range(3):
        for c in range(3):
            want = mol.S if x == c else np.zeros((n, n))
            assert np.abs(total[x, c] - want).max() < 1e-12 * scale, (x, c)
    t = np.array([0.37, -0.61, 0.23])
    moved = mol.with_coords(mol.coords + t, need_grad=False)
    d0, d1 = mol.dipole_integrals(ORIGIN), moved.dipole_integrals(ORIGIN)
    assert np.abs(d1 - d0 - t[:, None, None] * mol.S[None]).max() < 1e-12 * max(1.0, np.abs(d1).max())
    # the origin enters through the operator alone: ipdip(O) = ipdip(0) - O_c ipovlp
    ip0 = mol.dipole_grad_integrals()
    full = mol.with_coords(mol.coords)
    shift = ip0 - np.asarray(ORIGIN)[None, :, None, None] * full.ipovlp[:, None]
    assert np.abs(ip - shift).max() < 1e-12 * scale


def fd_dipole(mol, at, x, h):
    Rp, Rm = mol.coords.copy(), mol.coords.copy()
    Rp[at, x] += h
    Rm[at, x] -= h
    return (mol.with_coords(Rp, need_grad=False).dipole_integrals(ORIGIN)
            - mol.with_coords(Rm, need_grad=False).dipole_integrals(ORIGIN)) / (2.0 * h)


def measure_ipdip(name):
    make, h, _ = FD_CASES[name]
    mol = make()
    an = dipole_derivative(mol.dipole_grad_integrals(ORIGIN), mol.aoslices)
    gap = err = 0.0
    for at, x in ((0, 0), (1, 1), (mol.natm - 1, 2)):
        a, b = fd_dipole(mol, at, x, h), fd_dipole(mol, at, x, h / 2)
        gap = max(gap, np.abs(a - b).max())
        err = max(err, np.abs((4.0 * b - a) / 3.0 - an[at, x]).max())
    return gap, err


@pytest.mark.parametrize("name", sorted(FD_CASES))
def test_against_central_differences_of_the_dipole_integrals(name):
    gap, err = measure_ipdip(name)
    tol = FD_CASES[name][2]
    print(f"{name}: |FD(h) - FD(h/2)| = {gap:.3e}, |Richardson - analytic| = {err:.3e}, tolerance {tol:.1e}")
    assert gap < tol / 5.0           # the measurement the tolerance came from still describes this run
    assert err < tol


@pytest.fixture(scope="module")
def h4_training():
    S, one, two, _ = train([chain(4, d) for d in (1.5, 2.0, 2.8)])
    return S, one, two


def oracle_energies(mol, tr, nroots=2):
    S, one, two = tr
    return orc.approximate_multistate_OAO(bundle(mol), one, two, S, nroots)


def host_dipoles(mol, tr, C, origin):
    return pr.properties_host(tr[1], orc.loewdin_trafo(mol.S), C, [(k, k) for k in range(len(C))], mol.S,
                              mol.dipole_integrals(origin), mol.aoslices, mol.charges, mol.coords, origin)["dipole"]


def measure_hellmann_feynman(tr, h=2e-3):
    mol = hchain.s_gaussian_mol(H4_COORDS)
    _, C = oracle_energies(mol, tr)
    want = -host_dipoles(mol, tr, C, H4_ORIGIN)

    def fd(h):
        out = np.zeros((2, 3))
        for c in range(3):
            F = np.zeros(3)
            F[c] = h
            out[:, c] = (oracle_energies(mol.with_field(F, H4_ORIGIN), tr)[0]
                         - oracle_energies(mol.with_field(-F, H4_ORIGIN), tr)[0]) / (2.0 * h)
        return out

    a, b = fd(h), fd(h / 2)
    return np.abs(a - b).max(), np.abs((4.0 * b - a) / 3.0 - want).max(), want


def test_with_field_energy_derivative_is_minus_the_dipole(h4_training):
    gap, err, want = measure_hellmann_feynman(h4_training)
    print(f"dE/dF: |FD(h) - FD(h/2)| = {gap:.3e}, |Richardson + dipole| = {err:.3e}")
    assert np.abs(want).max() > 0.1
    assert gap < 4.4e-7 / 5.0 and err < 4.4e-7


def measure_forces(tr, h=2e-3):
    S, one, two = tr
    mf = hchain.s_gaussian_mol(H4_COORDS).with_field((0.01, -0.02, 0.015), H4_ORIGIN)
    _, g = orc.energy_with_grad(bundle(mf), one, two, S)
    picks = ((0, 0), (1, 2), (3, 1))

    def fd(h):
        out = []
        for at, x in picks:
            Rp, Rm = H4_COORDS.copy(), H4_COORDS.copy()
            Rp[at, x] += h
            Rm[at, x] -= h
            out.append((orc.energy_with_grad(bundle(mf.with_coords(Rp)), one, two, S)[0]
                        - orc.energy_with_grad(bundle(mf.with_coords(Rm)), one, two, S)[0]) / (2.0 * h))
        return np.array(out)

    a, b = fd(h), fd(h / 2)
    return np.abs(a - b).max(), np.abs((4.0 * b - a) / 3.0 - np.array([g[at, x] for at, x in picks])).max()


def test_with_field_forces_are_the_gradient_of_the_energy(h4_training):
    gap, err = measure_forces(h4_training)
    print(f"forces in a field: |FD(h) - FD(h/2)| = {gap:.3e}, |Richardson - analytic| = {err:.3e}")
    assert gap < 2.9e-6 / 5.0 and err < 2.9e-6


def test_with_field_records_replaces_and_follows_the_coordinates():
    mol = hchain.s_gaussian_mol(H4_COORDS, (1.0, 2.0, 0.5, 1.0))
    F = np.array([0.01, -0.02, 0.005])
    mf = mol.with_field(F, H4_ORIGIN)
    assert np.array_equal(mf.field, F) and mf.field_origin == H4_ORIGIN and mol.field is None
    assert np.array_equal(mf.S, mol.S) and np.array_equal(mf.eri, mol.eri) and np.array_equal(mf.ipovlp, mol.ipovlp)
    np.testing.assert_allclose(mf.hcore - mol.hcore, np.einsum("c,cij->ij", F, mol.dipole_integrals(H4_ORIGIN)), atol=1e-15)
    np.testing.assert_allclose(mf.enuc - mol.enuc, -mol.charges @ ((H4_COORDS - np.array(H4_ORIGIN)) @ F), atol=1e-14)
    np.testing.assert_allclose(mf.gnuc - mol.gnuc, -np.outer(mol.charges, F), atol=1e-15)
    add = mf.dhcore - mol.dhcore
    assert np.array_equal(mf.hcore, mf.hcore.T) and np.abs(add - add.transpose(0, 1, 3, 2)).max() < 1e-16
    # with_coords stays in the field; a second with_field replaces the first
    again = mf.with_coords(H4_COORDS)
    assert np.array_equal(again.field, F) and np.array_equal(again.hcore, mf.hcore)
    assert np.array_equal(again.dhcore, mf.dhcore)
    off = mf.with_field((0.0, 0.0, 0.0))
    assert np.abs(off.hcore - mol.hcore).max() < 1e-15 and np.abs(off.dhcore - mol.dhcore).max() < 1e-15
    # without gradients only hcore and enuc change
    bare = hchain.s_gaussian_mol(H4_COORDS, need_grad=False)
    bf = bare.with_field(F)
    assert np.array_equal(bf.dhcore, bare.dhcore) and np.array_equal(bf.gnuc, bare.gnuc)
    assert not np.array_equal(bf.hcore, bare.hcore)
    for make in (sp_molecule, spd_molecule):
        m = make()
        m = m.with_coords(m.coords)          # with gradients
        mf = m.with_field(F, ORIGIN)
        np.testing.assert_allclose(mf.dhcore - m.dhcore, np.einsum(
            "c,axcij->axij", F, dipole_derivative(m.dipole_grad_integrals(ORIGIN), m.aoslices)), atol=1e-15)
        assert np.array_equal(mf.with_coords(m.coords).hcore, mf.hcore)


def oracle_response(charges, tr, h):
    """``field_response_from_points`` on oracle energies, dipoles and forces of root 0 at ``field_points(h)``."""
    S, one, two = tr
    mol = hchain.s_gaussian_mol(H4_COORDS, charges=charges, nelec=(2, 2))
    E, D, G = [], [], []
    for F in field_points(h):
        m = mol.with_field(F, H4_ORIGIN) if F.any() else mol
        e, g = orc.energy_with_grad(bundle(m), one, two, S)
        _, C = oracle_energies(m, tr, 1)
        E.append([e])
        D.append(host_dipoles(m, tr, C, H4_ORIGIN))
        G.append(g[None])
    return field_response_from_points(E, D, G, h)


@pytest.mark.parametrize("charges", [(1.0, 1.0, 1.0, 1.0), (1.0, 2.0, 1.0, 1.0)])
def test_sum_rule_and_symmetric_polarisability(h4_training, charges):
    h = 1e-3
    r, r2 = oracle_response(charges, h4_training, h), oracle_response(charges, h4_training, h / 2)
    assert r["apt"].shape == (1, 4, 3, 3) and r["polarizability"].shape == (1, 3, 3) and r["dipole"].shape == (1, 3)
    Q = sum(charges) - 4.0
    worst = np.abs(r["apt"][0].sum(axis=0) - Q * np.eye(3)).max()
    alpha, gap = r["polarizability"][0], np.abs(r["polarizability"][0] - r2["polarizability"][0]).max()
    asym = np.abs(alpha - alpha.T).max()
    print(f"Q = {Q}: sum rule {worst:.2e}, alpha asymmetry {asym:.2e}, |alpha(h) - alpha(h/2)| = {gap:.2e}")
    assert worst < 1e-13 / h
    assert gap < 7.1e-8 / 5.0 and asym < 7.1e-8
    # three training states span the response: the ground state is polarisable in at most two directions
    assert np.linalg.eigvalsh(0.5 * (alpha + alpha.T))[-1] > 0.1


def test_ir_intensities():
    rng = np.random.default_rng(4)
    apt, m = rng.standard_normal((3, 3, 3)), np.array([16.0, 1.0, 1.0])
    L = np.linalg.qr(rng.standard_normal((9, 9)))[0]
    got = pr.ir_intensities(apt, L[:, :4], m)
    want = [np.sum((apt.reshape(9, 3).T @ (L[:, k] / np.sqrt(np.repeat(m, 3)))) ** 2) for k in range(4)]
    np.testing.assert_allclose(got, want, rtol=1e-14)
    # a rigid translation of a neutral molecule obeying the sum rule is dark
    apt0 = apt - apt.mean(axis=0)
    t = np.zeros((3, 3))
    t[:, 0] = np.sqrt(m)
    assert pr.ir_intensities(apt0, t.reshape(9, 1) / np.linalg.norm(t), m)[0] < 1e-28


# ---- closure of csrc/field.hip ------------------------------------------------------------------
def source(name="field.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def header():
    with open(os.path.join(REPO, "include", "evcont_hip.h")) as f:
        return f.read()


def test_calls_are_declared_bound_and_built():
    from evcont_amd import _lib, build
    build.build()
    lib = _lib.load()
    hdr = header()
    for name in CALLS:
        assert f"{name}(" in hdr, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name in hdr[:hdr.index("#define EVC_LAYOUT_FULL6")], "listed as additive in the ABI comment"
    assert _lib.SIGNATURES["evc_sgto_dipole_grad_batch"] == _lib.SIGNATURES["evc_sgto_dipole_batch"]
    assert _lib.SIGNATURES["evc_gto_dipole_grad_batch"] == _lib.SIGNATURES["evc_spdgto_dipole_batch"]
    assert "field.hip" in build.SOURCES


def test_every_kernel_is_launched_through_gto_launch_and_nothing_is_shared_between_threads():
    src = source()
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src))
    launched = set(re.findall(r"\bgto_launch\(\s*(\w+)\s*,", src))
    assert defined == launched == KERNELS, sorted(defined ^ launched)
    assert "<<<" not in src and "hipLaunchKernelGGL" not in src and "hipLaunchKernel(" not in src
    assert "atomic" not in src.lower() and "hipMalloc" not in src and "__shared__" not in src
    # the monomials of the d functions are shared with spdgto.hip, not copied
    assert "spd_mono(" in src and "void spd_mono(" not in src and "void spd_mono(" not in source("spdgto.hip")
    assert "void spd_mono(" in source("gto_shells.hpp")


def test_no_new_profile_stage_and_no_new_abi_version():
    from evcont_amd import _lib
    assert re.search(r"constexpr int kProfStages = 14;", source("pipeline.hpp"))
    assert re.search(r"#define\s+EVC_ABI_VERSION\s+10\b", header())
    assert _lib.ABI_VERSION == 10
    assert "note_kernel" not in source() and "EVC_PROF_" not in source()


def test_refusals_need_no_device():
    """Every refused argument is caught on the host, before anything is launched: rc < 0 and a message that starts with
    the function's name.  Placeholder pointers: nothing is dereferenced on the device side."""
    from evcont_amd import _lib, build
    build.build()
    lib = _lib.load()
    i32 = lambda *v: np.array(v, dtype=np.int32)
    f64 = lambda *v: np.array(v, dtype=np.float64)
    ptr = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)
    org = f64(0.0, 0.0, 0.0)

    def refused(rc, who, word, what):
        msg = lib.evc_last_error()
        assert rc < 0 and msg.startswith(who) and word in msg, (what, rc, msg)

    # evc_sgto_dipole_grad_batch: the limits and refusals of evc_sgto_dipole_batch
    ex, co = f64(3.42525091, 0.62391373, 0.16885540), f64(0.15432897, 0.53532814, 0.44463454)
    good = dict(natm=4, nprim=3, count=2, coords=256, ex=ex, co=co, origin=org, out=256)

    def sgrad(**kw):
        a = dict(good, **kw)
        return lib.evc_sgto_dipole_grad_batch(a["natm"], a["nprim"], a["count"], a["coords"], ptr(a["ex"]), ptr(a["co"]),
                                              ptr(a["origin"]), a["out"], None)

    for kw, word in ((dict(natm=0), b"natm"), (dict(natm=97), b"natm"), (dict(nprim=0), b"nprim"), (dict(nprim=9), b"nprim"),
                     (dict(count=0), b"count"), (dict(count=65536), b"count"), (dict(coords=None), b"null"),
                     (dict(ex=None), b"null"), (dict(co=None), b"null"), (dict(origin=None), b"null"),
                     (dict(out=None), b"null"), (dict(ex=f64(3.4, 0.0, 0.1)), b"exponent"),
                     (dict(ex=f64(3.4, -1.0, 0.1)), b"exponent"), (dict(out=260), b"misaligned")):
        refused(sgrad(**kw), b"evc_sgto_dipole_grad_batch", word, kw)

    # evc_gto_dipole_grad_batch: those of evc_spdgto_dipole_batch; water-like: O with s(3), p(3), d(3); two H with s(3)
    sa, sl, so = i32(0, 0, 0, 1, 2), i32(0, 1, 2, 0, 0), i32(0, 3, 6, 9, 12, 15)
    gex, gco = f64(*([3.4, 0.6, 0.2] * 5)), f64(*([0.2, 0.5, 0.4] * 5))
    good = dict(natm=3, nshell=5, count=2, coords=256, sa=sa, sl=sl, so=so, ex=gex, co=gco, origin=org, out=256)

    def ggrad(**kw):
        a = dict(good, **kw)
        return lib.evc_gto_dipole_grad_batch(a["natm"], a["nshell"], a["count"], a["coords"], ptr(a["sa"]), ptr(a["sl"]),
                                             ptr(a["so"]), ptr(a["ex"]), ptr(a["co"]), ptr(a["origin"]), a["out"], None)

    wide = 13                                     # 13 d shells: 65 functions
    for kw, word in ((dict(natm=0), b"natm"), (dict(natm=65), b"natm"), (dict(nshell=0), b"nshell"),
                     (dict(nshell=65), b"nshell"), (dict(count=0), b"count"), (dict(count=65536), b"count"),
                     (dict(coords=None), b"null"), (dict(sa=None), b"null"), (dict(sl=None), b"null"),
                     (dict(so=None), b"null"), (dict(ex=None), b"null"), (dict(co=None), b"null"),
                     (dict(origin=None), b"null"), (dict(out=None), b"null"),
                     (dict(sl=i32(0, 1, 3, 0, 0)), b"l=3"), (dict(sl=i32(0, -1, 1, 0, 0)), b"l=-1"),
                     (dict(sa=i32(0, 0, 0, 1, 3)), b"shell_atom"), (dict(sa=i32(0, 1, 0, 1, 2)), b"ascending"),
                     (dict(so=i32(1, 3, 6, 9, 12, 15)), b"shell_prim_offset"),
                     (dict(so=i32(0, 9, 10, 11, 12, 13)), b"primitives"),
                     (dict(nshell=wide, natm=wide, sa=i32(*range(wide)), sl=i32(*([2] * wide)), so=i32(*range(wide + 1)),
                           ex=f64(*([1.0] * wide)), co=f64(*([1.0] * wide))), b"nao=65"),
                     (dict(ex=f64(*([3.4, 0.0, 0.2] * 5))), b"exponent"), (dict(ex=f64(*([3.4, -1.0, 0.2] * 5))), b"exponent"),
                     (dict(out=260), b"misaligned")):
        refused(ggrad(**kw), b"evc_gto_dipole_grad_batch", word, kw)

    # evc_field_fold_batch
    good = dict(n=7, natm=3, count=2, dip=256, ipdip=256, aoslices=256, charges=256, coords=256, field=256, origin=org,
                flags=0, hcore=256, dhcore=256, enuc=256, gnuc=256)

    def fold(**kw):
        a = dict(good, **kw)
        return lib.evc_field_fold_batch(a["n"], a["natm"], a["count"], a["dip"], a["ipdip"], a["aoslices"], a["charges"],
                                        a["coords"], a["field"], ptr(a["origin"]), a["flags"], a["hcore"], a["dhcore"],
                                        a["enuc"], a["gnuc"], None)

    cases = [(dict(n=0), b"n=0"), (dict(n=97), b"n=97"), (dict(natm=0), b"natm"), (dict(natm=65536), b"natm"),
             (dict(count=0), b"count"), (dict(count=65536), b"count"), (dict(flags=2), b"flags"), (dict(flags=8), b"flags"),
             (dict(flags=_lib.FLAG_ENERGY_ONLY | _lib.FLAG_ERI_S4), b"flags"), (dict(hcore=260), b"misaligned"),
             (dict(field=260), b"misaligned"), (dict(dhcore=260), b"misaligned")]
    cases += [({k: None}, b"null") for k in ("dip", "charges", "coords", "field", "origin", "hcore", "enuc", "ipdip",
                                             "aoslices", "dhcore", "gnuc")]
    for kw, word in cases:
        refused(fold(**kw), b"evc_field_fold_batch", word, kw)
    # with EVC_FLAG_ENERGY_ONLY the gradient arrays may be absent: the next thing wrong is what is refused
    rc = fold(flags=_lib.FLAG_ENERGY_ONLY, ipdip=None, aoslices=None, dhcore=None, gnuc=None, n=0)
    refused(rc, b"evc_field_fold_batch", b"n=0", "energy only")
    refused(fold(flags=_lib.FLAG_ENERGY_ONLY, dip=None), b"evc_field_fold_batch", b"null", "energy only, dip")


if __name__ == "__main__":
    for name in sorted(FD_CASES):
        print(name, "gap %.3e  err %.3e" % measure_ipdip(name))
    tr = train([chain(4, d) for d in (1.5, 2.0, 2.8)])[:3]
    print("dE/dF gap %.3e err %.3e" % measure_hellmann_feynman(tr)[:2])
    print("forces gap %.3e err %.3e" % measure_forces(tr))
    for Z in ((1.0, 1.0, 1.0, 1.0), (1.0, 2.0, 1.0, 1.0)):
        a, b = oracle_response(Z, tr, 1e-3), oracle_response(Z, tr, 5e-4)
        al = a["polarizability"][0]
        print(Z, "sum rule %.2e  asym %.2e  |alpha(h) - alpha(h/2)| %.2e" % (
            np.abs(a["apt"][0].sum(axis=0) - (sum(Z) - 4.0) * np.eye(3)).max(), np.abs(al - al.T).max(),
            np.abs(al - b["polarizability"][0]).max()))
