"""GPU tests of S^2 on device CI vectors (csrc/fci_spin.hip: evc_fci_spin_apply, evc_fci_spin_diag) and of the spin penalty
of ``DeviceFCI(spin_penalty=...)`` on its three eigensolver routes and in the containers.

The entry points are called directly on poisoned, fenced buffers (tests/test_gpu_fci_abi.py ``Fenced``,
tests/test_gpu_fci_davidson.py ``VectorSet``): the vectors are the second rows of two-row sets at the pitch ``dim + 5``, so
their pointers are 8-byte aligned only, the first rows and the gaps hold NaN and must keep it.

Integer data: every term, sum and product by alpha in {1, 1/2} or (k - ss) in quarters is exact, so the device equals
``fci_tables.spin_square_through_tables`` bit for bit.  Random data: against an np.longdouble reference with the
element-wise bound (n_terms + 3) u (|beta out| + |alpha| (|k - ss| |c_I| + sum |c_J|)), u = 2^-53: a sequential sum of
n_terms + 1 terms, one product by alpha and one step for beta out, each rounded once (derived as in
tests/test_gpu_fci_davidson.py)."""
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from evcont_amd.fci_small import SmallFCI, spin_square_vector
from evcont_amd.fci_tables import packed_table, spin_square_through_tables
from evcont_amd.hchain import hydrogen_chain
from test_fci_davidson_host import oao_integrals
from test_fci_spin_closure import SPIN_RECORDS
from test_gpu_fci_abi import library
from test_gpu_fci_davidson import VectorSet, solve_record

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, (1, 0)), (2, (1, 1)), (4, (2, 2)), (5, (3, 2)), (6, (4, 2)), (6, (3, 0)), (8, (4, 4)), (12, (1, 1)),
          (16, (1, 1)), (13, (1, 2)), (16, (2, 2))]
NEW_KERNELS = ("fci_spin_apply_kernel", "fci_spin_diag_kernel")
# a workgroup walks a run of 4 ... 64 alpha strings, by na * ceil(nb / 64) (csrc/fci_spin.hip); the shapes of the table above
# all take runs of 4: one more of these with a second, nearly empty tile, and one with a longer run that does not divide na
MORE_SHAPES = [(12, (6, 2)), (16, (8, 2))]


def workgroups(na, nb):
    tiles = -(-nb // 64)
    run = min(64, 4 * -(-(na * tiles) // 4096))
    return tiles * -(-na // run), run


class Spin:
    """The two entry points on fenced buffers for one shape."""

    def __init__(self, norb, nelec):
        self.mod, self.lib, self.check = library()
        self.dev = torch.device("cuda:0")
        self.norb, self.nelec = norb, nelec
        ta, tb = packed_table(norb, nelec[0]), packed_table(norb, nelec[1])
        self.na, self.nb = ta.shape[0], tb.shape[0]
        self.dim = self.na * self.nb
        self.ld = self.dim + 5
        self.ta, self.tb = torch.from_numpy(ta).to(self.dev), torch.from_numpy(tb).to(self.dev)

    def _second_row(self, vec):
        rows = np.full((2, self.dim), np.nan)
        if vec is not None:
            rows[1] = np.asarray(vec, dtype=np.float64).reshape(-1)
        return VectorSet(self.dim, self.ld, 2, self.dev, rows)

    def apply(self, c, alpha=1.0, ss=0.0, beta=0.0, out0=None):
        C_, O = self._second_row(c), self._second_row(out0)        # out0 None: the output row is NaN before the call
        self.check(self.lib.evc_fci_spin_apply(self.norb, self.na, self.nb, self.ta.data_ptr(), self.tb.data_ptr(),
                                               C_.ptr + 8 * self.ld, alpha, ss, beta, O.ptr + 8 * self.ld, None),
                   "evc_fci_spin_apply")
        torch.cuda.synchronize()
        rec = solve_record()
        assert re.fullmatch(SPIN_RECORDS["evc_fci_spin_apply"], rec), rec
        assert rec.endswith(f" beta={int(beta != 0.0)} tiles={workgroups(self.na, self.nb)[0]}"), rec
        got_c, got = C_.rows(), O.rows()                             # fences and gaps
        assert np.isnan(got[0]).all() and np.isnan(got_c[0]).all()
        assert np.array_equal(got_c[1], np.asarray(c, dtype=np.float64).reshape(-1))
        return got[1].reshape(self.na, self.nb)

    def diag(self, hd0, alpha=1.0, ss=0.0):
        Hd = self._second_row(hd0)
        self.check(self.lib.evc_fci_spin_diag(self.norb, self.na, self.nb, self.ta.data_ptr(), self.tb.data_ptr(), alpha,
                                              ss, Hd.ptr + 8 * self.ld, None), "evc_fci_spin_diag")
        torch.cuda.synchronize()
        rec = solve_record()
        assert re.fullmatch(SPIN_RECORDS["evc_fci_spin_diag"], rec), rec
        got = Hd.rows()
        assert np.isnan(got[0]).all()
        return got[1].reshape(self.na, self.nb)


def host_diagonal(norb, nelec):
    """<I|S^2|I> = Sz (Sz + 1) + n_beta - popcount(occ(Ia) & occ(Ib)), from the occupation numbers."""
    from evcont_amd.fci_davidson import occupations
    sz = 0.5 * (nelec[0] - nelec[1])
    return sz * (sz + 1) + nelec[1] - occupations(norb, nelec[0]) @ occupations(norb, nelec[1]).T


@pytest.mark.parametrize("norb,nelec", SHAPES)
def test_apply_and_diag_integer_data_bit_for_bit(norb, nelec):
    p = Spin(norb, nelec)
    rng = np.random.default_rng(100 * norb + 10 * nelec[0] + nelec[1])
    c = rng.integers(-3, 4, size=(p.na, p.nb)).astype(np.float64)             # not symmetric in (Ia, Ib)
    o = rng.integers(-3, 4, size=(p.na, p.nb)).astype(np.float64)
    for alpha in (1.0, 0.5):
        for ss in (0.0, 0.75, 2.0):
            for beta in (0.0, 1.0):
                want = spin_square_through_tables(c, norb, nelec, alpha, ss, beta, o if beta else None)
                got = p.apply(c, alpha, ss, beta, o if beta else None)
                assert np.array_equal(got, want), (alpha, ss, beta, int((got != want).sum()))
    assert np.array_equal(p.apply(c), spin_square_vector(c, norb, nelec))      # and the CSR statement
    hd = rng.integers(-5, 6, size=(p.na, p.nb)).astype(np.float64)
    d = host_diagonal(norb, nelec)
    for alpha, ss in ((1.0, 0.0), (0.5, 0.75), (0.5, 2.0)):
        assert np.array_equal(p.diag(hd, alpha, ss), hd + alpha * (d - ss)), (alpha, ss)


@pytest.mark.parametrize("norb,nelec", MORE_SHAPES)
def test_apply_integer_data_runs_that_do_not_divide_na(norb, nelec):
    p = Spin(norb, nelec)
    run = workgroups(p.na, p.nb)[1]
    assert run == {12: 4, 16: 28}[norb]                  # (12,(6,2)): two tiles of beta strings, the second with two
    assert norb != 16 or p.na % run != 0                  # (16,(8,2)): runs of 28, the last of 18
    rng = np.random.default_rng(norb)
    c = rng.integers(-3, 4, size=(p.na, p.nb)).astype(np.float64)
    o = rng.integers(-3, 4, size=(p.na, p.nb)).astype(np.float64)
    for alpha, ss, beta in ((1.0, 0.0, 0.0), (0.5, 0.75, 1.0)):
        want = spin_square_through_tables(c, norb, nelec, alpha, ss, beta, o if beta else None)
        got = p.apply(c, alpha, ss, beta, o if beta else None)
        assert np.array_equal(got, want), (alpha, ss, beta, int((got != want).sum()))


def test_known_answers_and_the_diagonal_from_unit_vectors():
    # no beta electron: S^2 c = Sz (Sz + 1) c for any c
    for norb, n in ((6, 3), (5, 2)):
        p = Spin(norb, (n, 0))
        c = np.random.default_rng(n).integers(-3, 4, size=(p.na, 1)).astype(np.float64)
        assert np.array_equal(p.apply(c), 0.5 * n * (0.5 * n + 1) * c)
    # a closed-shell determinant is a singlet; the diagonal read off unit vectors is what evc_fci_spin_diag adds
    p = Spin(4, (2, 2))
    unit = np.zeros(p.dim)
    unit[0] = 1.0
    assert np.array_equal(p.apply(unit), np.zeros((p.na, p.nb)))
    diag = np.empty(p.dim)
    for k in range(p.dim):
        unit[:] = 0.0
        unit[k] = 1.0
        diag[k] = p.apply(unit).reshape(-1)[k]
    assert np.array_equal(p.diag(np.zeros(p.dim)).reshape(-1), diag)
    assert np.array_equal(diag.reshape(p.na, p.nb), host_diagonal(4, (2, 2)))


def longdouble_reference(c, norb, nelec, alpha, ss, beta, out):
    """(value, bound) per element, the sums in np.longdouble."""
    ta, tb = packed_table(norb, nelec[0]), packed_table(norb, nelec[1])
    na, nb = ta.shape[0], tb.shape[0]
    cl = c.astype(LD)
    sz = 0.5 * (nelec[0] - nelec[1])
    kms = LD(sz * (sz + 1) + nelec[1]) - LD(ss)
    t, mag, terms = kms * cl, abs(kms) * np.abs(cl), np.zeros((na, nb))
    for p in range(norb):
        for q in range(norb):
            a, b = ta[:, p * norb + q], tb[:, q * norb + p]
            ra, rb = np.flatnonzero(a), np.flatnonzero(b)
            if ra.size == 0 or rb.size == 0:
                continue
            g = cl[np.ix_(np.abs(a[ra]) - 1, np.abs(b[rb]) - 1)]
            t[np.ix_(ra, rb)] -= (np.sign(a[ra])[:, None] * np.sign(b[rb])[None, :]) * g
            mag[np.ix_(ra, rb)] += np.abs(g)
            terms[np.ix_(ra, rb)] += 1
    val = LD(alpha) * t + (LD(beta) * out.astype(LD) if beta else 0)
    bound = (terms + 3) * U * ((np.abs(beta * out) if beta else 0.0) + abs(alpha) * mag.astype(np.float64))
    return val, bound


@pytest.mark.parametrize("norb,nelec", [(8, (4, 4)), (10, (5, 5))])
def test_apply_random_data_within_the_derived_bound(norb, nelec):
    p = Spin(norb, nelec)
    rng = np.random.default_rng(norb)
    c, o = rng.standard_normal((p.na, p.nb)), rng.standard_normal((p.na, p.nb))
    for alpha, ss, beta in ((1.0, 0.0, 0.0), (0.2, 2.0, 1.0)):
        got = p.apply(c, alpha, ss, beta, o if beta else None)
        val, bound = longdouble_reference(c, norb, nelec, alpha, ss, beta, o)
        err = np.abs((got.astype(LD) - val).astype(np.float64))
        print(f"spin_apply random ({norb},{nelec}) alpha={alpha} beta={beta}: max err/bound = {(err / bound).max():.3f}")
        assert (err <= bound).all()
        assert np.array_equal(got, p.apply(c, alpha, ss, beta, o if beta else None))            # run to run
        assert np.array_equal(got, spin_square_through_tables(c, norb, nelec, alpha, ss, beta, o))  # the stated order


# ---- the solver ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_h6():
    """SmallFCI(spin_penalty=0.2) at H6, 1.8 Bohr, three roots: the reference of the three device routes."""
    h1, h2 = oao_integrals(6, 1.8)
    s = SmallFCI(spin_penalty=0.2)
    e, v = s.kernel(h1, h2, 6, (3, 3), nroots=3)
    return h1, h2, e, v, list(s.spin_squares)


def held_to_host(solver, h1, h2, norb, nelec, e_h, v_h, ss_h, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        e, v = solver.kernel(h1, h2, norb, nelec, nroots=len(e_h), **kw)
    assert np.abs(np.array(e) - e_h).max() < 1e-10
    for a, b in zip(v, v_h):
        assert min(np.abs(a - b).max(), np.abs(a + b).max()) < 1e-7
    assert np.abs(np.array(solver.spin_squares) - ss_h).max() < 1e-8
    return e, v


@pytest.mark.parametrize("route", ["dense", "eigsh", "davidson"])
def test_device_solver_with_penalty_against_host_h6(host_h6, route):
    from evcont_amd.fci_device import DeviceFCI
    h1, h2, e_h, v_h, ss_h = host_h6
    kw = dict(dense=dict(), eigsh=dict(dense_limit=100), davidson=dict(eigensolver="davidson"))[route]
    solver = DeviceFCI(spin_penalty=0.2, **kw)
    e, v = held_to_host(solver, h1, h2, 6, (3, 3), e_h, v_h, ss_h)
    assert np.abs(np.array(ss_h)).max() < 1e-8
    assert np.abs(np.array(e) - [-8.077851, -7.648414, -7.623083]).max() < 6e-7
    # contract is the shifted operator, as SmallFCI's
    c = np.random.default_rng(3).standard_normal((20, 20))
    want = SmallFCI(spin_penalty=0.2).contract(h1, h2, c, 6, (3, 3))
    assert np.abs(solver.contract(h1, h2, c, 6, (3, 3)) - want).max() < 1e-12
    for x in v:
        ss, mult = solver.spin_square(x, 6, (3, 3))
        assert abs(ss) < 1e-8 and abs(mult - 1.0) < 1e-7
        assert abs(solver.spin_square(torch.from_numpy(x).to("cuda:0"), 6, (3, 3))[0] - ss) < 1e-12


def test_plain_device_solver_keeps_its_mix_and_launches_none_of_the_new_kernels():
    from evcont_amd.fci_device import DeviceFCI
    h1, h2 = oao_integrals(6, 1.8)
    Spin(2, (1, 1)).diag(np.zeros(4))                      # the stage holds a new name before the plain runs
    assert solve_record() == "fci_spin_diag_kernel"
    for kw in (dict(), dict(eigensolver="davidson"), dict(spin_penalty=0.0, spin_target=None, eigensolver="davidson")):
        solver = DeviceFCI(**kw)
        e, v = solver.kernel(h1, h2, 6, (3, 3), nroots=3)
        rec = solve_record()
        if "eigensolver" in kw:
            assert rec and not any(k in rec for k in NEW_KERNELS), rec
        else:
            assert rec == "fci_spin_diag_kernel"           # the host routes launch nothing on this stage
        assert solver.spin_squares is None
        assert np.abs(np.array(e) - [-8.077851, -7.885217, -7.690716]).max() < 6e-7
    assert np.abs(np.array([solver.spin_square(x, 6, (3, 3))[0] for x in v]) - [0, 2, 2]).max() < 1e-8
    assert "fci_dots_kernel" in solve_record()            # spin_square: one apply, then one dot
    with pytest.raises(ValueError, match="spin_target"):
        DeviceFCI(spin_penalty=0.2, spin_target=1.0).kernel(h1, h2, 6, (3, 3))


def test_davidson_with_penalty_h8_and_warm_start():
    from evcont_amd.fci_device import DeviceFCI
    h1, h2 = oao_integrals(8, 1.8)
    host = SmallFCI(spin_penalty=0.2)
    e_h, v_h = host.kernel(h1, h2, 8, (4, 4), nroots=3)
    assert np.abs(np.array(e_h) - [-11.950523, -11.606001, -11.562580]).max() < 6e-7
    solver = DeviceFCI(spin_penalty=0.2, eigensolver="davidson")
    _, v = held_to_host(solver, h1, h2, 8, (4, 4), e_h, v_h, host.spin_squares)
    assert solver.converged and "fci_dots_kernel" in solve_record()
    cold = solver.davidson_info["nsigma"]
    # warm start from the neighbouring spacing
    h1n, h2n = oao_integrals(8, 1.85)
    e_n, v_n = host.kernel(h1n, h2n, 8, (4, 4), nroots=3)
    held_to_host(solver, h1n, h2n, 8, (4, 4), e_n, v_n, host.spin_squares, ci0=v)
    print(f"H8 three singlets: {cold} sigma vectors cold, {solver.davidson_info['nsigma']} warm")
    assert solver.davidson_info["nsigma"] < cold


def test_h4_fourth_root_warning_on_the_device():
    from evcont_amd.fci_device import DeviceFCI
    h1, h2 = oao_integrals(4, 1.8)
    for kw in (dict(), dict(eigensolver="davidson")):
        solver = DeviceFCI(spin_penalty=0.2, **kw)
        with pytest.warns(RuntimeWarning, match="root 3"):
            e, v = solver.kernel(h1, h2, 4, (2, 2), nroots=4)
        assert abs(e[3] - (-4.325077)) < 6e-7 and abs(solver.spin_squares[3] - 2.0) < 1e-8


def test_spin_square_survives_transform_ci():
    """A singlet solved in the Hartree-Fock basis and rotated into the Loewdin basis is still a singlet."""
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    from evcont_amd.fci_device import DeviceFCI
    solver = DeviceFCI(spin_penalty=0.2, eigensolver="davidson")
    c = FCI_EVCont_obj(cisolver=solver, cibasis="canonical", nroots=2)
    c.append_to_rdms(hydrogen_chain(6, 1.8, need_grad=False))
    for x in c.fcivecs:
        assert abs(solver.spin_square(x, 6, (3, 3))[0]) < 1e-10


# ---- containers ------------------------------------------------------------------------------------------------------
TRAIN = (1.4, 1.8, 2.4)


@pytest.fixture(scope="module")
def host_container():
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    c = FCI_EVCont_obj(cisolver=SmallFCI(spin_penalty=0.2), cibasis="OAO", nroots=2)
    for d in TRAIN:
        c.append_to_rdms(hydrogen_chain(6, d, need_grad=False))
    return c


def test_container_grown_with_the_penalty_on_the_device(host_container):
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    from evcont_amd.ab_initio_gradients_loewdin import get_multistate_energy_with_grad
    from evcont_amd.fci_device import DeviceFCI
    from test_hchain_physics import bent_chain
    from evcont_amd.hchain import s_gaussian_mol
    solver = DeviceFCI(spin_penalty=0.2, eigensolver="davidson")
    cd, ch = FCI_EVCont_obj(cisolver=solver, cibasis="OAO", nroots=2), host_container
    for d in TRAIN:
        cd.append_to_rdms(hydrogen_chain(6, d, need_grad=False))
    assert cd.mol_index == [0, 0, 1, 1, 2, 2]
    for x in cd.fcivecs:
        assert abs(solver.spin_square(x, 6, (3, 3))[0]) < 1e-8
    # at a training geometry the continuation is exact: the two lowest singlets of the dense host solve
    mt = hydrogen_chain(6, 1.8)
    h1, h2 = oao_integrals(6, 1.8)
    plain = SmallFCI()
    w, u = plain.kernel(h1, h2, 6, (3, 3), nroots=6)
    singlets = [e for e, x in zip(w, u) if abs(plain.spin_square(x, 6, (3, 3))[0]) < 1e-8][:2]
    E, _ = get_multistate_energy_with_grad(mt, cd.one_rdm, cd.two_rdm, cd.overlap, 2)
    assert np.abs(E - (np.array(singlets) + mt.energy_nuc())).max() < 1e-9
    # and between them it agrees with the container grown on the host
    m = s_gaussian_mol(bent_chain(6, d=1.9, seed=11, amp=0.15))
    Ed, gd = get_multistate_energy_with_grad(m, cd.one_rdm, cd.two_rdm, cd.overlap, 2)
    Eh, gh = get_multistate_energy_with_grad(m, ch.one_rdm, ch.two_rdm, ch.overlap, 2)
    print(f"H6 singlet container: |dE|={np.abs(Ed - Eh).max():.2e} |dg|={np.abs(gd - gh).max():.2e}")
    assert np.abs(Ed - Eh).max() < 1e-10 and np.abs(gd - gh).max() < 1e-9


def test_resident_container_grown_with_the_penalty(host_container):
    from evcont_amd.ab_initio_gradients_loewdin import get_multistate_energy_with_grad
    from evcont_amd.evaluator import ContinuationEvaluator, DeviceAO
    from evcont_amd.fci_device import DeviceFCI
    from evcont_amd.integrals import ao_arrays
    from evcont_amd.resident import ResidentFCI_EVCont_obj
    solver = DeviceFCI(spin_penalty=0.2, eigensolver="davidson")
    cr = ResidentFCI_EVCont_obj(cisolver=solver, cibasis="OAO", nroots=2, layout="sym8")
    for d in TRAIN:
        cr.append_to_rdms(hydrogen_chain(6, d, need_grad=False))
    for x in cr.fcivecs:
        assert abs(solver.spin_square(x, 6, (3, 3))[0]) < 1e-8
    ch = host_container
    t = cr.device_trdms()
    for mol in (hydrogen_chain(6, 1.8), hydrogen_chain(6, 2.1)):
        ao = ao_arrays(mol, need_grad=True)
        res = ContinuationEvaluator(t, 6).energies_with_grads(DeviceAO.from_arrays(ao, t.device), 2)
        Eh, gh = get_multistate_energy_with_grad(mol, ch.one_rdm, ch.two_rdm, ch.overlap, 2)
        assert np.abs(res[0] - Eh).max() < 1e-10 and np.abs(res[2][:2] - gh).max() < 1e-9
    assert np.abs(np.array(cr.ens) - np.array(ch.ens)).max() < 1e-10


def test_example_trains_on_singlets(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "h6_excited_pes.py"), "--solver", "device-davidson",
                        "--points", "3"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    values = [float(x) for x in re.findall(r"<S\^2> = (-?\d+\.\d+)", r.stdout)]
    assert len(values) == 12 and max(abs(v) for v in values) < 5e-7, r.stdout      # 3 protocols x (1 + 1 + 2) states
