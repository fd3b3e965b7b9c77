"""CPU tests of the block Davidson driver (evcont_amd/fci_davidson.py) on its numpy back-end, which runs the same
iteration as ``DeviceFCI(eigensolver="davidson")`` with ``SmallFCI.contract`` as the sigma vector: the diagonal of H, the
convergence, restart and basis-complete logic, the warm start and the iteration cap.

Bounds: energies to 1e-10 Ha and eigenvectors to 1e-7 up to the sign against ``SmallFCI.kernel`` -- the tolerances of
tests/test_gpu_fci_device.py::test_kernel_against_host.  With a residual norm of at most conv_tol = 1e-10 the energy
error is of second order and the vector error at most conv_tol over the gap to the next state (about 1e-10 / 0.1 Ha
here), both far inside them."""
import warnings

import numpy as np
import pytest

from evcont_amd.fci_davidson import NumpyOps, davidson, hdiag_numpy
from evcont_amd.fci_small import SmallFCI
from evcont_amd.hchain import hydrogen_chain
from oracle import evcont_oracle as orc
from test_hchain_physics import bundle

_HOST = SmallFCI()
RESTART_CASE = (6, (3, 3), 1, 6)     # (norb, nelec, nroots, max_space): a restart every few iterations; also run on the GPU


def oao_integrals(norb, d=1.8):
    m = hydrogen_chain(norb, d, need_grad=False)
    return orc.integrals_oao(bundle(m), orc.loewdin_trafo(m.S))


def integer_integrals(norb, seed):
    """Integer h1, even-integer h2, no permutation symmetry: every intermediate of the diagonal is an integer."""
    rng = np.random.default_rng(seed)
    h1 = rng.integers(-6, 7, size=(norb, norb)).astype(np.float64)
    h2 = 2.0 * rng.integers(-4, 5, size=(norb,) * 4).astype(np.float64)
    return h1, h2


@pytest.mark.parametrize("norb,nelec", [(3, (2, 1)), (4, (2, 2)), (5, (3, 2))])
def test_hdiag_is_the_diagonal_of_the_dense_matrix_exactly(norb, nelec):
    h1, h2 = integer_integrals(norb, seed=norb)
    _, _, na, nb = _HOST._ops(norb, nelec)
    dim = na * nb
    eye = np.eye(dim)
    diag = np.array([_HOST.contract(h1, h2, eye[k].reshape(na, nb), norb, nelec).reshape(-1)[k] for k in range(dim)])
    got = hdiag_numpy(h1, h2, norb, nelec)
    assert got.shape == (na, nb)
    assert np.array_equal(got.reshape(-1), diag)
    assert np.abs(diag).max() > 0 and len(set(diag.tolist())) > 1


def solve(norb, nelec, nroots, **kw):
    h1, h2 = oao_integrals(norb)
    ops = NumpyOps(h1, h2, norb, nelec, _HOST)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        e, v, conv, info = davidson(ops, nroots=nroots, **kw)
    return h1, h2, e, v, conv, info


@pytest.mark.parametrize("norb,nelec,nroots,max_space",
                         [(2, (1, 1), 3, None), (4, (2, 2), 3, None), (6, (3, 2), 3, None), (6, (3, 3), 1, None),
                          RESTART_CASE])
def test_driver_against_host_kernel(norb, nelec, nroots, max_space):
    h1, h2, e, v, conv, info = solve(norb, nelec, nroots, max_space=max_space)
    e_h, v_h = _HOST.kernel(h1, h2, norb, nelec, nroots=nroots)
    if nroots == 1:
        e_h, v_h = [e_h], [v_h]
    de = max(abs(a - b) for a, b in zip(e, e_h))
    dv = max(min(np.abs(a - b.reshape(-1)).max(), np.abs(a + b.reshape(-1)).max()) for a, b in zip(v, v_h))
    print(f"davidson norb={norb} nelec={nelec} nroots={nroots} max_space={max_space}: {info['iterations']} iterations, "
          f"{info['nsigma']} sigma vectors, {info['restarts']} restarts, |dE|={de:.2e} |dv|={dv:.2e}")
    assert conv and de < 1e-10 and dv < 1e-7
    assert (info["residuals"] <= 1e-10).all()
    assert np.abs(v @ v.T - np.eye(nroots)).max() < 1e-9
    dim = v.shape[1]
    if max_space is not None and max_space < dim:
        assert info["restarts"] >= 3                 # the case is there for the restarts
    if norb == 2:
        assert info["nsigma"] == dim == 4           # three start vectors and one correction complete the basis


@pytest.mark.parametrize("norb,nelec,nroots", [(6, (3, 3), 1), (6, (3, 2), 3)])
def test_converged_start_vectors_cost_one_sigma_vector_each(norb, nelec, nroots):
    h1, h2 = oao_integrals(norb)
    e_h, v_h = _HOST.kernel(h1, h2, norb, nelec, nroots=nroots)
    ci0 = v_h if nroots == 1 else list(v_h)
    e, v, conv, info = davidson(NumpyOps(h1, h2, norb, nelec, _HOST), nroots=nroots, ci0=ci0)
    assert conv and info["nsigma"] == nroots and info["iterations"] == 1
    assert np.abs(np.atleast_1d(e_h) - e).max() < 1e-10


def test_iteration_cap_reports_not_converged():
    h1, h2 = oao_integrals(6)
    with pytest.warns(RuntimeWarning, match="not converged"):
        e, v, conv, info = davidson(NumpyOps(h1, h2, 6, (3, 3), _HOST), nroots=1, max_cycle=2)
    assert conv is False and info["iterations"] == 2 and v.shape == (1, 400)
    assert abs(np.linalg.norm(v[0]) - 1.0) < 1e-12   # the best vector so far is returned


def test_unknown_eigensolver_raises():
    from evcont_amd.fci_device import DeviceFCI
    with pytest.raises(ValueError, match="nonsense"):
        DeviceFCI(eigensolver="nonsense")
    assert DeviceFCI().eigensolver == "host"


def test_davidson_without_a_device_raises():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from evcont_amd._lib import EvcontHipError
    from evcont_amd.fci_device import DeviceFCI
    h1, h2 = oao_integrals(4)
    with pytest.raises(EvcontHipError):
        DeviceFCI(eigensolver="davidson").kernel(h1, h2, 4, (2, 2))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Host-side validation of the vector entry points (no device needed: nothing is enqueued)."""
    from evcont_amd import _lib, build
    build.build()
    lib = _lib.load()
    a = 1 << 20                                         # pointers are only compared, never followed
    assert lib.evc_fci_combine(100, a, 100, 3, a, 2, 2, 0.0, a + 8 * 250, 100, None) < 0      # Out inside V
    assert b"alias" in lib.evc_last_error()
    assert lib.evc_fci_combine(100, a + 800, 100, 3, a, 2, 2, 0.0, a, 100, None) < 0          # Out's second row inside V
    assert b"alias" in lib.evc_last_error()
    assert lib.evc_fci_combine(100, a, 99, 3, a, 2, 2, 0.0, a + (1 << 16), 100, None) < 0
    assert b"ldv=99" in lib.evc_last_error()
    assert lib.evc_fci_dots(100, a, 100, 0, a, 100, 1, a, a, 1 << 16, None) < 0
    assert b"nx=0" in lib.evc_last_error()
    assert lib.evc_fci_dots(100, a, 100, 2, a, 100, 2, a, a, 8, None) < 0
    assert b"workspace" in lib.evc_last_error()
    assert lib.evc_fci_davidson_correction(100, a, 100, a, 100, 2, a, 1, a, 1, a + (1 << 18), a + 8 * 50, 100, a, a, 1 << 16,
                                           None) < 0
    assert b"alias" in lib.evc_last_error()
    assert lib.evc_fci_hdiag(17, 1, 1, a, a, a, a, a, a, 1 << 20, None) < 0
    assert b"norb=17" in lib.evc_last_error()
    assert lib.evc_fci_solve_workspace_bytes(10, 252, 252, 300) == 0
    rows = 256                                          # 63 504 determinants: 249 blocks of 256
    assert lib.evc_fci_solve_workspace_bytes(10, 252, 252, 20) >= -(-63504 // rows) * 20 * 20 * 8
