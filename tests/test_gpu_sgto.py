"""GPU tests of the device AO integrals of s-Gaussian molecules (include/evcont_hip.h evc_sgto_integrals_batch,
csrc/sgto.hip), through ctypes on NaN-poisoned, fenced output buffers and workspace, against ``hchain.s_gaussian_mol``
within the derived bound of tests/sgto_reference.py: per element 2^-53 (n_terms + 432) sum|terms|.

Largest |device - s_gaussian_mol| in units of 2^-53 sum|terms|, per shape: DESIGN.md section 8.2."""
import numpy as np
import pytest

import sgto_reference as ref
from evcont_amd import _lib
from evcont_amd.hchain import (STO3G_H_COEFFICIENTS, STO3G_H_EXPONENTS, STO6G_H_COEFFICIENTS, STO6G_H_EXPONENTS,
                               s_gaussian_mol)
from sgto_harness import GRAD_FIELDS, MODES, run, unpack

pytestmark = pytest.mark.gpu

STO3G = (STO3G_H_EXPONENTS, STO3G_H_COEFFICIENTS)
STO6G = (STO6G_H_EXPONENTS, STO6G_H_COEFFICIENTS)
ONE = ((0.4,), (1.0,))


def _cluster(A, G, seed):
    """G perturbed chains of A centres: neighbours 1.7 Bohr apart along x, every coordinate moved by up to 0.3."""
    rng = np.random.default_rng(seed)
    R = np.zeros((G, A, 3))
    R[:, :, 0] = 1.7 * np.arange(A)
    return R + 0.3 * rng.uniform(-1.0, 1.0, (G, A, 3))


def _chain(A, d):
    R = np.zeros((1, A, 3))
    R[0, :, 0] = d * np.arange(A)
    return R


# id -> (coordinates (G,A,3), charges, (exponents, coefficients))
SHAPES = {
    "A1_K3_G1": (np.array([[[0.3, -0.2, 0.5]]]), [1.0], STO3G),
    "A2_K1_G1": (np.array([[[0.0, 0.1, -0.2], [1.3, -0.4, 0.6]]]), [1.0, 1.0], ONE),
    "A2_K6_G2": (_cluster(2, 2, 1), [1.0, 1.0], STO6G),
    "A3_K3_G3_charges": (1.5 * np.random.default_rng(2).standard_normal((3, 3, 3)), [1.0, 2.0, 0.5], STO3G),
    "A3_K3_G1_close_pair": (np.array([[[0.0, 0.0, 0.0], [0.02, -0.02, 0.01], [6.0, 0.3, -0.2]]]), [1.0, 1.0, 1.0], STO3G),
    "A5_K3_G2": (_cluster(5, 2, 3), [1.0] * 5, STO3G),
    "A7_K1_G1": (_cluster(7, 1, 4), [1.0] * 7, ONE),
    "A17_K1_G2": (_cluster(17, 2, 5), [1.0] * 17, ONE),
    "H10_K3_G1": (_chain(10, 1.8), [1.0] * 10, STO3G),
}


@pytest.fixture(scope="module", params=sorted(SHAPES))
def shape(request):
    R, Z, basis = SHAPES[request.param]
    res = {m: run(R, Z, basis, m) for m in MODES}
    host = [s_gaussian_mol(r, Z, *basis) for r in R]
    sums = [ref.abs_sums(r, Z, *basis) for r in R]
    return request.param, R, Z, basis, res, host, sums


def test_calls_succeed_with_fences_intact(shape):
    _, R, _, _, res, _, _ = shape
    for mode, (rc, arrays, intact, _) in res.items():
        assert rc == 0, (mode, _lib.load().evc_last_error())
        assert intact, mode
        written = GRAD_FIELDS if mode != "energy" else ()
        for k, v in arrays.items():
            if k in written or k not in GRAD_FIELDS:
                assert np.all(np.isfinite(v)), (mode, k)


def test_against_s_gaussian_mol_within_the_bound(shape):
    name, R, Z, basis, res, host, sums = shape
    A, K = R.shape[1], len(basis[0])
    full = res["full"][1]
    for field in ref.NAMES:
        worst = max(ref.worst_ratio(field, A, K, full[field][g], getattr(host[g], field), sums[g][field])
                    for g in range(R.shape[0]))
        print(f"{name} {field}: worst |device - s_gaussian_mol| = {worst:.1f} x 2^-53 sum|terms| "
              f"(bound {ref.n_terms(field, A, K) + ref.ROUNDINGS})")
        for g in range(R.shape[0]):
            err = np.abs(full[field][g] - np.asarray(getattr(host[g], field)))
            assert np.all(err <= ref.allowed(field, A, K, sums[g][field])), (field, g, float(err.max()))
    for field in ("enuc", "S", "hcore", "eri"):                    # the energy-only call against the host as well
        for g in range(R.shape[0]):
            err = np.abs(res["energy"][1][field][g] - np.asarray(getattr(host[g], field)))
            assert np.all(err <= ref.allowed(field, A, K, sums[g][field])), ("energy-only", field, g)


def test_full_is_the_unpacked_packed_form(shape):
    _, R, _, _, res, _, _ = shape
    packed, full = res["packed"][1], res["full"][1]
    eri, ip1 = unpack(packed, R.shape[1])
    assert np.array_equal(full["eri"], eri)
    assert np.array_equal(full["eri_ip1"], ip1)
    for k in ("enuc", "S", "hcore", "ipovlp", "dhcore", "gnuc"):
        assert np.array_equal(full[k], packed[k]), k


def test_energy_only_has_the_bits_of_the_full_call_and_leaves_the_derivatives_alone(shape):
    _, R, Z, basis, res, _, _ = shape
    energy, full = res["energy"][1], res["full"][1]
    for k in ("enuc", "S", "hcore", "eri"):
        assert np.array_equal(energy[k], full[k]), k
    for k in GRAD_FIELDS:
        assert np.all(np.isnan(energy[k])), k
    rc, arrays, intact, _ = run(R, Z, basis, "energy", null_grad=True)     # NULL derivative pointers are accepted
    assert rc == 0 and intact
    assert np.array_equal(arrays["eri"], full["eri"]) and np.array_equal(arrays["hcore"], full["hcore"])
    rc, arrays, intact, _ = run(R, Z, basis, "energy", flags=_lib.FLAG_ENERGY_ONLY | _lib.FLAG_ERI_S4)
    assert rc == 0 and intact
    assert np.array_equal(arrays["eri"].reshape(-1)[:res["packed"][1]["eri"].size], res["packed"][1]["eri"].reshape(-1))


def test_batch_is_its_geometries_and_runs_repeat(shape):
    _, R, Z, basis, res, _, _ = shape
    for mode in ("packed", "full"):
        again = run(R, Z, basis, mode)[1]
        for k, v in res[mode][1].items():
            assert np.array_equal(v, again[k]), (mode, k)
    if R.shape[0] > 1:
        for g in range(R.shape[0]):
            single = run(R[g:g + 1], Z, basis, "packed")[1]
            for k, v in res["packed"][1].items():
                assert np.array_equal(v[g], single[k][0]), (g, k)


def test_exact_symmetries(shape):
    _, _, _, _, res, _, _ = shape
    full = res["full"][1]
    for k in ("S", "hcore"):
        assert np.array_equal(full[k], np.swapaxes(full[k], 1, 2)), k
    assert np.array_equal(full["eri"], np.swapaxes(full["eri"], 1, 2))
    assert np.array_equal(full["eri"], np.swapaxes(full["eri"], 3, 4))


def test_refusals_leave_the_outputs_alone():
    """Every refused argument: rc < 0, a message, and neither the poisoned outputs nor the workspace touched."""
    lib = _lib.load()
    R, Z, basis = SHAPES["A3_K3_G3_charges"]
    need = lib.evc_sgto_workspace_bytes(3, 3, 3)
    bad_ex = np.array([3.4, -1.0, 0.1])
    cases = [(dict(natm=0), b"natm"), (dict(natm=97), b"natm"), (dict(nprim=0), b"nprim"), (dict(nprim=9), b"nprim"),
             (dict(count=0), b"count"), (dict(coords=None), b"null"), (dict(charges=None), b"null"),
             (dict(ex=None), b"null"), (dict(co=None), b"null"), (dict(out=None), b"null"), (dict(ws=None), b"null"),
             (dict(flags=_lib.FLAG_PARTIAL_RANK), b"flags"), (dict(flags=_lib.FLAG_WARM_START), b"flags"),
             (dict(flags=64), b"flags"), (dict(ex=bad_ex.ctypes.data), b"exponent"), (dict(ws_bytes=need - 8), b"workspace"),
             (dict(natm=65, flags=_lib.FLAG_IP1_S2KL), b"natm <= 64")]
    for override, word in cases:
        rc, arrays, intact, bufs = run(R, Z, basis, "full", **override)
        assert rc < 0, override
        assert word in lib.evc_last_error(), (override, lib.evc_last_error())
        assert intact, override
        for k, v in arrays.items():
            assert np.all(np.isnan(v)), (override, k)
    rc, arrays, intact, _ = run(R, Z, basis, "full", null_grad=True)       # NULL derivative pointers without the flag
    assert rc < 0 and b"null" in lib.evc_last_error() and intact
    assert all(np.all(np.isnan(v)) for v in arrays.values())
