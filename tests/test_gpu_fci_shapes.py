"""GPU tests of the device full-CI solver on every orbital count 1 ... 16 and every tiling its dispatch can reach
(tests/fci_dispatch_table.py), against the host solver fci_small.SmallFCI.

Two kinds of input per case:

* Integers: CI vectors with entries in -3 ... 3, a symmetric integer h1 and an h2 of even integers without any
  permutation symmetry.  Every intermediate -- D, the product tiles, the split-K partials, g1, G, G/2 + h'c, sigma -- is
  then an integer far below 2^53 and exact in FP64 in any summation order, so the device must give the bits of the host
  (np.array_equal) and the overlap the exact integer dot product.  The host result is asserted integral first.
* Random normalised vectors with hydrogen-chain integrals in the OAO basis, held to the bounds derived in
  tests/test_gpu_fci_device.py (imported from there).

The kernels each call launched (evc_profile_kernel) must be those of the table.
"""
import time

import numpy as np
import pytest
import torch

from evcont_amd.fci_small import SmallFCI
from fci_dispatch_table import SHAPE_CASES, sigma_record, trdm_record
from test_gpu_fci_device import check_identities, oao_integrals, random_vectors, sigma_bound, solver, trdm_bound

pytestmark = pytest.mark.gpu

_HOST = SmallFCI()
IDS = [f"{n}-{e}".replace(" ", "") for n, e in SHAPE_CASES]


def nelec2(nelec):
    if isinstance(nelec, int):
        return (nelec + 1) // 2, nelec // 2
    return tuple(nelec)


def strings(norb, nelec):
    _, _, na, nb = _HOST._ops(norb, nelec2(nelec))
    return na, nb


def integer_vectors(norb, nelec, count, seed):
    na, nb = strings(norb, nelec)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        v = rng.integers(-3, 4, size=(na, nb)).astype(np.float64)
        if not v.any():
            v.flat[0] = 2.0
        out.append(v)
    return out


def integer_integrals(norb, seed):
    """h1 symmetric integers, h2 even integers with no permutation symmetry."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-2, 3, size=(norb, norb))
    h1 = (np.triu(a) + np.triu(a, 1).T).astype(np.float64)
    h2 = (2 * rng.integers(-2, 3, size=(norb,) * 4)).astype(np.float64)
    return h1, h2


def integral(x):
    x = np.asarray(x)
    return bool(np.array_equal(x, np.rint(x)) and np.abs(x).max(initial=0.0) < 2.0 ** 40)


def records():
    from evcont_amd import _lib
    lib = _lib.load()
    return {k: lib.evc_profile_kernel(s).decode() for k, s in _lib.FCI_PROF_STAGES.items()}


def expect_trdm_record(norb, dim):
    """A resident call: the bra side whole, every ket in one launch."""
    head = trdm_record(norb, dim)
    blocks = int(head.split("blocks=")[1])
    rec = records()
    assert rec["fci_trdm"] == f"{head}bra_resident=1 ket_blocks={blocks}", rec
    assert rec["fci_excite"] == "fci_excite_det_kernel<0>", rec


def expect_sigma_record(norb, dim):
    rec = records()
    ldg = (dim + 63) // 64 * 64
    assert rec["fci_sigma"] == f"{sigma_record(norb)}{ldg} + fci_sigma_gather_kernel", rec
    assert rec["fci_excite"] == "fci_excite_orb_kernel", rec


@pytest.mark.parametrize("norb,nelec", SHAPE_CASES, ids=IDS)
def test_integer_inputs_give_the_bits_of_the_host(norb, nelec):
    """A row call of three kets and the bra, its single-pair calls and the sigma vector, bit for bit."""
    dev = solver()
    ne = nelec2(nelec)
    na, nb = strings(norb, nelec)
    K = 3
    vecs = integer_vectors(norb, nelec, K + 1, seed=1000 + 17 * norb + ne[0] + 3 * ne[1])
    bra, kets = vecs[0], vecs[1:] + [vecs[0]]
    ov, one, two = dev.trans_rdm12_rows(bra, kets, norb, nelec)
    expect_trdm_record(norb, na * nb)
    assert ov.shape == (K + 1,) and one.shape == (K + 1, norb, norb) and two.shape == (K + 1,) + (norb,) * 4
    big = 0.0
    for i, ket in enumerate(kets):
        r1, r2 = _HOST.trans_rdm12(bra, ket, norb, ne)
        assert integral(r1) and integral(r2)
        big = max(big, np.abs(r2).max())
        assert ov[i] == float(np.dot(bra.ravel().astype(np.int64), ket.ravel().astype(np.int64))), (i, ov[i])
        assert np.array_equal(one[i], r1), (i, np.abs(one[i] - r1).max())
        assert np.array_equal(two[i], r2), (i, np.abs(two[i] - r2).max())
        s1, s2 = dev.trans_rdm12(bra, ket, norb, nelec)
        assert np.array_equal(s1, r1) and np.array_equal(s2, r2), i
    expect_trdm_record(norb, na * nb)
    h1, h2 = integer_integrals(norb, seed=2000 + norb)
    assert not np.array_equal(h2, h2.transpose(1, 0, 2, 3)) or norb == 1
    want = _HOST.contract(h1, h2, bra, norb, ne)
    assert integral(want)
    got = dev.contract(h1, h2, bra, norb, nelec)
    expect_sigma_record(norb, na * nb)
    assert got.shape == want.shape == (na, nb)
    assert np.array_equal(got, want), np.abs(got - want).max()
    print(f"integers norb={norb} nelec={nelec}: dim={na * nb} max|dm2|={big:.0f} max|sigma|={np.abs(want).max():.0f}")


@pytest.mark.parametrize("norb,nelec", SHAPE_CASES, ids=IDS)
def test_random_inputs_within_the_derived_bounds(norb, nelec):
    """Random normalised vectors, OAO hydrogen-chain integrals: the bounds of tests/test_gpu_fci_device.py; up to
    dense_limit determinants also the eigenpairs (1e-10 Ha, 1e-7), for one root and for three where there are three."""
    dev = solver()
    ne = nelec2(nelec)
    na, nb = strings(norb, nelec)
    dim = na * nb
    K = 3
    vecs = random_vectors(norb, ne, K + 1, seed=norb * 10 + ne[1])
    bra, kets = vecs[0], vecs[1:] + [vecs[0]]
    ov, one, two = dev.trans_rdm12_rows(bra, kets, norb, nelec)
    expect_trdm_record(norb, dim)
    worst = 0.0
    for i, ket in enumerate(kets):
        r1, r2 = _HOST.trans_rdm12(bra, ket, norb, ne)
        tol = 2.0 * trdm_bound(bra, ket, norb, ne)
        e1, e2 = np.abs(one[i] - r1).max(), np.abs(two[i] - r2).max()
        eo = abs(ov[i] - np.dot(bra.ravel(), ket.ravel()))
        worst = max(worst, e1 / tol, e2 / tol, eo / tol)
        print(f"trdm norb={norb} nelec={nelec} ket {i}: dim={dim} bound={tol:.3e} |d dm1|={e1:.3e} |d dm2|={e2:.3e} "
              f"|d ovlp|={eo:.3e}")
        assert e1 <= tol and e2 <= tol and eo <= tol
        check_identities(ov[i], one[i], two[i], ne, tol)
        s1, s2 = dev.trans_rdm12(bra, ket, norb, nelec)
        assert np.array_equal(s1, one[i]) and np.array_equal(s2, two[i])
    h1, h2 = oao_integrals(norb)
    got = dev.contract(h1, h2, bra, norb, nelec)
    expect_sigma_record(norb, dim)
    want = _HOST.contract(h1, h2, bra, norb, ne)
    stol = 2.0 * sigma_bound(h1, h2, bra, norb, ne)
    err = np.abs(got - want)
    assert got.shape == want.shape and (err <= stol).all()
    ratio = float((err[stol > 0] / stol[stol > 0]).max()) if (stol > 0).any() else 0.0
    print(f"random norb={norb} nelec={nelec}: dim={dim} worst error / allowed: trdm {worst:.3e} sigma {ratio:.3e}")
    if dim > dev.dense_limit:
        return
    top = min(3, dim)
    e_h, v_h = _HOST.kernel(h1, h2, norb, ne, nroots=top)       # dense on both sides: one root = the first of three
    if top == 1:
        e_h, v_h = [e_h], [v_h]
    for nroots in sorted({1, top}):
        e_d, v_d = dev.kernel(h1, h2, norb, nelec, nroots=nroots)
        if nroots == 1:
            assert isinstance(e_d, float) and v_d.shape == (na, nb)
            e_d, v_d = [e_d], [v_d]
        assert len(e_d) == len(v_d) == nroots
        de = max(abs(a - b) for a, b in zip(e_d, e_h))
        dv = max(min(np.abs(a - b).max(), np.abs(a + b).max()) for a, b in zip(v_d, v_h))
        for v in v_d:
            assert v.flat[np.argmax(np.abs(v))] > 0.0
        print(f"kernel norb={norb} nelec={nelec} nroots={nroots}: |dE|={de:.2e} |dv|={dv:.2e}")
        assert de < 1e-10 and dv < 1e-7


def test_large_case_on_the_quadrant_path():
    """(13, (4, 3)): 204 490 determinants in 246 blocks of 832 rows, more than 256 rows a block on the quadrant tiling.
    One pair and one sigma vector, as integers (bitwise) and random (bounds)."""
    norb, nelec = 13, (4, 3)
    dev = solver()
    na, nb = strings(norb, nelec)
    dim = na * nb
    assert dim == 204490 and trdm_record(norb, dim) == "fci_trdm_kernel<3,2> quadrants=4 blocks=246 "
    bra, ket = integer_vectors(norb, nelec, 2, seed=1343)
    t0 = time.time()
    d1, d2 = dev.trans_rdm12(bra, ket, norb, nelec)
    t1 = time.time()
    r1, r2 = _HOST.trans_rdm12(bra, ket, norb, nelec)
    t2 = time.time()
    expect_trdm_record(norb, dim)
    assert integral(r1) and integral(r2)
    assert np.array_equal(d1, r1) and np.array_equal(d2, r2)
    ov = dev.trans_rdm12_rows(bra, [ket], norb, nelec)[0][0]
    assert ov == float(np.dot(bra.ravel().astype(np.int64), ket.ravel().astype(np.int64)))
    h1, h2 = integer_integrals(norb, seed=1344)
    t3 = time.time()
    got = dev.contract(h1, h2, bra, norb, nelec)
    t4 = time.time()
    want = _HOST.contract(h1, h2, bra, norb, nelec)
    t5 = time.time()
    expect_sigma_record(norb, dim)
    assert integral(want) and np.array_equal(got, want)
    print(f"(13,(4,3)) integers: dim={dim} t-RDM pair device call {t1 - t0:.2f} s host {t2 - t1:.2f} s; sigma device call "
          f"{t4 - t3:.2f} s host {t5 - t4:.2f} s; max|dm2|={np.abs(r2).max():.0f} max|sigma|={np.abs(want).max():.0f}")
    bra, ket = random_vectors(norb, nelec, 2, seed=1345)
    d1, d2 = dev.trans_rdm12(bra, ket, norb, nelec)
    r1, r2 = _HOST.trans_rdm12(bra, ket, norb, nelec)
    tol = 2.0 * trdm_bound(bra, ket, norb, nelec)
    e1, e2 = np.abs(d1 - r1).max(), np.abs(d2 - r2).max()
    ov = dev.trans_rdm12_rows(bra, [ket], norb, nelec)[0][0]
    eo = abs(ov - np.dot(bra.ravel(), ket.ravel()))
    print(f"(13,(4,3)) random: bound={tol:.3e} |d dm1|={e1:.3e} |d dm2|={e2:.3e} |d ovlp|={eo:.3e} "
          f"worst error / allowed = {max(e1, e2, eo) / tol:.3e}")
    assert e1 <= tol and e2 <= tol and eo <= tol
    check_identities(ov, d1, d2, nelec, tol)
    h1, h2 = oao_integrals(norb)
    got = dev.contract(h1, h2, bra, norb, nelec)
    want = _HOST.contract(h1, h2, bra, norb, nelec)
    stol = 2.0 * sigma_bound(h1, h2, bra, norb, nelec)
    err = np.abs(got - want)
    print(f"(13,(4,3)) random sigma: max|d|={err.max():.3e} max(err/bound)={(err / stol).max():.3e}")
    assert (err <= stol).all()


# ---- input forms and the upload cache ---------------------------------------------------------------------------
def _all_results(dev, bra, ket, h1, h2, norb, nelec):
    ov, one, two = dev.trans_rdm12_rows(bra, [ket], norb, nelec)
    p1, p2 = dev.trans_rdm12(bra, ket, norb, nelec)
    return [ov, one, two, p1, p2, dev.contract(h1, h2, ket, norb, nelec)]


def test_equivalent_input_forms_give_the_same_bits():
    """Fortran-ordered, flattened, transposed-view and float32 arrays, torch CPU and device tensors: the bits of the
    float64 C-contiguous call (and, the data being integers, of the host).  An array is taken in its logical row-major
    order whatever its strides: ``x.T`` of an (nb, na) array is the (na, nb) vector with c[i, j] = x[j, i]."""
    from evcont_amd.fci_device import DeviceFCI
    norb, nelec = 6, (2, 3)
    na, nb = strings(norb, nelec)
    assert (na, nb) == (15, 20)
    bra, ket = integer_vectors(norb, nelec, 2, seed=66)
    h1, h2 = integer_integrals(norb, seed=67)
    base = _all_results(DeviceFCI(), bra, ket, h1, h2, norb, nelec)
    r1, r2 = _HOST.trans_rdm12(bra, ket, norb, nelec)
    assert np.array_equal(base[3], r1) and np.array_equal(base[4], r2)
    assert np.array_equal(base[5], _HOST.contract(h1, h2, ket, norb, nelec))
    dev = torch.device("cuda:0")
    forms = {
        "fortran": lambda v: np.asfortranarray(v),
        "flat": lambda v: v.reshape(-1).copy(),
        "transposed view": lambda v: np.ascontiguousarray(v.T).T,
        "float32": lambda v: v.astype(np.float32),
        "float32 fortran": lambda v: np.asfortranarray(v.astype(np.float32)),
        "torch cpu": lambda v: torch.from_numpy(v.copy()),
        "torch cpu float32": lambda v: torch.from_numpy(v.astype(np.float32)),
        "torch device": lambda v: torch.from_numpy(v).to(dev),
        "torch device transposed": lambda v: torch.from_numpy(np.ascontiguousarray(v.T)).to(dev).T,
    }
    for name, f in forms.items():
        b, k = f(bra), f(ket)
        if name in ("fortran", "transposed view"):
            assert not b.flags.c_contiguous and b.shape == (na, nb)
        got = _all_results(DeviceFCI(), b, k, h1, h2, norb, nelec)
        for x, y in zip(got, base):
            assert np.array_equal(x, y), name
    # the order is the logical one: the view ket.T, shape (nb, na), is read row by row -- the vector whose (na, nb)
    # reshape is not ket -- exactly as the host solver reads it
    view = ket.T
    assert view.shape == (nb, na) and not view.flags.c_contiguous
    as_read = np.ascontiguousarray(view).reshape(na, nb)
    assert not np.array_equal(as_read, ket)
    got = _all_results(DeviceFCI(), bra, view, h1, h2, norb, nelec)
    want = _all_results(DeviceFCI(), bra, as_read, h1, h2, norb, nelec)
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    h1v, h2v = _HOST.trans_rdm12(bra, view, norb, nelec)
    assert np.array_equal(got[3], h1v) and np.array_equal(got[4], h2v)
    assert not np.array_equal(got[4], base[4])


def test_vector_changed_in_place_is_uploaded_again():
    """The device copies of a row call are remembered per host array; an array changed in place since must give the
    RDMs of its new contents, an unchanged one is not uploaded twice, forget() drops what it is told to."""
    from evcont_amd.fci_device import DeviceFCI
    norb, nelec = 6, (3, 2)
    na, nb = strings(norb, nelec)
    dev = DeviceFCI()
    bra, k1, k2 = integer_vectors(norb, nelec, 3, seed=91)

    def host(bra, kets):
        return [_HOST.trans_rdm12(bra, k, norb, nelec) for k in kets]

    def same(got, want, bra, kets):
        for i, (r1, r2) in enumerate(want):
            assert got[0][i] == float(np.dot(bra.ravel(), kets[i].ravel()))
            assert np.array_equal(got[1][i], r1) and np.array_equal(got[2][i], r2)

    same(dev.trans_rdm12_rows(bra, [k1, k2], norb, nelec), host(bra, [k1, k2]), bra, [k1, k2])
    held = [dev._upload(v, na, nb, cache=True) for v in (bra, k1, k2)]
    same(dev.trans_rdm12_rows(bra, [k1, k2], norb, nelec), host(bra, [k1, k2]), bra, [k1, k2])
    assert all(dev._upload(v, na, nb, cache=True) is t for v, t in zip((bra, k1, k2), held))     # uploaded once
    old = host(bra, [k1, k2])
    k1 *= -1.0
    k1[0, 0] += 2.0
    new = host(bra, [k1, k2])
    assert not np.array_equal(new[0][1], old[0][1])
    same(dev.trans_rdm12_rows(bra, [k1, k2], norb, nelec), new, bra, [k1, k2])
    assert dev._upload(k2, na, nb, cache=True) is held[2] and dev._upload(k1, na, nb, cache=True) is not held[1]
    bra[1, :] = 3.0
    bra[:, 2] -= 1.0
    same(dev.trans_rdm12_rows(bra, [k1, k2, bra], norb, nelec), host(bra, [k1, k2, bra]), bra, [k1, k2, bra])
    k2[-1, -1] = np.nan                                          # a NaN never compares equal: uploaded again, not reused
    assert np.isnan(dev.trans_rdm12_rows(bra, [k2], norb, nelec)[0][0])
    k2[-1, -1] = 1.0
    same(dev.trans_rdm12_rows(bra, [k2], norb, nelec), host(bra, [k2]), bra, [k2])
    kept = dev._upload(k2, na, nb, cache=True)
    dev.forget(keep=[k2])
    assert dev._upload(k2, na, nb, cache=True) is kept and set(dev._vecs) == {id(k2)}
    same(dev.trans_rdm12_rows(bra, [k1, k2], norb, nelec), host(bra, [k1, k2]), bra, [k1, k2])
