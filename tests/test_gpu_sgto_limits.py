"""GPU tests of the device AO integrals of s-Gaussian molecules (csrc/sgto.hip, hchain_device.py) at their limits, through
NaN-poisoned, fenced output buffers and workspace (tests/sgto_harness.py):

* against the exact values of tests/golden/sgto_truth.npz (mpmath) within the bound of tests/sgto_reference.py,
  2^-53 [(n_terms + 32) sum|terms| + c cancel + cond] with c = C_CANCEL: Boys arguments on either side of the switch at
  t = 1e-2, centres 40 Bohr apart (Kab exactly 0, t in the thousands), eight primitives;
* more than 64 centres (the second round of nuclei of ``sgto_one_kernel``, the second wave of ``sgto_nuc_kernel``), the
  packed limit of 64 and the limit of 96, charges 1, 2, 0.5 in turn, against ``s_gaussian_mol`` / ``one_electron`` /
  ``eri_rows``.  Two float64 routes of one statement share the roundings of Kab and P, so no ``cond`` here
  (``sgto_reference.allowed_pair``): 2^-53 [(n_terms + 32) sum|terms| + 2 C_CANCEL cancel] + 2^-1022;
* eight primitives on three centres with the bit identities of tests/test_gpu_sgto.py;
* the documented paths of ``DeviceSGaussians`` against a direct call on the same inputs, bit for bit.

Worst ratios per case and array: DESIGN.md section 8.2."""
import os

import numpy as np
import pytest
import torch

import sgto_reference as ref
from evcont_amd.hchain import STO6G_H_COEFFICIENTS, STO6G_H_EXPONENTS, s_gaussian_mol
from sgto_harness import DEV, GRAD_FIELDS, MODES, run, unpack

pytestmark = pytest.mark.gpu

TRUTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sgto_truth.npz")
CASES = ("3c_spread1.5_K3", "4c_K1", "K8", "far", "far_K1", "switch_K1", "switch_K3")
ENERGY_FIELDS = ("enuc", "S", "hcore", "eri")
ONE = ((0.4,), (1.0,))
TWO = ((1.3, 0.35), (0.45, 0.65))
EIGHT = (tuple(0.05 * 3.0 ** k for k in range(8)), (0.21, -0.34, 0.48, 0.39, -0.17, 0.12, 0.06, -0.02))


def _charges(A):
    """1, 2, 0.5 in turn: a nucleus attributed to the wrong lane changes the result."""
    return [(1.0, 2.0, 0.5)[i % 3] for i in range(A)]


def _full(arrays, A, mode):
    """The arrays of a call with ``eri`` / ``eri_ip1`` in their full forms."""
    if mode != "packed":
        return arrays
    eri, ip1 = unpack(arrays, A)
    return dict(arrays, eri=eri, eri_ip1=ip1)


# ---- C.1 the device against the exact values -------------------------------------------------------------------
@pytest.fixture(scope="module", params=CASES)
def truth(request):
    case = request.param
    with np.load(TRUTH) as T:
        R, Z, ex, co = (T[f"{case}/{k}"] for k in ("R", "Z", "ex", "co"))
        fields = {}
        for name in ref.NAMES:
            hi, lo, ab = T[f"{case}/{name}_hi"], T[f"{case}/{name}_lo"].astype(np.float64), T[f"{case}/{name}_abs"]
            zero = np.zeros_like(ab)
            fields[name] = (hi, lo, ab, T[f"{case}/{name}_cancel"] if name in ref.CANCEL_FIELDS else zero,
                            T[f"{case}/{name}_cond"] if f"{case}/{name}_cond" in T.files else zero)
    return case, R, len(ex), fields, {m: run(R, Z, (ex, co), m) for m in MODES}


def test_device_against_the_exact_values(truth):
    case, R, K, fields, res = truth
    A = R.shape[1]
    failures = []
    for mode, (rc, arrays, intact, _) in res.items():
        assert rc == 0 and intact, mode
        arrays = _full(arrays, A, mode)
        for name in ref.NAMES:
            if mode == "energy" and name in GRAD_FIELDS:
                assert np.all(np.isnan(arrays[name])), (mode, name)
                continue
            hi, lo, ab, cancel, cond = fields[name]
            got = arrays[name].reshape(hi.shape)
            assert np.all(np.isfinite(got)), (mode, name)
            assert np.all(got[ab == 0.0] == 0.0), (mode, name, "an element whose addends all vanish is not exactly 0")
            ratio = ref.truth_ratio(name, A, K, got, hi, lo, ab, cancel, cond)
            bare = ref.worst_ratio(name, A, K, got - hi, lo, ab)
            print(f"{case} {mode} {name}: worst |device - truth| = {ratio:.3f} x bound "
                  f"({bare:.1f} x 2^-53 sum|terms|)")
            if not ratio <= 1.0:
                failures.append((mode, name, ratio))
    assert not failures, failures


# ---- C.2 more than 64 centres ----------------------------------------------------------------------------------------
_host_bound = ref.allowed_pair


def _units(got, want, ab):
    """Largest |got - want| in units of 2^-53 sum|terms| over the elements whose 2^-53 sum|terms| is a normal number (a long
    chain has elements down to exact 0 through the subnormal range): for the record."""
    err, ab = np.abs(np.asarray(got) - np.asarray(want)), np.asarray(ab)
    big = ab > 2.0 ** -960
    return float(np.max(err[big] / (2.0 ** -53 * ab[big]))) if np.any(big) else 0.0


def _host_sums(R, Z, basis):
    """{name: (sum|terms|, cancel)} of every array of one geometry, without the primitives^4 pass of ``abs_sums``."""
    A = len(Z)
    sums = {k: (ab, cc) for k, (_, ab, cc, _) in ref.one_electron(R, Z, *basis).items()}
    rows = ref.eri_rows(R, *basis, [(i, j) for i in range(A) for j in range(A)])
    sums["eri"] = (rows["eri"][1].reshape(A, A, A, A), rows["eri"][2].reshape(A, A, A, A))
    sums["eri_ip1"] = tuple(np.moveaxis(rows["eri_ip1"][f].reshape(A, A, 3, A, A), 2, 0) for f in (1, 2))
    return sums


def _against_host(tag, arrays, names, mol, sums, A, K):
    failures = []
    for name in names:
        got, want = arrays[name][0], np.asarray(getattr(mol, name))
        ab, cancel = sums[name]
        assert np.all(np.isfinite(got)), (tag, name)
        err = np.abs(got - want)
        print(f"{tag} {name}: worst |device - s_gaussian_mol| = {_units(got, want, ab):.1f} x 2^-53 "
              f"sum|terms|, {float(np.max(err / np.maximum(_host_bound(name, A, K, ab, cancel), 1e-300))):.3f} x bound")
        if not np.all(err <= _host_bound(name, A, K, ab, cancel)):
            failures.append((tag, name))
    assert not failures, failures


@pytest.fixture(scope="module", params=[64, 65])
def chain(request):
    A = request.param
    R, Z = ref._perturbed_chain(A, 1, 60 + A), _charges(A)
    return A, R, Z, s_gaussian_mol(R[0], Z, *ONE), _host_sums(R[0], Z, ONE)


def test_64_and_65_centres_against_s_gaussian_mol(chain):
    """64: the packed limit, packed with derivatives.  65: the smallest shape in the second round of nuclei, full with
    derivatives and energy-only."""
    A, R, Z, mol, sums = chain
    if A == 64:
        rc, arrays, intact, _ = run(R, Z, ONE, "packed")
        assert rc == 0 and intact
        _against_host("A64 packed", _full(arrays, A, "packed"), ref.NAMES, mol, sums, A, 1)
        return
    rc, full, intact, _ = run(R, Z, ONE, "full")
    assert rc == 0 and intact
    _against_host("A65 full", full, ref.NAMES, mol, sums, A, 1)
    rc, energy, intact, _ = run(R, Z, ONE, "energy")
    assert rc == 0 and intact
    _against_host("A65 energy-only", energy, ENERGY_FIELDS, mol, sums, A, 1)
    for name in ENERGY_FIELDS:
        assert np.array_equal(energy[name], full[name]), name
    for name in GRAD_FIELDS:
        assert np.all(np.isnan(energy[name])), name
    for name in ("S", "hcore"):
        assert np.array_equal(full[name], np.swapaxes(full[name], 1, 2)), name


def test_96_centres_two_primitives():
    """The limit: eri_ip1 is 2.0 GB and stays on the device; the one-electron arrays in full against ``one_electron``,
    fifteen bra rows of eri / eri_ip1 over all kets against ``eri_rows``, the exact symmetries on the device."""
    A, K = 96, 2
    R, Z = ref._perturbed_chain(A, 1, 96), _charges(A)
    small = ("enuc", "gnuc", "S", "hcore", "ipovlp", "dhcore")
    rc, arrays, intact, bufs = run(R, Z, TWO, "full", fetch=small)
    assert rc == 0 and intact
    failures = []
    for name, (want, ab, cancel, _) in ref.one_electron(R[0], Z, *TWO).items():
        got = arrays[name][0]
        assert np.all(np.isfinite(got)), name
        bound = _host_bound(name, A, K, ab, cancel)
        err = np.abs(got - want)
        print(f"A96 {name}: worst |device - one_electron| = {_units(got, want, ab):.1f} x 2^-53 "
              f"sum|terms|, {float(np.max(err / np.maximum(bound, 1e-300))):.3f} x bound")
        if not np.all(err <= bound):
            failures.append(name)
    rng = np.random.default_rng(9)
    pairs = [(0, 0), (95, 95), (95, 0), (0, 95), (64, 63), (63, 64), (70, 70)] + \
            [tuple(int(v) for v in rng.integers(0, A, 2)) for _ in range(8)]
    rows = ref.eri_rows(R[0], *TWO, pairs)
    n = A
    for b, (i, j) in enumerate(pairs):
        for name, got in (("eri", bufs["eri"].rows((1, n, n, n, n), (0, i, j))),
                          ("eri_ip1", bufs["eri_ip1"].device((1, 3, n, n, n, n))[0, :, i, j].cpu().numpy())):
            want, ab, cancel, _ = (rows[name][f][b] for f in range(4))
            bound = _host_bound(name, A, K, ab, cancel)
            err = np.abs(got - want)
            print(f"A96 {name} row ({i},{j}): worst |device - eri_rows| = {_units(got, want, ab):.1f} "
                  f"x 2^-53 sum|terms|, {float(np.max(err / np.maximum(bound, 1e-300))):.3f} x bound")
            if not (np.all(np.isfinite(got)) and np.all(err <= bound)):
                failures.append((name, i, j))
    assert not failures, failures
    eri, ip1 = bufs["eri"].device((n, n, n, n)), bufs["eri_ip1"].device((3, n, n, n, n))
    assert bool(torch.isfinite(eri).all()) and bool(torch.isfinite(ip1).all())
    assert torch.equal(eri, eri.transpose(0, 1))
    assert torch.equal(eri, eri.transpose(2, 3))
    assert torch.equal(ip1, ip1.transpose(3, 4))
    rc, energy, intact, ebufs = run(R, Z, TWO, "energy", fetch=("hcore", "S", "enuc"))
    assert rc == 0 and intact
    assert torch.equal(ebufs["eri"].device(), bufs["eri"].device())
    for name in ("hcore", "S", "enuc"):
        assert np.array_equal(energy[name], arrays[name]), name
    assert bool(torch.isnan(ebufs["eri_ip1"].device()).all()) and bool(torch.isnan(ebufs["dhcore"].device()).all())


# ---- C.3 eight primitives beyond two centres -----------------------------------------------------------------------
def test_eight_primitives_on_three_centres():
    A, K, G = 3, 8, 2
    R, Z = ref._perturbed_chain(A, G, 38), [1.0, 2.0, 0.5]
    res = {m: run(R, Z, EIGHT, m) for m in MODES}
    for mode, (rc, _, intact, _) in res.items():
        assert rc == 0 and intact, mode
    packed, full, energy = (res[m][1] for m in ("packed", "full", "energy"))
    failures = []
    for g in range(G):
        mol = s_gaussian_mol(R[g], Z, *EIGHT)
        sums, cancel, _ = ref.abs_sums(R[g], Z, *EIGHT, with_cancel=True)
        for name in ref.NAMES:
            got, want = full[name][g], np.asarray(getattr(mol, name))
            assert np.all(np.isfinite(got)), name
            bound = _host_bound(name, A, K, sums[name], cancel.get(name, 0.0))
            err = np.abs(got - want)
            print(f"A3_K8 g{g} {name}: worst |device - s_gaussian_mol| = "
                  f"{_units(got, want, sums[name]):.1f} x 2^-53 sum|terms|, "
                  f"{float(np.max(err / np.maximum(bound, 1e-300))):.3f} x bound")
            if not np.all(err <= bound):
                failures.append((g, name))
    assert not failures, failures
    eri, ip1 = unpack(packed, A)
    assert np.array_equal(full["eri"], eri) and np.array_equal(full["eri_ip1"], ip1)
    for name in ("enuc", "S", "hcore", "ipovlp", "dhcore", "gnuc"):
        assert np.array_equal(full[name], packed[name]), name
    for name in ENERGY_FIELDS:
        assert np.array_equal(energy[name], full[name]), name
    for name in GRAD_FIELDS:
        assert np.all(np.isnan(energy[name])), name
    for g in range(G):
        rc, single, intact, _ = run(R[g:g + 1], Z, EIGHT, "packed")
        assert rc == 0 and intact
        for name, v in packed.items():
            assert np.array_equal(v[g], single[name][0]), (g, name)


# ---- C.4 DeviceSGaussians against a direct call, bit for bit -------------------------------------------------------
STO6G = (STO6G_H_EXPONENTS, STO6G_H_COEFFICIENTS)
Z3 = [1.0, 2.0, 0.5]


def _same(aob_or_dict, arrays, names=ref.NAMES):
    get = (lambda k: aob_or_dict[k]) if isinstance(aob_or_dict, dict) else (lambda k: getattr(aob_or_dict, k))
    for name in names:
        got = get(name).cpu().numpy()
        assert got.shape == arrays[name].shape, (name, got.shape, arrays[name].shape)
        assert np.array_equal(got, arrays[name]), name


def _direct(R, basis=STO6G, mode="full", Z=Z3):
    rc, arrays, intact, _ = run(np.asarray(R, dtype=np.float64).reshape((-1,) + np.shape(R)[-2:]), Z, basis, mode)
    assert rc == 0 and intact
    return arrays


@pytest.fixture()
def sg():
    from evcont_amd.hchain_device import DeviceSGaussians
    return DeviceSGaussians(charges=Z3, exponents=STO6G[0], coefficients=STO6G[1])


def test_wrapper_takes_one_geometry_as_A_by_3(sg):
    R = ref._perturbed_chain(3, 1, 41)[0]
    want = _direct(R)
    _same(sg.integrals(R), want)
    _same(sg.integrals(torch.from_numpy(R).to(DEV)), want)
    _same(sg.integrals(R, packed=True), _direct(R, mode="packed"))
    aob = sg.integrals(R, need_grad=False)
    _same(aob, _direct(R, mode="energy"), ENERGY_FIELDS)
    assert aob.ipovlp is None and aob.dhcore is None and aob.eri_ip1 is None and aob.gnuc is None


def test_wrapper_writes_into_out_and_leaves_its_own_buffers(sg):
    R = ref._perturbed_chain(3, 2, 42)
    first = sg.integrals(R[:1])
    want_first = _direct(R[:1])
    out = sg.allocate(1)
    for v in out.values():
        v.fill_(float("nan"))
    aob = sg.integrals(R[1:], out=out)
    want = _direct(R[1:])
    _same(out, want)
    _same(aob, want)
    assert all(getattr(aob, k).data_ptr() == out[k].data_ptr() for k in ref.NAMES)
    _same(first, want_first)                                            # the kept buffers: not written
    packed = sg.allocate(1, need_grad=False, packed=True)
    assert sorted(packed) == sorted(ENERGY_FIELDS)
    sg.integrals(R[1:], need_grad=False, packed=True, out=packed)
    _same(packed, _direct(R[1:], mode="packed"), ENERGY_FIELDS)      # the energy-only eri has the bits of the full call's


def test_wrapper_from_mol_carries_charges_contraction_and_electrons():
    from evcont_amd.hchain_device import DeviceSGaussians
    R = ref._perturbed_chain(3, 2, 43)
    mol = s_gaussian_mol(R[0], Z3, *STO6G, need_grad=False, nelec=(2, 1))
    sg = DeviceSGaussians.from_mol(mol)
    assert sg.nelec == (2, 1)
    _same(sg.integrals(R), _direct(R))
    assert np.array_equal(sg._charges.cpu().numpy(), np.asarray(Z3)) and sg.natm == 3


def test_wrapper_takes_float32_and_strided_device_tensors(sg):
    R = ref._perturbed_chain(3, 2, 44)
    r32 = torch.from_numpy(R).to(DEV).to(torch.float32)
    _same(sg.integrals(r32), _direct(r32.to(torch.float64).cpu().numpy()))
    wide = torch.full((2, 3, 6), 7.0, dtype=torch.float64, device=DEV)
    view = wide[:, :, ::2]
    view.copy_(torch.from_numpy(R))
    assert not view.is_contiguous()
    _same(sg.integrals(view), _direct(R))
    assert bool((wide[:, :, 1::2] == 7.0).all())


def test_wrapper_regrows_its_workspace_and_keeps_buffers_per_batch_size(sg):
    R = ref._perturbed_chain(3, 9, 45)
    first = sg.integrals(R[:2])
    ptrs = {k: getattr(first, k).data_ptr() for k in ref.NAMES}
    _same(first, _direct(R[:2]))
    small = sg._ws.numel()
    nine = sg.integrals(R)
    assert sg._ws.numel() > small
    _same(nine, _direct(R))
    _same(first, _direct(R[:2]))                                        # untouched by the larger call
    again = sg.integrals(R[7:])
    assert {k: getattr(again, k).data_ptr() for k in ref.NAMES} == ptrs
    _same(again, _direct(R[7:]))
    _same(nine, _direct(R))


def test_wrapper_refuses_another_molecule_size_and_leaves_its_buffers(sg):
    R = ref._perturbed_chain(3, 2, 46)
    kept = sg.integrals(R)
    want = _direct(R)
    other = ref._perturbed_chain(4, 2, 47)
    for bad in (other, other[0], torch.from_numpy(other).to(DEV)):
        with pytest.raises(ValueError, match="4 centres for a molecule of 3"):
            sg.integrals(bad)
    torch.cuda.synchronize()
    _same(kept, want)
    _same(sg.integrals(R), want)


def test_wrapper_enqueues_on_the_current_stream():
    from evcont_amd.hchain_device import DeviceSGaussians
    R = ref._perturbed_chain(3, 4, 48)
    want, want_packed = _direct(R), _direct(R, mode="packed")
    rt = torch.from_numpy(R).to(DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(s):
        sg = DeviceSGaussians(charges=Z3, exponents=STO6G[0], coefficients=STO6G[1])
        on_tensor = sg.integrals(rt)
        s.synchronize()
        _same(on_tensor, want)
        on_host = sg.integrals(R, packed=True)
        s.synchronize()
        _same(on_host, want_packed)
