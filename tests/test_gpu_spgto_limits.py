"""GPU tests of the device AO integrals of s and p Gaussian shells (csrc/spgto.hip) beyond one block, at the limits of
the call and per flag, through NaN-poisoned, fenced output buffers and workspace (tests/spgto_harness.py):

* B1  more than one block of every kernel (water in 6-31G: Ms = 91, 22 primitives; six s + p centres: N = 24, Ms = 300,
      five blocks with 44 threads in the last, 324 primitive pairs) against the host statement, in every flag set;
* B2  the limits natm = nshell = N = 64 with 128 primitives (s only, against ``hchain.s_gaussian_mol`` on sub-molecules
      and tests/sgto_reference.py on all centres), eight primitives
      in a shell, and N = 64 with 32 shells and 128 primitives (16 s + p centres: gridDim.y = 4096, Ms = 2080), whose
      blocks must have the bits of the same call on sub-molecules, two of which are held to the host statement;
      (the oracles of B2 are chosen by their cost on a CPU: see the tests)
* B3  each flag alone: packed forms are the packing of the full ones, a flag changes nothing but its own array;
* B4  a nucleus without basis functions.

Gate against the host statement: ``spgto_cases.DEVICE_HOST_GATE`` under ``scaled_diff``.  Worst values per array:
DESIGN.md section 8.2.1."""
import numpy as np
import pytest

import spgto_cases as sc
from evcont_amd import gto_small as gs
from evcont_amd.hchain import s_gaussian_mol
from spgto_harness import ENERGY, ENERGY_FIELDS, GRAD_FIELDS, S2KL, S4, Basis, run, run_dipole

pytestmark = pytest.mark.gpu

FLAG_SETS = (0, S4, S2KL, S4 | S2KL, ENERGY, ENERGY | S4, ENERGY | S2KL | S4)
ORIGIN = (0.3, -0.1, 0.2)
TWO = ((1.3, 0.35), (0.45, 0.65))
EIGHT = (tuple(0.05 * 3.0 ** k for k in range(8)), (0.21, -0.34, 0.48, 0.39, -0.17, 0.12, 0.06, -0.02))


def _charges(A):
    """1, 2, 0.5 in turn: a nucleus attributed to the wrong lane changes the result."""
    return [(1.0, 2.0, 0.5)[i % 3] for i in range(A)]


def _grid(shape, seed, spacing=1.9, jitter=0.2):
    """Centres on a grid of ``spacing`` Bohr, every coordinate moved by up to ``jitter``: at least 1.5 Bohr apart."""
    rng = np.random.default_rng(seed)
    R = spacing * np.stack(np.meshgrid(*[np.arange(k) for k in shape], indexing="ij"), axis=-1).reshape(-1, 3)
    R = R + jitter * rng.uniform(-1.0, 1.0, R.shape)
    d = np.linalg.norm(R[:, None] - R[None], axis=-1) + 10.0 * np.eye(len(R))
    assert d.min() >= 1.5
    return R


def _six():
    """Six s + p centres in general position, s of two primitives and p of one, other exponents on every centre."""
    R = _grid((3, 2, 1), 24, spacing=2.1, jitter=0.3)
    shells = [[gs.Shell(0, (2.1 + 0.17 * i, 0.45 + 0.04 * i), (0.4, 0.7)), gs.Shell(1, (0.9 + 0.11 * i,), (1.0,))]
              for i in range(6)]
    return R, _charges(6), shells


BIG_R = _grid((4, 2, 2), 16)
BIG_Z = _charges(16)
BIG_SHELLS = [[gs.Shell(0, tuple(e * (1.0 + 0.03 * i) for e in (6.0, 1.8, 0.6, 0.2)), (0.15, 0.4, 0.45, 0.2)),
               gs.Shell(1, tuple(e * (1.0 + 0.02 * i) for e in (3.5, 1.1, 0.4, 0.15)), (0.2, 0.45, 0.4, 0.15))]
              for i in range(16)]


def _quadruples():
    """Six sets of four atoms of the 16, each with the first and the last atom (fixed seed)."""
    rng = np.random.default_rng(16)
    out = []
    while len(out) < 6:
        mid = tuple(sorted(int(v) for v in rng.choice(np.arange(1, 15), 2, replace=False)))
        if (0,) + mid + (15,) not in out:
            out.append((0,) + mid + (15,))
    return out


QUADS = _quadruples()
# Held to the host statement, with the other 14 nuclei kept bare.  The host statement walks primitive FUNCTIONS: a
# quadruple of these centres (64 of them) takes it 55 s, a pair 2.7 s, so pairs are held; quartets over three and four
# centres reach the host through test_more_than_one_block_against_the_host_statement.
HELD = [(0, 15), (6, 15)]


def _sub(atoms, bare):
    """(R, Z, shells) of the sub-molecule of ``atoms`` (ascending) of the 16 centres.  ``bare``: all 16 nuclei stay, the
    others without functions."""
    if bare:
        return BIG_R, BIG_Z, [BIG_SHELLS[i] if i in atoms else [] for i in range(16)]
    return BIG_R[list(atoms)], [BIG_Z[i] for i in atoms], [BIG_SHELLS[i] for i in atoms]


@pytest.fixture(scope="module")
def hosts():
    """name -> (R, Basis, host statement), computed once, never changed."""
    T = sc.load_truth()
    out = {}
    a = sc.case_mol(T, "a")
    out["a"] = (a.coords, Basis(a.charges, a.shells, renormalize=False), a)
    w = gs.water("6-31g")
    out["water631"] = (w.coords, Basis(w.charges, w.shells), w)
    R, Z, shells = _six()
    out["six"] = (R, Basis(Z, shells), gs.sp_gaussian_mol(R, Z, shells))
    for atoms in HELD:
        R, Z, shells = _sub(atoms, True)
        out[atoms] = (R, Basis(Z, shells), gs.sp_gaussian_mol(R, Z, shells))
    return out


@pytest.fixture(scope="module")
def calls(hosts):
    """(name, flags) -> the result of ``run``, one call per molecule and flag set, shared by B1 and B3."""
    memo = {}

    def get(name, flags):
        if (name, flags) not in memo:
            R, basis, _ = hosts[name]
            memo[name, flags] = run(R, basis, flags)
        return memo[name, flags]
    return get


def _full(arrays, n, flags):
    """The arrays of geometry 0 with ``eri`` / ``eri_ip1`` in their full forms."""
    out = {k: v[0] for k, v in arrays.items()}
    if flags & S4:
        out["eri"] = sc.unpack_eri(out["eri"], n)
    if flags & S2KL and "eri_ip1" in out and not flags & ENERGY:
        out["eri_ip1"] = sc.unpack_ip1(out["eri_ip1"], n)
    return out


def _check_call(tag, result, mol, flags, worst):
    """What B1 asserts of one call; the largest scaled difference per array goes into ``worst``."""
    rc, arrays, intact, _ = result
    assert rc == 0, tag
    assert intact, (tag, "a guard was overwritten")
    requested = ENERGY_FIELDS if flags & ENERGY else sc.NAMES
    for name in sc.NAMES:
        if name in requested:
            assert np.all(np.isfinite(arrays[name])), (tag, name, "an element was not written")
        elif name in arrays:
            assert np.all(np.isnan(arrays[name])), (tag, name, "written by an energy-only call")
    got = _full({k: arrays[k] for k in requested}, mol.nao, flags)
    bad = []
    for name in requested:
        want = np.asarray(getattr(mol, name))
        assert got[name].shape == want.shape, (tag, name)
        d = sc.scaled_diff(got[name], want)
        worst[name] = max(worst.get(name, 0.0), d)
        if not d < sc.DEVICE_HOST_GATE:
            bad.append((name, d))
    assert not bad, (tag, bad)


def _check_dipole(tag, R, basis, mol, worst):
    rc, dip, intact, _ = run_dipole(R, basis, ORIGIN)
    assert rc == 0 and intact, tag
    assert np.all(np.isfinite(dip)), (tag, "an element was not written")
    d = sc.scaled_diff(dip[0], mol.dipole_integrals(ORIGIN))
    worst["dip"] = max(worst.get("dip", 0.0), d)
    assert d < sc.DEVICE_HOST_GATE, (tag, d)
    return dip


def _report(tag, worst):
    print(f"{tag}: worst scaled |device - host| per array: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


# ---- B1 more than one block ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["water631", "six"])
def test_more_than_one_block_against_the_host_statement(hosts, calls, name):
    R, basis, mol = hosts[name]
    assert basis.nao * (basis.nao + 1) // 2 > 64 and basis.nprim ** 2 > 256
    worst = {}
    for flags in FLAG_SETS:
        _check_call(f"{name} flags={flags}", calls(name, flags), mol, flags, worst)
    _check_dipole(name, R, basis, mol, worst)
    _report(name, worst)


# ---- B3 flags ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "six"])
def test_each_flag_alone(hosts, calls, name):
    """Packed arrays are the packing of the full ones and unpack to them, bit for bit; an array that a flag does not
    concern has the same bits in every flag set of its EVC_FLAG_ENERGY_ONLY setting; energy-only calls succeed on null
    gradient pointers; EVC_FLAG_IP1_S2KL changes nothing under EVC_FLAG_ENERGY_ONLY."""
    R, basis, mol = hosts[name]
    n = basis.nao
    res = {}
    for flags in FLAG_SETS:
        rc, arrays, intact, _ = calls(name, flags)
        assert rc == 0 and intact, flags
        res[flags] = arrays
    for base in (0, ENERGY):
        group = [f for f in FLAG_SETS if f & ENERGY == base]
        first = res[group[0]]
        for flags in group[1:]:
            for k in ("enuc", "S", "hcore", "ipovlp", "dhcore", "gnuc"):
                assert np.array_equal(res[flags][k], first[k], equal_nan=True), (flags, k)
        full_eri = res[base]["eri"]
        for flags in group:
            if flags & S4:
                assert np.array_equal(sc.unpack_eri(res[flags]["eri"][0], n), full_eri[0]), (flags, "eri")
            else:
                assert np.array_equal(res[flags]["eri"], full_eri), (flags, "eri")
    full_ip1 = res[0]["eri_ip1"]
    assert np.all(np.isfinite(full_ip1))
    for flags in (S4, S2KL, S4 | S2KL):
        if flags & S2KL:
            assert np.array_equal(sc.unpack_ip1(res[flags]["eri_ip1"][0], n), full_ip1[0]), (flags, "eri_ip1")
        else:
            assert np.array_equal(res[flags]["eri_ip1"], full_ip1), (flags, "eri_ip1")
    for flags in (ENERGY, ENERGY | S4, ENERGY | S2KL | S4, ENERGY | S2KL):
        twin = res[flags & ~S2KL]
        rc, arrays, intact, bufs = run(R, basis, flags, null_grad=True)
        assert rc == 0 and intact and sorted(bufs) == sorted(ENERGY_FIELDS), flags
        for k in ENERGY_FIELDS:
            assert np.array_equal(arrays[k], twin[k]), (flags, k, "null gradient pointers")
        if flags == ENERGY | S2KL:
            rc, arrays, intact, _ = run(R, basis, flags)
            assert rc == 0 and intact
        else:
            arrays = res[flags]
        for k in ENERGY_FIELDS:
            assert np.array_equal(arrays[k], twin[k]), (flags, k)
        for k in GRAD_FIELDS:
            assert np.all(np.isnan(arrays[k])), (flags, k)


# ---- B2 the limits -------------------------------------------------------------------------------------------------
def _against_hchain(tag, R, Z, contraction):
    A = len(Z)
    shells = [[gs.Shell(0, *contraction)] for _ in range(A)]
    basis = Basis(Z, shells, renormalize=False)
    mol = s_gaussian_mol(R, Z, *contraction)
    worst = {}
    for flags in (0, S4 | S2KL):
        _check_call(f"{tag} flags={flags}", run(R, basis, flags), mol, flags, worst)
    rc, dip, intact, _ = run_dipole(R, basis, ORIGIN)
    assert rc == 0 and intact and np.all(np.isfinite(dip))
    worst["dip"] = sc.scaled_diff(dip[0], mol.dipole_integrals(ORIGIN))
    assert worst["dip"] < sc.DEVICE_HOST_GATE
    _report(tag, worst)
    return basis


def test_s_only_at_64_centres_64_shells_128_primitives():
    """natm = nshell = N = 64 with 128 primitives.  ``s_gaussian_mol`` on all 64 centres of two primitives takes 105 s on
    a CPU (4.4 s with one primitive), so it is the oracle where it is affordable: S, ipovlp, eri and eri_ip1, which do
    not depend on the other nuclei, on three sub-molecules of 16 centres that hold the first and the last one.  The
    arrays that see all 64 nuclei are compared in full with ``sgto_reference.one_electron``, and twelve bra rows of eri
    and eri_ip1 over all kets with ``sgto_reference.eri_rows``, the statements tests/test_gpu_sgto_limits.py uses at 96
    centres.  The packed forms unpack to the full ones and eri is exactly symmetric."""
    import sgto_reference as ref
    A = 64
    R, Z = _grid((4, 4, 4), 64), _charges(A)
    basis = Basis(Z, [[gs.Shell(0, *TWO)] for _ in range(A)], renormalize=False)
    assert (basis.natm, basis.nshell, basis.nao, basis.nprim) == (64, 64, 64, 128)
    rc, arrays, intact, _ = run(R, basis, 0)
    assert rc == 0 and intact
    rc, packed, intact, _ = run(R, basis, S4 | S2KL)
    assert rc == 0 and intact
    for res in (arrays, packed):
        for k, v in res.items():
            assert np.all(np.isfinite(v)), (k, "an element was not written")
    full = {k: v[0] for k, v in arrays.items()}
    assert np.array_equal(sc.unpack_eri(packed["eri"][0], A), full["eri"])
    assert np.array_equal(sc.unpack_ip1(packed["eri_ip1"][0], A), full["eri_ip1"])
    for k in ("enuc", "S", "hcore", "ipovlp", "dhcore", "gnuc"):
        assert np.array_equal(packed[k][0], full[k]), k
    assert np.array_equal(full["eri"], full["eri"].transpose(1, 0, 2, 3))
    assert np.array_equal(full["eri"], full["eri"].transpose(0, 1, 3, 2))
    assert np.array_equal(full["eri_ip1"], full["eri_ip1"].transpose(0, 1, 2, 4, 3))
    worst = {}

    def hold(name, got, want):
        d = sc.scaled_diff(got, want)
        worst[name] = max(worst.get(name, 0.0), d)
        assert d < sc.DEVICE_HOST_GATE, (name, d)

    for name, (want, _, _, _) in ref.one_electron(R, Z, *TWO).items():
        hold(name, full[name], want)
    rng = np.random.default_rng(64)
    pairs = [(0, 0), (63, 63), (63, 0), (0, 63)] + [tuple(int(v) for v in rng.integers(0, A, 2)) for _ in range(8)]
    rows = ref.eri_rows(R, *TWO, pairs)
    for b, (i, j) in enumerate(pairs):
        hold("eri", full["eri"][i, j], rows["eri"][0][b])
        hold("eri_ip1", full["eri_ip1"][:, i, j], rows["eri_ip1"][0][b])
    rc, dip, intact, _ = run_dipole(R, basis, ORIGIN)
    assert rc == 0 and intact and np.all(np.isfinite(dip))
    for mid in (range(1, 15), range(25, 39), range(49, 63)):
        ix = np.array([0] + list(mid) + [63])
        mol = s_gaussian_mol(R[ix], [Z[i] for i in ix], *TWO)
        i2, i4 = np.ix_(ix, ix), np.ix_(ix, ix, ix, ix)
        hold("S", full["S"][i2], mol.S)
        hold("ipovlp", full["ipovlp"][(slice(None),) + i2], mol.ipovlp)
        hold("eri", full["eri"][i4], mol.eri)
        hold("eri_ip1", full["eri_ip1"][(slice(None),) + i4], mol.eri_ip1)
        hold("dip", dip[0][(slice(None),) + i2], mol.dipole_integrals(ORIGIN))
    _report("s64", worst)


def test_eight_primitives_in_a_shell():
    basis = _against_hchain("s8_K8", _grid((2, 2, 2), 8), _charges(8), EIGHT)
    assert basis.nprim == 64 and int(np.diff(basis.shell_prim_offset).max()) == 8


def _ao(atoms):
    return np.concatenate([np.arange(4 * i, 4 * i + 4) for i in atoms])


@pytest.fixture(scope="module")
def big():
    """The 16 s + p centres in the full forms: ({name: array of geometry 0}, dipole integrals, Basis)."""
    basis = Basis(BIG_Z, BIG_SHELLS)
    assert (basis.natm, basis.nshell, basis.nao, basis.nprim) == (16, 32, 64, 128)
    assert int(basis.shell_prim_offset[-2]) == 124
    rc, arrays, intact, _ = run(BIG_R, basis, 0)
    assert rc == 0 and intact
    for k, v in arrays.items():
        assert np.all(np.isfinite(v)), (k, "an element was not written")
    rc, dip, intact, _ = run_dipole(BIG_R, basis, ORIGIN)
    assert rc == 0 and intact and np.all(np.isfinite(dip))
    return {k: v[0] for k, v in arrays.items()}, dip[0], basis


def test_n64_packed_forms_unpack_to_the_full_ones(big):
    full, _, basis = big
    rc, arrays, intact, _ = run(BIG_R, basis, S4 | S2KL)
    assert rc == 0 and intact
    for k, v in arrays.items():
        assert np.all(np.isfinite(v)), (k, "an element was not written")
    assert np.array_equal(sc.unpack_eri(arrays["eri"][0], 64), full["eri"])
    assert np.array_equal(sc.unpack_ip1(arrays["eri_ip1"][0], 64), full["eri_ip1"])
    for k in ("enuc", "S", "hcore", "ipovlp", "dhcore", "gnuc"):
        assert np.array_equal(arrays[k][0], full[k]), k


def test_n64_blocks_have_the_bits_of_the_sub_molecules(big, hosts):
    """Each thread reads only the pair-table rows of its own functions and walks nuclei and primitives in ascending
    order, so a block of the big molecule has the bits of the same call on the sub-molecule of its atoms: S, ipovlp, eri,
    eri_ip1 and the dipole integrals on the atoms alone, hcore and dhcore (all 16 atom rows) with the other 15 nuclei
    kept bare.  Two sub-molecules (HELD) are held to the host statement: truth -> host -> small device -> big device."""
    full, dip, _ = big
    pairs = [(0, j) for j in range(1, 16)] + [(i, 15) for i in range(1, 15)]
    unequal = []
    worst = {}
    for atoms in pairs + QUADS:
        ix = _ao(atoms)
        i2, i4 = np.ix_(ix, ix), np.ix_(ix, ix, ix, ix)
        want = {"S": full["S"][i2], "hcore": full["hcore"][i2], "eri": full["eri"][i4],
                "ipovlp": full["ipovlp"][(slice(None),) + i2], "eri_ip1": full["eri_ip1"][(slice(None),) + i4],
                "dhcore": full["dhcore"][(slice(None), slice(None)) + i2], "enuc": full["enuc"], "gnuc": full["gnuc"]}
        for bare in (False, True):
            R, Z, shells = _sub(atoms, bare)
            basis = Basis(Z, shells)
            rc, arrays, intact, _ = run(R, basis, 0)
            assert rc == 0 and intact, (atoms, bare)
            if bare:
                assert np.array_equal(basis.aoslices[:, 1] - basis.aoslices[:, 0], [4 * (i in atoms) for i in range(16)])
            rc, sub_dip, intact, _ = run_dipole(R, basis, ORIGIN)
            assert rc == 0 and intact, (atoms, bare)
            names = sc.NAMES if bare else ("S", "ipovlp", "eri", "eri_ip1")
            for k in names:
                if not np.array_equal(arrays[k][0], want[k]):
                    unequal.append((atoms, bare, k, sc.scaled_diff(arrays[k][0], want[k])))
            if not np.array_equal(sub_dip[0], dip[(slice(None),) + i2]):
                unequal.append((atoms, bare, "dip"))
            if bare and atoms in HELD:
                mol = hosts[atoms][2]
                _check_call(f"sub-molecule {atoms} bare={bare}", (rc, arrays, intact, None), mol, 0, worst)
                d = sc.scaled_diff(sub_dip[0], mol.dipole_integrals(ORIGIN))
                worst["dip"] = max(worst.get("dip", 0.0), d)
                assert d < sc.DEVICE_HOST_GATE
    _report("sub-molecules of the 16 centres", worst)
    assert not unequal, unequal


# ---- B4 a nucleus without basis functions --------------------------------------------------------------------------
@pytest.mark.parametrize("where", [1, 3])
def test_bare_nucleus(where):
    """A point charge without shells in STO-3G water, as the middle atom and as the last."""
    from evcont_amd.gto_device import DeviceGaussians
    w = gs.water("sto-3g")
    R = np.insert(w.coords, where, [0.9, -1.1, 0.7], axis=0)
    Z = np.insert(w.charges, where, 1.5)
    shells = list(w.shells)
    shells.insert(where, [])
    mol = gs.sp_gaussian_mol(R, Z, shells)
    basis = Basis(Z, shells)
    assert np.array_equal(basis.aoslices, mol.aoslices) and mol.aoslices[where, 0] == mol.aoslices[where, 1]
    worst = {}
    for flags in (0, S4 | S2KL, ENERGY):
        result = run(R, basis, flags)
        _check_call(f"bare nucleus at {where} flags={flags}", result, mol, flags, worst)
        if flags == 0:
            arrays = result[1]
    _check_dipole(f"bare nucleus at {where}", R, basis, mol, worst)
    _report(f"bare nucleus at {where}", worst)
    for k in ("gnuc", "dhcore"):
        row = arrays[k][0, where]
        assert np.all(np.isfinite(row)) and np.abs(row).max() > 1e-3, k
    dg = DeviceGaussians.from_mol(mol, device="cuda")
    aob = dg.integrals(R)
    assert np.array_equal(aob.aoslices.cpu().numpy(), mol.aoslices)
    for k in sc.NAMES:
        assert np.array_equal(getattr(aob, k).cpu().numpy(), arrays[k]), k
