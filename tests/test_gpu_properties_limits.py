"""The observables kernels (csrc/properties.hip: evc_properties_roots_batch, evc_sgto_dipole_batch) where their
mechanisms can fail and tests/test_gpu_properties.py does not look: inputs of which nothing is symmetric (an index choice
then differs from its transpose), every instantiation of prop_d1_kernel and the edges of its 32-slot groups, root pairs
beyond word 0 of the diagonal mask up to the 4096 slots of a call, the row chunks at their edges up to T = 512, atom
loops that go round twice and slices that are empty, out of order or beyond N, one block and several of
prop_sdip_kernel up to 96 centres, 8 primitives and 65535 geometries, and the chunked loop of
get_multistate_properties.  Every call of the ABI writes into NaN-poisoned outputs and scratch between guards
(tests/properties_harness.py) and is compared with the numpy statement evcont_amd/properties.py at the project's bar of
1e-10 absolute (coordinates within 10 Bohr).  What of this needs no device (the tables below against the ladder and the
constants in the source, the chunk arithmetic, that the inputs can tell a transpose from the truth) is asserted in
tests/test_properties_limits_host.py as well.  Worst deviations of a device run: DESIGN.md section 4.9."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from properties_harness import BAR, DEV, OUTPUTS, REPO, Problem, compare, source_constant

pytestmark = pytest.mark.gpu

DIAG3 = [(0, 0), (0, 1), (1, 1)]


def all_pairs(nvec):
    return [(k, l) for k in range(nvec) for l in range(k, nvec)]


def check_fenced(pb, what, want=OUTPUTS):
    """One call into fenced buffers: the guards stand, and every output is the reference at the bar."""
    got, intact = pb.call(want)
    assert intact, (what, "a guard of an output or of the scratch was written")
    return got, compare(got, {k: pb.reference()[k] for k in got}, what)


# ---- 1. inputs of which nothing is symmetric ----------------------------------------------------------------------------
# n, T, G, pairs, AO counts per atom: one N per tiling of prop_ao_kernel (TM = 2, 4, 6), none a multiple of 16, and the limit
NONSYM_SHAPES = [
    (7, 3, 2, DIAG3, (1, 4, 2)),
    (37, 3, 2, DIAG3, (17, 1, 19)),
    (83, 2, 2, DIAG3, (40, 42, 1)),
    (96, 2, 2, DIAG3, (1, 47, 48)),
]
TELLS = 1e-3


def nonsym_problem(shape, **kw):
    n, T, G, pairs, sizes = shape
    return Problem(n, T, G, pairs, sizes, seed=900 + n, symmetric=False, fenced=True, **kw)


def can_tell_a_transpose(pb, ref):
    """(max |P - P^T|, max |Mulliken with S^T - Mulliken|, max |D - D^T|, max |tr(P^T r) - tr(P r)|) of a problem: how
    far the answer of a kernel with a transposed index would be from the reference."""
    from evcont_amd import properties as pr
    P, D = ref["d_ao"], ref["d_oao"]
    mull = np.stack([[pr.mulliken_pop(P[p, g], pb.S[g].T, pb.aoslices) for g in range(pb.G)] for p in range(len(pb.pairs))])
    trT = np.einsum("gxij,pgij->pgx", pb.dip, P) - np.einsum("gxij,pgji->pgx", pb.dip, P)
    return (float(np.abs(P - np.swapaxes(P, -1, -2)).max()), float(np.abs(mull - ref["mulliken"]).max()),
            float(np.abs(D - np.swapaxes(D, -1, -2)).max()), float(np.abs(trT).max()))


@pytest.mark.parametrize("shape", NONSYM_SHAPES, ids=[f"n{s[0]}" for s in NONSYM_SHAPES])
def test_nothing_symmetric(shape):
    pb = nonsym_problem(shape)
    tells = can_tell_a_transpose(pb, pb.reference())
    print(f"n={shape[0]}: a transposed P, S, D, tr(P r) would be off by {tells}")
    assert min(tells) > TELLS, tells
    check_fenced(pb, f"nothing symmetric, n={shape[0]}:")


# ---- 2. every NS and the edges of the 32-slot groups --------------------------------------------------------------------
# total slots = count x pairs (n = 5, T = 9; the first pairs of all_pairs(9)), and the instantiation of prop_d1_kernel that
# the ladder of evc_properties_roots_batch picks for each group of 32 consecutive slots.  Where the total allows it, count
# does not divide 32, so that a group ends inside a pair and (s0 + s) % count, (s0 + s) / count step inside a group.
SLOT_SHAPES = [
    # slots, count, pairs, NS per group
    (3, 3, 1, (4,)),               # <4>, one absent slot
    (4, 2, 2, (4,)),               # <4>, full
    (5, 5, 1, (8,)),               # <8>, three absent
    (9, 3, 3, (16,)),              # <16>, seven absent
    (16, 4, 4, (16,)),             # <16>, full
    (17, 17, 1, (32,)),            # <32>, fifteen absent
    (31, 31, 1, (32,)),            # <32>, one absent slot; one pair
    (31, 1, 31, (32,)),            # <32>, one absent slot; one geometry, 31 pairs
    (32, 2, 16, (32,)),            # <32>, a full group
    (34, 17, 2, (32, 2)),          # <32> full, then <2>
    (64, 32, 2, (32, 32)),         # two full groups, each one pair
    (64, 2, 32, (32, 32)),         # two full groups of 16 pairs
    (45, 1, 45, (32, 16)),         # every pair of nvec = 9: <32> full, then 13 slots in <16>
    (135, 3, 45, (32, 32, 32, 32, 8)),   # the same pairs, three geometries: four full groups, then 7 slots in <8>
]
SLOT_N, SLOT_T = 5, 9


def ladder():
    """[(largest ns, NS)] of the dispatch ladder in evc_properties_roots_batch, and the slots of a group, read from the
    source."""
    with open(os.path.join(REPO, "evcont_amd", "csrc", "properties.hip")) as f:
        src = f.read()
    rungs = re.findall(r"(?:if \(ns (==|<=) (\d+)\)|else) prop_d1_go<(\d+)>", src)
    group = source_constant("kPropGroup")
    return [(int(top) if op else group, int(ns)) for op, top, ns in rungs], group


def instantiations(nslots):
    """NS of every launch of prop_d1_kernel for a call of ``nslots`` slots."""
    rungs, group = ladder()
    out = []
    for s0 in range(0, nslots, group):
        ns = min(group, nslots - s0)
        out.append(next(NS for top, NS in rungs if ns <= top))
    return tuple(out)


def slot_problem(count, npairs, **kw):
    return Problem(SLOT_N, SLOT_T, count, all_pairs(SLOT_T)[:npairs], (2, 3), seed=500 + 7 * count + npairs,
                   symmetric=False, fenced=True, **kw)


@pytest.mark.parametrize("slots,count,npairs,ns", SLOT_SHAPES, ids=[f"s{s[0]}g{s[1]}p{s[2]}" for s in SLOT_SHAPES])
def test_every_instantiation_and_group_edge(slots, count, npairs, ns):
    assert slots == count * npairs and instantiations(slots) == ns
    check_fenced(slot_problem(count, npairs), f"{slots} slots = {count} x {npairs} pairs, NS {ns}:")


# ---- 3. the result does not depend on the grid --------------------------------------------------------------------------
@pytest.mark.parametrize("count,npairs", [(3, 45), (32, 2), (2, 32)], ids=["s135", "s64g32", "s64p32"])
def test_a_slot_does_not_depend_on_its_group(count, npairs):
    """A slot of a batched call (NS = 32 or 8, any place in its group) has the bits of the call on its geometry and its
    pair alone (count = 1, npairs = 1, NS = 1): the first slot, the last, and the slots on either side of every boundary
    between two groups."""
    pb = slot_problem(count, npairs)
    got, intact = pb.call()
    assert intact
    nslots = count * npairs
    slots = sorted({0, nslots - 1} | {s for b in range(32, nslots, 32) for s in (b - 1, b)})
    differ = []
    for s in slots:
        p, g = divmod(s, count)
        alone, intact = pb.single(g, p).call()
        assert intact
        for k in OUTPUTS:
            a, b = got[k][p, g], alone[k][0, 0]
            if not torch.equal(a, b):
                differ.append((s, k, float((a - b).abs().max())))
    print(f"{nslots} slots, slots {slots} alone against the batch:", differ or "equal bits")
    assert not differ, differ


# ---- 4. more than 32 pairs ----------------------------------------------------------------------------------------------
def check_by_kind(pb, what):
    """As check_fenced, the dipoles of the diagonal and of the transition slots apart: the nuclear term on a wrong slot
    (a wrong word or bit of the mask) is named."""
    got, intact = pb.call()
    assert intact, what
    ref = pb.reference()
    diag = pb.pairs[:, 0] == pb.pairs[:, 1]
    dev = np.abs(got["dipole"].cpu().numpy() - ref["dipole"]).max(axis=(1, 2))
    nuclear = np.linalg.norm(np.einsum("a,gax->gx", pb.charges, pb.coords - np.asarray(pb.origin)), axis=1).min()
    print(f"{what} dipole of {diag.sum()} diagonal slots {dev[diag].max():.2e}, of {(~diag).sum()} transition slots "
          f"{dev[~diag].max() if (~diag).any() else 0.0:.2e} (smallest nuclear term {nuclear:.2e})")
    assert nuclear > 1e-3        # (a misplaced nuclear term cannot hide)
    assert dev[diag].max() < BAR, (what, "diagonal slots", np.nonzero(diag & (dev >= BAR))[0])
    assert not (~diag).any() or dev[~diag].max() < BAR, (what, "transition slots", np.nonzero(~diag & (dev >= BAR))[0])
    return compare(got, ref, what)


@pytest.mark.parametrize("G", [1, 2])
def test_78_pairs_three_words_of_the_mask(G):
    pairs = all_pairs(12)
    words = {p >> 5 for p, (k, l) in enumerate(pairs) if k == l}
    assert len(pairs) == 78 and words == {0, 1, 2}
    check_by_kind(Problem(4, 12, G, pairs, (1, 3), seed=78 + G, symmetric=False, fenced=True), f"78 pairs, G={G}:")


def test_4095_pairs_of_one_geometry():
    pairs = all_pairs(90)
    assert len(pairs) == 4095 and max(p >> 5 for p, (k, l) in enumerate(pairs) if k == l) == 127
    check_by_kind(Problem(2, 90, 1, pairs, (1, 1), seed=4095, symmetric=False, fenced=True), "4095 pairs:")


def test_4096_slots_512_geometries():
    assert 512 * 8 == source_constant("kPropMaxSlots")
    check_by_kind(Problem(2, 4, 512, all_pairs(4)[:8], (1, 1), seed=4096, symmetric=False, fenced=True),
                  "512 geometries x 8 pairs:")


# ---- 5. the row chunks --------------------------------------------------------------------------------------------------
# T: (rows per chunk, chunks, rows of the last chunk) -- one chunk exactly; kPropMaxChunks chunks of the smallest size; a
# last chunk of ONE row; a last chunk whose last 64-row weight tile is cut at 57; the limit of T
CHUNKS = {16: (256, 1, 256), 128: (256, 64, 256), 129: (320, 53, 1), 181: (512, 64, 505), 512: (4096, 64, 4096)}


def chunking(T):
    """prop_rows_per_chunk and prop_chunks with the constants of the source."""
    rows_min, max_chunks, tile = (source_constant(k) for k in ("kPropRowsMin", "kPropMaxChunks", "kPropRowTile"))
    up = lambda a, b: (a + b - 1) // b
    rows = T * T
    per = max(rows_min, up(up(rows, max_chunks), tile) * tile)
    chunks = up(rows, per)
    return per, chunks, rows - (chunks - 1) * per


def chunks_of_the_library(T):
    """The chunks the library plans: its scratch is chunks x slots x N^2 doubles, 256 bytes per chunk at N = 4, 2 slots."""
    from evcont_amd import _lib
    nbytes = _lib.load().evc_properties_workspace_bytes(4, T, 1, 1, 2)
    assert nbytes > 0 and nbytes % 256 == 0
    return nbytes // 256


@pytest.mark.parametrize("T", sorted(CHUNKS))
def test_row_chunks_at_their_edges(T):
    assert chunking(T) == CHUNKS[T] and chunks_of_the_library(T) == CHUNKS[T][1]
    pb = Problem(3, T, 1, [(0, 0), (0, T - 1), (T - 1, T - 1)], (1, 2), seed=40 + T, symmetric=False, fenced=True)
    first, _ = check_fenced(pb, f"T={T}, chunks {CHUNKS[T]}:")
    second, intact = pb.call()
    assert intact and all(torch.equal(first[k], second[k]) for k in OUTPUTS)


# ---- 6. atoms -----------------------------------------------------------------------------------------------------------
ATOMS_N = 6


def many_atoms_slices(A=300, holders=(299, 0, 256, 7, 255, 298)):
    """AO mu belongs to atom holders[mu]; every other atom is empty, at varying places (start == stop in 0 .. N)."""
    sl = np.array([[a % (ATOMS_N + 1)] * 2 for a in range(A)], dtype=np.int64)
    for mu, at in enumerate(holders):
        sl[at] = (mu, mu + 1)
    return sl


# atoms out of order and overlapping, AO 2 in no atom, an empty atom, a slice that ends at N + 5
ODD_SLICES = np.array([[4, 6], [0, 2], [3, ATOMS_N + 5], [2, 2]], dtype=np.int64)


@pytest.mark.parametrize("name", ["300 atoms", "odd slices"])
def test_atom_loops_and_slices(name):
    sl = many_atoms_slices() if name == "300 atoms" else ODD_SLICES
    pb = Problem(ATOMS_N, 3, 2, DIAG3, None, seed=300 + len(sl), symmetric=False, aoslices=sl, fenced=True)
    ref = pb.reference()
    assert ref["mulliken"].shape == (3, 2, len(sl)) and pb.charges.shape == (len(sl),)
    if name == "300 atoms":
        held = np.abs(ref["mulliken"]).max(axis=(0, 1)) > 0
        assert len(sl) > 256 and held.sum() == ATOMS_N and held[[0, 255, 256, 299]].all()
    else:
        per_ao = np.einsum("ij,ji->i", ref["d_ao"][0, 0], pb.S[0])
        assert ref["mulliken"][0, 0, 2] == np.sum(per_ao[3:6]) and ref["mulliken"][0, 0, 3] == 0.0
    check_fenced(pb, f"{name}:")


# ---- 7. outputs one at a time beyond one tile ---------------------------------------------------------------------------
def test_every_output_may_be_null_at_n37():
    """tests/test_gpu_properties.py::test_every_output_may_be_null at N = 37 (TM = 4, three tile rows the last of 5), T = 17
    (two chunks), 33 slots (two groups): the early return after the Loewdin sums and the branches without d_ao."""
    pb = Problem(37, 17, 11, DIAG3, (1, 17, 19), seed=37, symmetric=False, fenced=True)
    full, _ = check_fenced(pb, "n=37 T=17, 33 slots:")
    for skip in OUTPUTS:
        part, intact = pb.call(tuple(k for k in OUTPUTS if k != skip))
        assert intact and skip not in part
        for k in part:
            assert torch.equal(part[k], full[k]), (skip, k)
    for only in OUTPUTS:
        one, intact = pb.call((only,))
        assert intact and torch.equal(one[only], full[only]), only


# ---- 8. evc_sgto_dipole_batch at its limits -----------------------------------------------------------------------------
SDIP_ORIGIN = (0.7, -1.3, 2.1)


def sdip_basis(nprim):
    from evcont_amd.hchain import STO3G_H_COEFFICIENTS, STO3G_H_EXPONENTS, STO6G_H_COEFFICIENTS, STO6G_H_EXPONENTS
    if nprim == 1:
        return (0.4,), (1.0,)
    if nprim == 3:
        return STO3G_H_EXPONENTS, STO3G_H_COEFFICIENTS
    if nprim == 6:
        return STO6G_H_EXPONENTS, STO6G_H_COEFFICIENTS
    assert nprim == 8
    ex = 0.1 * 400.0 ** (np.arange(8) / 7.0)                 # 0.1 ... 40
    co = np.array([0.10, 0.22, 0.30, 0.26, 0.18, 0.11, 0.06, 0.03])
    cn = co * (2.0 * ex / np.pi) ** 0.75
    norm = np.sum(cn[:, None] * cn[None, :] * (np.pi / (ex[:, None] + ex[None, :])) ** 1.5)
    return tuple(ex), tuple(co / np.sqrt(norm))               # <mu|mu> = 1


def sdip_cluster(natm, G, seed):
    """A 3-D cluster within 10 Bohr and G - 1 perturbed copies; in every geometry atoms 0, 1 share x and y but not z,
    atoms 2, 3 share y alone, atoms 4, 5 coincide."""
    rng = np.random.default_rng(seed)
    moved = (np.arange(G) > 0)[:, None, None]
    R = rng.uniform(-4.5, 4.5, (natm, 3))[None] + 0.05 * rng.standard_normal((G, natm, 3)) * moved
    R[:, 1, :2] = R[:, 0, :2]
    R[:, 3, 1] = R[:, 2, 1]
    R[:, 5] = R[:, 4]
    assert np.abs(R).max() < 5.0
    return np.ascontiguousarray(R)


def sdip_call(R, basis, origin=SDIP_ORIGIN):
    """evc_sgto_dipole_batch into a fenced buffer -> ((G,3,N,N) on the device, fences intact)."""
    from evcont_amd import _lib
    from sgto_harness import Fenced
    G, A = R.shape[:2]
    ex, co = (np.ascontiguousarray(b, dtype=np.float64) for b in basis)
    out = Fenced(G * 3 * A * A)
    dR = torch.from_numpy(np.ascontiguousarray(R)).to(DEV)
    o = (C.c_double * 3)(*origin)
    lib = _lib.load()
    rc = lib.evc_sgto_dipole_batch(A, len(ex), G, dR.data_ptr(), ex.ctypes.data, co.ctypes.data, C.cast(o, C.c_void_p),
                                   out.ptr, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.evc_last_error()
    torch.cuda.synchronize()
    return out.device((G, 3, A, A)), out.fences_intact()


def sdip_reference(R, basis, origin=SDIP_ORIGIN):
    """``dipole_integrals(origin)`` of the molecule ``s_gaussian_mol`` returns, at every geometry of R (the method reads
    coordinates and basis alone, so the molecule is built once, on one centre: 96 centres of 8 primitives have 768^4
    primitive repulsion integrals, and coincident nuclei no repulsion energy)."""
    from evcont_amd.hchain import s_gaussian_mol
    mol = s_gaussian_mol(np.zeros((1, 3)), None, basis[0], basis[1], need_grad=False)
    return np.stack([dataclasses.replace(mol, coords=r).dipole_integrals(origin) for r in R])


def sdip_vectorised(R, basis, origin=SDIP_ORIGIN):
    """The same formula for many geometries of few centres at once: (G,3,A,A)."""
    ex, co = (np.asarray(b, dtype=np.float64) for b in basis)
    cn = co * (2.0 * ex / np.pi) ** 0.75
    pp = ex[:, None] + ex[None, :]
    A_, B_ = R[:, :, None, None, None, :], R[:, None, :, None, None, :]         # (G,i,j,a,b,x)
    r2 = np.sum((A_ - B_) ** 2, axis=-1)
    sp = (np.pi / pp) ** 1.5 * np.exp(-(ex[:, None] * ex[None, :] / pp) * r2) * (cn[:, None] * cn[None, :])
    P = np.where(A_ == B_, A_, (ex[:, None, None] * A_ + ex[None, :, None] * B_) / pp[:, :, None])
    return np.moveaxis(np.sum((P - np.asarray(origin)) * sp[..., None], axis=(3, 4)), -1, 1)


# natm x nprim: exactly one block (N^2 = 256), a second block, the limit; every supported kind of contraction once
@pytest.mark.parametrize("natm,nprim", [(16, 1), (17, 3), (17, 6), (96, 8)])
def test_sgto_dipole_blocks_and_primitives(natm, nprim):
    basis, R = sdip_basis(nprim), sdip_cluster(natm, 2, seed=natm + nprim)
    got, intact = sdip_call(R, basis)
    again, intact2 = sdip_call(R, basis)
    assert intact and intact2
    a, want = got.cpu().numpy(), sdip_reference(R, basis)
    dev = np.abs(a - want)
    near = {"shared x, y": dev[:, :, 0, 1].max(), "shared y": dev[:, :, 2, 3].max(), "coincident": dev[:, :, 4, 5].max()}
    print(f"natm={natm} nprim={nprim}: max |d dip| = {dev.max():.2e}", {k: f"{v:.2e}" for k, v in near.items()})
    assert np.all(np.isfinite(a)) and dev.max() < BAR
    assert torch.equal(got, again) and np.array_equal(a, a.transpose(0, 1, 3, 2))


@pytest.mark.parametrize("natm", [1, 2])
def test_sgto_dipole_65535_geometries(natm):
    basis, G = sdip_basis(3), 65535
    R = np.random.default_rng(65535 + natm).uniform(-5.0, 5.0, (G, natm, 3))
    # (two float64 routes of one sum of 9 terms of size |R - O| < 8, a dozen roundings each)
    assert np.abs(sdip_vectorised(R[:3], basis) - sdip_reference(R[:3], basis)).max() < 1e-13
    got, intact = sdip_call(R, basis)
    assert intact
    a, want = got.cpu().numpy(), sdip_vectorised(R, basis)
    if natm == 1:        # (R_g - O) S_00
        S00 = sdip_vectorised(np.zeros((1, 1, 3)), basis, origin=(-1.0, 0.0, 0.0))[0, 0, 0, 0]
        assert np.abs(want[:, :, 0, 0] - (R[:, 0] - np.asarray(SDIP_ORIGIN)) * S00).max() < 1e-13
    print(f"natm={natm}, 65535 geometries: max |d dip| = {np.abs(a - want).max():.2e}")
    assert np.all(np.isfinite(a)) and np.abs(a - want).max() < BAR
    assert np.array_equal(a, a.transpose(0, 1, 3, 2))
    for g in (0, 1, G - 1):
        alone, intact = sdip_call(R[g: g + 1], basis)
        assert intact and torch.equal(alone[0], got[g]), g


# ---- 9. the chunked loop of get_multistate_properties -------------------------------------------------------------------
def test_get_multistate_properties_in_ragged_chunks(monkeypatch):
    """Five geometries under a BATCH_WORKSPACE_BUDGET of two and a half geometries: batches of 2, 2 and 1, the same
    numbers as the one batch of five, and per geometry those of a host evaluation; then with forces (the other
    per-geometry workspace formula)."""
    from evcont_amd import _lib
    from evcont_amd import ab_initio_gradients_loewdin as agl
    from evcont_amd.ab_initio_eigenvector_continuation import get_multistate_properties
    from evcont_amd.hchain import s_gaussian_mol
    from oracle import evcont_oracle as orc
    from test_gpu_properties import check_props, host_reference
    from test_properties_host import H4_CHARGES, H4_COORDS, h4_problem
    _, S_train, one, two = h4_problem()
    rng = np.random.default_rng(5)
    mols = [s_gaussian_mol(H4_COORDS + 0.05 * rng.standard_normal((4, 3)), H4_CHARGES) for _ in range(5)]
    origin, charges, lib = (0.1, 0.2, -0.3), np.asarray(H4_CHARGES), _lib.load()
    seen = []
    make = agl._batched_evaluator

    def spy(t, natm, count, *a, **kw):
        seen.append((t, natm, count))
        return make(t, natm, count, *a, **kw)

    monkeypatch.setattr(agl, "_batched_evaluator", spy)
    for forces in (False, True):
        del seen[:]
        E, whole = get_multistate_properties(mols, one, two, S_train, 2, DIAG3, origin, return_forces=forces)
        assert [s[2] for s in seen] == [5]
        t, natm = seen[0][:2]
        per_geo = (lib.evc_workspace_bytes_roots_batch(C.byref(t.cstruct), natm, 1, 1) * len(DIAG3) if forces else
                   lib.evc_workspace_bytes_batch(C.byref(t.cstruct), natm, 1))
        assert per_geo > 0
        del seen[:]
        with monkeypatch.context() as m:
            m.setattr(agl, "BATCH_WORKSPACE_BUDGET", 2 * per_geo + per_geo // 2)
            E2, parts = get_multistate_properties(mols, one, two, S_train, 2, DIAG3, origin, return_forces=forces)
        assert [s[2] for s in seen] == [2, 2, 1]
        assert set(parts) == set(whole) and E.shape == (5, 2) and whole["dipole"].shape == (5, 3, 3)
        gap = {"E": float(np.abs(E2 - E).max())}
        # (an eigenvector's sign is the solver's; the observables of a pair are compared below)
        gap.update({k: float(np.abs(parts[k] - whole[k]).max()) for k in whole if k != "C"})
        print(f"forces={forces}: chunks of 2, 2, 1 against one batch of 5:", gap)
        assert max(gap.values()) < BAR, gap
        # observed: a geometry's energies and observables do not depend on its batch, to the last bit (the forces do,
        # by 1e-16)
        assert all(gap[k] == 0.0 for k in ("E", "dipole", "mulliken_charges", "loewdin_charges")), gap
        # per geometry against the host, with the eigenvectors the call solved for
        for g, mol in enumerate(mols):
            b = orc.AOBundle(mol.S, mol.hcore, mol.eri, mol.ipovlp, mol.dhcore, mol.eri_ip1, mol.aoslices, mol.enuc,
                             mol.gnuc)
            E_host, _ = orc.approximate_multistate_OAO(b, one, two, S_train, 2)
            assert np.abs(E2[g] - E_host).max() < BAR, (g, E2[g], E_host)
        ref = host_reference(one, parts["C"], DIAG3, mols, np.stack([m.dipole_integrals(origin) for m in mols]), charges,
                             np.stack([m.coords for m in mols]), origin)
        check_props({k: parts[k] for k in ("dipole", "mulliken_charges", "loewdin_charges")}, ref, DIAG3, charges,
                    f"forces={forces}, chunked against the host:")
