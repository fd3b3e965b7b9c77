"""What tests/test_gpu_properties_limits.py rests on and needs no device: its tables against the dispatch ladder and the
constants of csrc/properties.hip, the chunk arithmetic against the library's own workspace size, that its inputs can tell
a transposed index from the truth, and its vectorised dipole formula against HChainMol.dipole_integrals."""
import numpy as np
import pytest

import test_gpu_properties_limits as lim
from properties_harness import source_constant


def test_the_slot_table_names_the_instantiations_the_ladder_picks():
    rungs, group = lim.ladder()
    assert group == 32 and [ns for _, ns in rungs] == [1, 2, 4, 8, 16, 32] and all(top <= ns for top, ns in rungs)
    for slots, count, npairs, ns in lim.SLOT_SHAPES:
        assert slots == count * npairs and npairs <= len(lim.all_pairs(lim.SLOT_T))
        assert lim.instantiations(slots) == ns, (slots, lim.instantiations(slots))
    totals = {s[0] for s in lim.SLOT_SHAPES}
    assert {3, 4, 5, 9, 16, 17, 31, 32, 64, 45, 135} <= totals
    # every instantiation but <1> (the single calls of the grouping test), a full group, one with an absent slot
    assert {ns for s in lim.SLOT_SHAPES for ns in s[3]} == {2, 4, 8, 16, 32}
    assert any(32 % count for _, count, _, _ in lim.SLOT_SHAPES)


@pytest.mark.parametrize("T", sorted(lim.CHUNKS))
def test_chunk_arithmetic(T):
    per, chunks, last = lim.chunking(T)
    assert (per, chunks, last) == lim.CHUNKS[T]
    assert chunks <= source_constant("kPropMaxChunks") and per % source_constant("kPropRowTile") == 0
    assert (chunks - 1) * per < T * T <= chunks * per and 1 <= last <= per
    assert lim.chunks_of_the_library(T) == chunks


def test_chunk_edges_are_the_ones_named():
    assert lim.CHUNKS[16][1] == 1 and lim.chunking(17)[1] == 2
    assert lim.CHUNKS[128][:2] == (source_constant("kPropRowsMin"), source_constant("kPropMaxChunks"))
    assert lim.CHUNKS[129][2] == 1
    assert lim.CHUNKS[181][2] % source_constant("kPropRowTile") == 57
    from evcont_amd import _lib
    assert max(lim.CHUNKS) == 512 and _lib.load().evc_properties_workspace_bytes(4, 513, 1, 1, 2) == 0      # the limit of T


@pytest.mark.parametrize("shape", lim.NONSYM_SHAPES, ids=[f"n{s[0]}" for s in lim.NONSYM_SHAPES])
def test_the_inputs_can_tell_a_transpose(shape):
    pb = lim.nonsym_problem(shape, upload=False)
    tells = lim.can_tell_a_transpose(pb, pb.reference())
    assert min(tells) > lim.TELLS, tells
    assert shape[0] % 16 != 0 or shape[0] == 96


def test_the_pair_lists_reach_the_words_they_are_meant_to():
    diag_words = lambda pairs: {p >> 5 for p, (k, l) in enumerate(pairs) if k == l}
    assert diag_words(lim.all_pairs(12)) == {0, 1, 2} and len(lim.all_pairs(12)) == 78
    assert len(lim.all_pairs(90)) == 4095
    assert max(diag_words(lim.all_pairs(90))) == source_constant("kPropMaxSlots") // 32 - 1


def test_atom_tables():
    sl = lim.many_atoms_slices()
    assert sl.shape == (300, 2) and np.all(sl[:, 0] <= sl[:, 1]) and sl.max() <= lim.ATOMS_N
    held = np.nonzero(sl[:, 1] - sl[:, 0])[0]
    assert sorted(sl[held, 0]) == list(range(lim.ATOMS_N)) and {0, 255, 256, 299} <= set(held)
    odd = lim.ODD_SLICES
    covered = {mu for a, b in odd for mu in range(a, min(b, lim.ATOMS_N))}
    assert 2 not in covered and odd[:, 1].max() == lim.ATOMS_N + 5 and odd[0, 0] > odd[1, 0]


def test_sdip_inputs_and_the_vectorised_formula():
    for nprim in (1, 3, 6, 8):
        ex, co = lim.sdip_basis(nprim)
        assert len(ex) == len(co) == nprim and min(ex) > 0 and min(co) > 0
        S00 = lim.sdip_vectorised(np.zeros((1, 1, 3)), (ex, co), origin=(-1.0, 0.0, 0.0))[0, 0, 0, 0]
        assert nprim == 1 or abs(S00 - 1.0) < 1e-5, (nprim, S00)      # (tabulated contractions: normalised to their digits)
    ex, _ = lim.sdip_basis(8)
    assert abs(min(ex) - 0.1) < 1e-12 and abs(max(ex) - 40.0) < 1e-9
    R = lim.sdip_cluster(17, 2, seed=1)
    assert np.all(R[:, 0, :2] == R[:, 1, :2]) and np.all(R[:, 0, 2] != R[:, 1, 2])
    assert np.all(R[:, 2, 1] == R[:, 3, 1]) and np.all(R[:, 2, [0, 2]] != R[:, 3, [0, 2]]) and np.all(R[:, 4] == R[:, 5])
    for basis in (lim.sdip_basis(3), lim.sdip_basis(8)):
        a, b = lim.sdip_vectorised(R[:, :6], basis), lim.sdip_reference(R[:, :6], basis)
        assert a.shape == b.shape == (2, 3, 6, 6) and np.abs(a - b).max() < 1e-13, np.abs(a - b).max()
