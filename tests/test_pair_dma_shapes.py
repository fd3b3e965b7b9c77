"""CPU checks of the shape classes behind tests/test_gpu_pair_dma_sweep.py (tests/pair_dma_shapes.py): the table of
DESIGN.md 4.4 restated from N, every orbital count a class of its own, and the sweep reaching every ragged last
workgroup.  Someone who trims the sweep sees here which class they drop.  No kernel source and no assembly is read."""
import pair_dma_shapes as sh

#  N: npairs, odd, tiles, live in the last tile, passes / cntA / cntB per wave (0..3), tiles in the last workgroup at 2 / 4 / 8
TABLE = {
    17: (153, 1, 20, 1, (3, 3, 2, 2), (2, 2, 1, 1), (0, 0, 0, 0), (2, 4, 4)),
    18: (171, 1, 22, 3, (3, 3, 3, 2), (2, 2, 2, 1), (0, 0, 0, 0), (2, 2, 6)),
    19: (190, 0, 24, 6, (3, 3, 3, 3), (2, 2, 2, 2), (0, 0, 0, 0), (2, 4, 8)),
    20: (210, 0, 27, 2, (4, 4, 3, 3), (3, 3, 2, 2), (0, 0, 0, 0), (1, 3, 3)),
    21: (231, 1, 29, 7, (4, 4, 4, 3), (3, 3, 3, 2), (0, 0, 0, 0), (1, 1, 5)),
    22: (253, 1, 32, 5, (4, 4, 4, 4), (3, 3, 3, 3), (0, 0, 0, 0), (2, 4, 8)),
    23: (276, 0, 35, 4, (5, 5, 4, 4), (3, 3, 3, 3), (0, 0, 0, 0), (1, 3, 3)),
    24: (300, 0, 38, 4, (5, 5, 5, 4), (3, 3, 3, 3), (0, 0, 0, 0), (2, 2, 6)),
    25: (325, 1, 41, 5, (6, 5, 5, 5), (3, 3, 3, 3), (1, 0, 0, 0), (1, 1, 1)),
    26: (351, 1, 44, 7, (6, 6, 5, 5), (3, 3, 3, 3), (1, 1, 0, 0), (2, 4, 4)),
    27: (378, 0, 48, 2, (6, 6, 6, 6), (3, 3, 3, 3), (1, 1, 1, 1), (2, 4, 8)),
    28: (406, 0, 51, 6, (7, 7, 6, 6), (3, 3, 3, 3), (2, 2, 1, 1), (1, 3, 3)),
    29: (435, 1, 55, 3, (7, 7, 7, 7), (3, 3, 3, 3), (2, 2, 2, 2), (1, 3, 7)),
    30: (465, 1, 59, 1, (8, 8, 7, 7), (3, 3, 3, 3), (3, 3, 2, 2), (1, 3, 3)),
}


def test_table_restated_from_n():
    assert sorted(TABLE) == sh.SIZES == list(range(17, 31))
    for n in sh.SIZES:
        assert sh.table_row(n) == (n,) + TABLE[n], n
        # a wave's waits count what it stores: cntA and cntB are the passes 1..3 and 5..7 among its passes
        for w in range(4):
            p = sh.passes_per_wave(n)[w]
            assert sh.cnt_a_per_wave(n)[w] == min(max(p - 1, 0), 3) and sh.cnt_b_per_wave(n)[w] == min(max(p - 5, 0), 3)


def test_pairstep_tiles_thresholds():
    assert [sh.pairstep_tiles(G) for G in (4, 7, 8, 31, 32, 33)] == [2, 2, 4, 4, 8, 8]
    assert sorted({sh.pairstep_tiles(G) for _, G in sh.SWEEP}) == [2, 4, 8]
    assert [sh.pairstep_tiles(G) for _, G in sh.BOUNDARY] == [2, 4, 8]
    assert sh.passes_per_wave(sh.BOUNDARY_N)[0] == 4 and all(max(sh.passes_per_wave(n)) < 4 for n in range(17, sh.BOUNDARY_N))


def test_every_orbital_count_is_its_own_class():
    classes = {n: sh.shape_class(n) for n in sh.SIZES}
    assert len(set(classes.values())) == len(sh.SIZES), classes
    # ... and the pass counts the suite had never run are among them: four and six passes, wave 0 alone in the sixth
    assert {max(sh.passes_per_wave(n)) for n in sh.SIZES} == {3, 4, 5, 6, 7, 8}
    assert [n for n in sh.SIZES if sh.passes_per_wave(n) == (6, 5, 5, 5)] == [25]


def test_sweep_covers_every_size_on_both_routes():
    for G in sh.SWEEP_COUNTS:
        assert sorted(n for n, g in sh.SWEEP if g == G) == sh.SIZES, G
    assert sorted(n for n, _ in sh.KNOBS_OFF) == sh.SIZES
    # the fused kernels need at least 4 slots; the neighbouring tests' shapes stay covered
    assert all(G >= 4 for _, G in sh.SWEEP + sh.BOUNDARY + sh.KNOBS_OFF)
    assert set(sh.KEEP_SIZES) <= set(sh.SIZES) and set(sh.ROOTS_SIZES) <= set(sh.SIZES)


def test_sweep_reaches_every_ragged_last_workgroup():
    for tiles in (2, 4, 8):
        possible = {sh.tiles_in_last_workgroup(n, tiles) for n in sh.SIZES}
        reached = {sh.tiles_in_last_workgroup(n, tiles) for n, G in sh.SWEEP + sh.BOUNDARY if sh.pairstep_tiles(G) == tiles}
        assert reached == possible, (tiles, sorted(possible - reached))
    assert {sh.tiles_in_last_workgroup(n, 8) for n in sh.SIZES} == {1, 3, 4, 5, 6, 7, 8}
    # slab counts (= workgroups, what the gradient tail sums): 3 .. 30
    slabs = {sh.workgroups(n, sh.pairstep_tiles(G)) for n, G in sh.SWEEP}
    assert min(slabs) == 3 and max(slabs) == 30, sorted(slabs)
