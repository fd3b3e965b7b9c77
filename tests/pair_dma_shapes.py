"""The shape classes of the LDS-DMA pair-step kernels (csrc/pair_dma.hip: ptd_kernel<0>, ptd_kernel<0, 1>, y2d_kernel<1>) as
plain arithmetic on the orbital count N and the batch size G, and the (N, G) lists of tests/test_gpu_pair_dma_sweep.py.
No GPU import: tests/test_pair_dma_shapes.py holds the lists to the classes on the CPU.

The formulas restate the kernels' (they are not read from the source):
  npairs = N (N + 1) / 2 leading pairs, tiles of 8, the last one ragged;
  the write-out of a tile runs in passes of 64 rows, wave w writing whole groups of 16 rows: pass k <=> 64 k < npairs - 16 w;
  the counted waits leave the stores of the passes c = 1..3 (even phase, cntA) or c = 5..7 (odd phase, cntB) in flight;
  pairstep_tiles(G) tiles per workgroup for the kernels with one workgroup per CU, the last workgroup ragged.
"""
SIZES = list(range(17, 31))            # every orbital count the kernels take
SWEEP_COUNTS = [4, 8, 32]              # 2, 4 and 8 tiles per workgroup
SWEEP = [(n, G) for n in SIZES for G in SWEEP_COUNTS]
BOUNDARY_N = 20                        # the smallest orbital count with four passes
BOUNDARY = [(BOUNDARY_N, G) for G in (7, 31, 33)]   # the neighbours of the pairstep_tiles thresholds 8 and 32
KNOBS_OFF = [(n, 4) for n in SIZES]    # the unfused route (both knobs 0), one child process
KEEP_SIZES = [20, 25, 28]              # the unpacked 2-RDM requested, G = 4
ROOTS_SIZES = [22, 25]                 # the multi-slot roots call


def npairs(n):
    return n * (n + 1) // 2


def ntiles(n):
    return (npairs(n) + 7) // 8


def live_in_last_tile(n):
    return npairs(n) - 8 * (ntiles(n) - 1)


def passes_per_wave(n):
    return tuple(sum(64 * k < npairs(n) - 16 * w for k in range(8)) for w in range(4))


def cnt_a_per_wave(n):
    return tuple(sum(64 * c < npairs(n) - 16 * w for c in (1, 2, 3)) for w in range(4))


def cnt_b_per_wave(n):
    return tuple(sum(64 * c < npairs(n) - 16 * w for c in (5, 6, 7)) for w in range(4))


def pairstep_tiles(count):
    return 8 if count >= 32 else 4 if count >= 8 else 2


def workgroups(n, tiles_per_wg):
    return (ntiles(n) + tiles_per_wg - 1) // tiles_per_wg


def tiles_in_last_workgroup(n, tiles_per_wg):
    return ntiles(n) - tiles_per_wg * (workgroups(n, tiles_per_wg) - 1)


def shape_class(n):
    """What tells the orbital counts apart inside the kernels."""
    return passes_per_wave(n), cnt_b_per_wave(n), live_in_last_tile(n), npairs(n) % 2


def table_row(n):
    """One row of the table of DESIGN.md 4.4."""
    return (n, npairs(n), npairs(n) % 2, ntiles(n), live_in_last_tile(n), passes_per_wave(n), cnt_a_per_wave(n),
            cnt_b_per_wave(n), tuple(tiles_in_last_workgroup(n, t) for t in (2, 4, 8)))
