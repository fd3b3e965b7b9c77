"""What the device full-CI entry points (evcont_amd/csrc/fci.hip) launch for every orbital count, written down from
include/evcont_hip.h and the dispatch rules of fci_trdm_config / fci_rt -- data, not a call of the library.

tests/test_gpu_fci_shapes.py holds the ``evc_profile_kernel`` records of every case to these rows;
tests/test_dispatch_closure.py holds the ``launch_trdm`` and sigma switches of fci.hip to them, so that an instantiation
without a tested orbital count fails ``pytest -m "not gpu"``.
"""

# norb: npad = norb^2 rounded up to 16, nt = npad / 16 tiles per edge;
#       trdm = (RT, NBW) of fci_trdm_kernel and the number of quadrants (blockIdx.y); sigma = RT of fci_sigma_gemm_kernel
#       and the row groups nbw a determinant tile is shared by.
TILINGS = {
    1: dict(npad=16, trdm=(1, 1), quadrants=1, sigma=1, sigma_nbw=1),
    2: dict(npad=16, trdm=(1, 1), quadrants=1, sigma=1, sigma_nbw=1),
    3: dict(npad=16, trdm=(1, 1), quadrants=1, sigma=1, sigma_nbw=1),
    4: dict(npad=16, trdm=(1, 1), quadrants=1, sigma=1, sigma_nbw=1),
    5: dict(npad=32, trdm=(2, 1), quadrants=1, sigma=2, sigma_nbw=1),
    6: dict(npad=48, trdm=(3, 1), quadrants=1, sigma=3, sigma_nbw=1),
    7: dict(npad=64, trdm=(4, 1), quadrants=1, sigma=4, sigma_nbw=1),
    8: dict(npad=64, trdm=(4, 1), quadrants=1, sigma=4, sigma_nbw=1),
    9: dict(npad=96, trdm=(3, 2), quadrants=1, sigma=3, sigma_nbw=2),
    10: dict(npad=112, trdm=(4, 2), quadrants=1, sigma=4, sigma_nbw=2),
    11: dict(npad=128, trdm=(4, 2), quadrants=1, sigma=4, sigma_nbw=2),
    12: dict(npad=144, trdm=(3, 3), quadrants=1, sigma=3, sigma_nbw=3),
    13: dict(npad=176, trdm=(3, 2), quadrants=4, sigma=4, sigma_nbw=3),
    14: dict(npad=208, trdm=(4, 2), quadrants=4, sigma=4, sigma_nbw=4),
    15: dict(npad=240, trdm=(4, 2), quadrants=4, sigma=4, sigma_nbw=4),
    16: dict(npad=256, trdm=(4, 2), quadrants=4, sigma=4, sigma_nbw=4),
}

# (norb, nelec) run by tests/test_gpu_fci_shapes.py::test_every_orbital_count; nelec an int or (n_alpha, n_beta)
SHAPE_CASES = [
    (1, (1, 0)), (2, (1, 1)), (3, (0, 2)), (4, (2, 2)),
    (5, (3, 2)), (5, 5),
    (6, (2, 3)), (7, (3, 4)), (7, (7, 7)), (8, (4, 4)),
    (9, (2, 2)), (9, (4, 4)), (10, (2, 3)), (11, (2, 2)), (12, (2, 2)),
    (13, (2, 2)), (13, (3, 2)), (14, (2, 1)), (15, (2, 2)),
    (16, (1, 0)), (16, (1, 1)), (16, (2, 2)), (16, (3, 1)), (16, (16, 16)),
]

# layout code of evc_fci_excite -> the kernel its record names
EXCITE_KERNELS = {0: "fci_excite_det_kernel<0>", 1: "fci_excite_det_kernel<1>", 2: "fci_excite_orb_kernel"}

KMIN_ROWS = 256        # determinants per split-K block, at least
KMAX_BLOCKS = 256      # split-K blocks, at most


def rows_per_block(dim):
    """R of include/evcont_hip.h: max(256, ceil(dim / 256) rounded up to 64)."""
    r = -(-dim // KMAX_BLOCKS)
    return max(KMIN_ROWS, -(-r // 64) * 64)


def trdm_record(norb, dim):
    """The start of the fci_trdm record: everything but the workspace regime."""
    t = TILINGS[norb]
    blocks = -(-dim // rows_per_block(dim))
    return f"fci_trdm_kernel<{t['trdm'][0]},{t['trdm'][1]}> quadrants={t['quadrants']} blocks={blocks} "


def sigma_record(norb):
    return f"fci_sigma_gemm_kernel<{TILINGS[norb]['sigma']}> chunk="


def trdm_instantiations():
    return {t["trdm"] for n, t in TILINGS.items() if any(c[0] == n for c in SHAPE_CASES)}


def sigma_instantiations():
    return {t["sigma"] for n, t in TILINGS.items() if any(c[0] == n for c in SHAPE_CASES)}
