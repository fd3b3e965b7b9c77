"""String tables of the device full-CI kernels (``csrc/fci.hip``): for every orbital pair ``(p, q)`` and every occupation
string ``I`` the one string ``J`` with ``<I| a_p^+ a_q |J> != 0`` and its sign -- the content of the CSR matrices of
``fci_small._excitation_ops`` (row ``I``, column ``J``), in the same string order (by integer value).  Host numpy,
built once per ``(norb, nocc)``."""
from __future__ import annotations

from functools import lru_cache
from typing import Tuple

import numpy as np

from .fci_small import _strings

MAX_ORB = 16


def npad_of(norb: int) -> int:
    """``norb**2`` rounded up to the 16 columns of an MFMA tile: the row pitch of the packed tables."""
    return (norb * norb + 15) // 16 * 16


@lru_cache(maxsize=32)
def excitation_table(norb: int, nocc: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(index, sign)``, both ``(norb**2, n_strings)``: ``index[p*norb+q, I] = J`` (int32, -1 where ``a_p^+ a_q``
    reaches ``I`` from no string) and ``sign[p*norb+q, I]`` = +1 / -1 (int8, 0 where there is none)."""
    if not (1 <= norb <= MAX_ORB and 0 <= nocc <= norb):
        raise ValueError(f"excitation_table: norb={norb}, nocc={nocc} (1 <= norb <= {MAX_ORB}, 0 <= nocc <= norb)")
    strs = np.asarray(_strings(norb, nocc), dtype=np.int64)
    ns = strs.size
    lookup = np.full(1 << norb, -1, dtype=np.int32)
    lookup[strs] = np.arange(ns, dtype=np.int32)
    index = np.full((norb * norb, ns), -1, dtype=np.int32)
    sign = np.zeros((norb * norb, ns), dtype=np.int8)
    popcount = np.array([bin(x).count("1") for x in range(1 << norb)], dtype=np.int8)
    cols = np.arange(ns, dtype=np.int32)
    for p in range(norb):
        for q in range(norb):
            occ_q = ((strs >> q) & 1).astype(bool)
            if p == q:
                index[p * norb + q, occ_q] = cols[occ_q]
                sign[p * norb + q, occ_q] = 1
                continue
            ok = occ_q & ~((strs >> p) & 1).astype(bool)
            src = strs[ok]
            dst = (src ^ (1 << q)) | (1 << p)
            lo, hi = (p, q) if p < q else (q, p)
            between = popcount[src & (((1 << hi) - 1) ^ ((1 << (lo + 1)) - 1))]
            rows = lookup[dst]
            index[p * norb + q, rows] = cols[ok]
            sign[p * norb + q, rows] = np.where(between & 1, -1, 1)
    index.setflags(write=False)
    sign.setflags(write=False)
    return index, sign


def packed_table(norb: int, nocc: int) -> np.ndarray:
    """The device form, ``(n_strings, npad)`` int32: entry ``[I, p*norb+q] = sign * (J + 1)``, 0 where there is no
    ``J`` and in the pad columns."""
    index, sign = excitation_table(norb, nocc)
    out = np.zeros((index.shape[1], npad_of(norb)), dtype=np.int32)
    out[:, :norb * norb] = (sign.astype(np.int32) * (index + 1)).T
    return out


def excite_through_tables(c, norb: int, nelec: Tuple[int, int]) -> np.ndarray:
    """What the device excite kernel computes, in numpy: ``D[p*norb+q] = E_pq c`` gathered through the packed tables,
    ``(norb**2, na, nb)``; equal to ``SmallFCI._excite_all`` bit for bit."""
    ta, tb = packed_table(norb, int(nelec[0])), packed_table(norb, int(nelec[1]))
    na, nb = ta.shape[0], tb.shape[0]
    c = np.asarray(c, dtype=np.float64).reshape(na, nb)
    D = np.empty((norb * norb, na, nb))
    for pq in range(norb * norb):
        a, b = ta[:, pq], tb[:, pq]
        va = np.where((a != 0)[:, None], np.sign(a)[:, None] * c[np.abs(a) - 1, :], 0.0)
        vb = np.where((b != 0)[None, :], np.sign(b)[None, :] * c[:, np.abs(b) - 1], 0.0)
        D[pq] = va + vb
    return D


def spin_square_through_tables(c, norb: int, nelec: Tuple[int, int], alpha: float = 1.0, ss: float = 0.0,
                               beta: float = 0.0, out=None) -> np.ndarray:
    """What ``evc_fci_spin_apply`` computes, in numpy and in the kernel's order: ``beta out + alpha (S^2 c - ss c)``,
    ``(na, nb)``.  Per element: ``(k - ss) c`` with ``k = Sz (Sz + 1) + n_beta``, then, ``pq = p norb + q`` ascending,
    ``- sgn_a sgn_b c[Ja, Jb]`` with ``Ja`` from ``tab_a[Ia][p norb + q]`` and ``Jb`` from ``tab_b[Ib][q norb + p]`` where
    both entries are non-zero, then ``alpha`` times that sum, then ``+ beta out`` (``beta == 0`` does not read ``out``);
    every step rounded on its own.  The bit-level reference of the device kernel."""
    n_a, n_b = int(nelec[0]), int(nelec[1])
    ta, tb = packed_table(norb, n_a), packed_table(norb, n_b)
    na, nb = ta.shape[0], tb.shape[0]
    c = np.asarray(c, dtype=np.float64).reshape(na, nb)
    sz = 0.5 * (n_a - n_b)
    t = ((sz * (sz + 1.0) + n_b) - ss) * c
    for p in range(norb):
        for q in range(norb):
            a, b = ta[:, p * norb + q], tb[:, q * norb + p]
            ra, rb = np.flatnonzero(a), np.flatnonzero(b)
            if ra.size == 0 or rb.size == 0:
                continue
            sgn = (np.sign(a[ra])[:, None] * np.sign(b[rb])[None, :]).astype(np.float64)
            t[np.ix_(ra, rb)] -= sgn * c[np.ix_(np.abs(a[ra]) - 1, np.abs(b[rb]) - 1)]
    r = alpha * t
    if beta != 0.0:
        r = beta * np.asarray(out, dtype=np.float64).reshape(na, nb) + r
    return r
