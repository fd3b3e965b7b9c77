"""GPU tests of the full-CI C entry points (include/evcont_hip.h: evc_fci_trdm_rows, evc_fci_sigma, evc_fci_excite),
called directly, with every buffer they are handed poisoned and fenced:

* the workspace is ``ws_bytes`` of 0xFF (NaN as doubles: reading workspace that nothing wrote shows in the result)
  followed by 4096 bytes of 0xA5 that must be untouched afterwards; the outputs sit between two such fences;
* the workspace size is swept from the least to the resident one; every size must give the bits of the resident result,
  and on integer inputs (tests/test_gpu_fci_shapes.py) the bits of the host; the regime of every run is read from the
  profile record, and the sweep has to reach all four t-RDM regimes and all three sigma regimes;
* evc_fci_excite is compared bit for bit with fci_tables.excite_through_tables in its three layouts (D is a two-term
  sum, so this holds for any real input), NaN sentinels marking what it must leave alone.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

from evcont_amd.fci_small import SmallFCI
from evcont_amd.fci_tables import excite_through_tables, npad_of, packed_table
from fci_dispatch_table import EXCITE_KERNELS, sigma_record, trdm_record
from test_gpu_fci_device import check_identities, oao_integrals, random_vectors, sigma_bound, trdm_bound
from test_gpu_fci_shapes import integer_integrals, integer_vectors, integral

pytestmark = pytest.mark.gpu

_HOST = SmallFCI()
FENCE = 4096
SWEEP_CASES = [(9, (4, 4)), (13, (3, 2)), (16, (2, 2))]
FRACTIONS = (0.01, 0.03, 0.1, 0.2, 0.35, 0.5, 0.65, 0.8, 0.95)


def library():
    from evcont_amd import _lib
    from evcont_amd._lib import check
    return _lib, _lib.load(), check


class Fenced:
    """``nbytes`` of 0xFF between two fences of 0xA5, on the device."""

    def __init__(self, nbytes, dev, front=True):
        self.off = FENCE if front else 0
        self.nbytes = nbytes
        self.buf = torch.full((self.off + nbytes + FENCE,), 0xA5, dtype=torch.uint8, device=dev)
        self.buf[self.off:self.off + nbytes] = 0xFF

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def fences_intact(self):
        front = self.buf[:self.off]
        back = self.buf[self.off + self.nbytes:]
        return bool((front == 0xA5).all().item()) and bool((back == 0xA5).all().item()) and back.numel() == FENCE

    def doubles(self):
        assert self.nbytes % 8 == 0
        return self.buf[self.off:self.off + self.nbytes].cpu().numpy().view(np.float64).copy()


class Problem:
    def __init__(self, norb, nelec):
        self.lib_mod, self.lib, self.check = library()
        self.dev = torch.device("cuda:0")
        self.norb, self.nelec = norb, nelec
        ta, tb = packed_table(norb, nelec[0]), packed_table(norb, nelec[1])
        self.na, self.nb = ta.shape[0], tb.shape[0]
        self.dim = self.na * self.nb
        self.npad = npad_of(norb)
        self.ta, self.tb = torch.from_numpy(ta).to(self.dev), torch.from_numpy(tb).to(self.dev)
        self.least = self.lib.evc_fci_workspace_bytes(norb, self.na, self.nb, 1)
        self.full = self.lib.evc_fci_workspace_bytes(norb, self.na, self.nb, 0)
        assert 0 < self.least <= self.full

    def up(self, x):
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).reshape(-1)).to(self.dev)

    def record(self, stage):
        return self.lib.evc_profile_kernel(self.lib_mod.FCI_PROF_STAGES[stage]).decode()

    def trdm_rows(self, bra, kets, ws_bytes):
        n2, K = self.norb ** 2, len(kets)
        dbra, dkets = self.up(bra), [self.up(k) for k in kets]
        ws = Fenced(ws_bytes, self.dev, front=False)
        ov, d1, d2 = Fenced(8 * K, self.dev), Fenced(8 * K * n2, self.dev), Fenced(8 * K * n2 * n2, self.dev)
        ptrs = (C.c_void_p * K)(*[t.data_ptr() for t in dkets])
        self.check(self.lib.evc_fci_trdm_rows(self.norb, self.na, self.nb, self.ta.data_ptr(), self.tb.data_ptr(),
                                              dbra.data_ptr(), ptrs, K, ov.ptr, d1.ptr, d2.ptr, ws.ptr, ws_bytes, None),
                   "evc_fci_trdm_rows")
        torch.cuda.synchronize()
        for f in (ws, ov, d1, d2):
            assert f.fences_intact(), ws_bytes
        return (ov.doubles(), d1.doubles().reshape(K, self.norb, self.norb),
                d2.doubles().reshape((K,) + (self.norb,) * 4), self.record("fci_trdm"))

    def sigma(self, h1, h2, c, ws_bytes):
        dh1, dh2, dc = self.up(h1), self.up(h2), self.up(c)
        ws = Fenced(ws_bytes, self.dev, front=False)
        out = Fenced(8 * self.dim, self.dev)
        self.check(self.lib.evc_fci_sigma(self.norb, self.na, self.nb, self.ta.data_ptr(), self.tb.data_ptr(),
                                          dh1.data_ptr(), dh2.data_ptr(), dc.data_ptr(), out.ptr, ws.ptr, ws_bytes, None),
                   "evc_fci_sigma")
        torch.cuda.synchronize()
        assert ws.fences_intact() and out.fences_intact(), ws_bytes
        return out.doubles().reshape(self.na, self.nb), self.record("fci_sigma")


def trdm_regime(rec, norb, dim):
    head = trdm_record(norb, dim)
    m = re.fullmatch(re.escape(head) + r"bra_resident=([01]) ket_blocks=(\d+)", rec)
    assert m, rec
    blocks, resident, cb = int(head.split("blocks=")[1]), int(m.group(1)), int(m.group(2))
    assert 1 <= cb <= blocks
    if not resident:
        return "bra_resident=0 ket_blocks=1" if cb == 1 else "bra_resident=0 ket_blocks>1"
    return "bra_resident=1 ket_blocks=blocks" if cb == blocks else "bra_resident=1 ket_blocks<blocks"


def sigma_regime(rec, norb, dim):
    m = re.fullmatch(re.escape(sigma_record(norb)) + r"(\d+) \+ fci_sigma_gather_kernel", rec)
    assert m, rec
    chunk, ldg = int(m.group(1)), (dim + 63) // 64 * 64
    assert 64 <= chunk <= ldg and chunk % 64 == 0
    if chunk == ldg:
        return "chunk=ldg"
    if chunk == 64:
        return "chunk=64"
    return "64<chunk<ldg, short last chunk" if ldg % chunk else "64<chunk<ldg, no short chunk"


@functools.lru_cache(maxsize=None)
def sweep(norb, nelec):
    """Runs the case at every workspace size and checks every result; returns the regimes it went through."""
    p = Problem(norb, nelec)
    sizes = sorted({p.least, p.least + 1, p.full - 1, p.full} |
                   {p.least + int(f * (p.full - p.least)) for f in FRACTIONS})
    assert len(sizes) >= 8 or p.least == p.full
    K = 2
    ivec = integer_vectors(norb, nelec, K + 1, seed=300 + norb)
    ih1, ih2 = integer_integrals(norb, seed=400 + norb)
    host_i = [_HOST.trans_rdm12(ivec[0], k, norb, nelec) for k in ivec[1:]]
    host_s = _HOST.contract(ih1, ih2, ivec[0], norb, nelec)
    assert all(integral(a) and integral(b) for a, b in host_i) and integral(host_s)
    rvec = random_vectors(norb, nelec, K + 1, seed=500 + norb)
    rh1, rh2 = oao_integrals(norb)
    # the resident results of the random data: against the host within the derived bounds, then the reference bits
    rov, r1, r2, rec = p.trdm_rows(rvec[0], rvec[1:], p.full)
    assert trdm_regime(rec, norb, p.dim) == "bra_resident=1 ket_blocks=blocks"
    for i, ket in enumerate(rvec[1:]):
        h1_, h2_ = _HOST.trans_rdm12(rvec[0], ket, norb, nelec)
        tol = 2.0 * trdm_bound(rvec[0], ket, norb, nelec)
        assert np.abs(r1[i] - h1_).max() <= tol and np.abs(r2[i] - h2_).max() <= tol
        assert abs(rov[i] - np.dot(rvec[0].ravel(), ket.ravel())) <= tol
        check_identities(rov[i], r1[i], r2[i], nelec, tol)
    rsig, rec = p.sigma(rh1, rh2, rvec[0], p.full)
    assert sigma_regime(rec, norb, p.dim) == "chunk=ldg"
    assert (np.abs(rsig - _HOST.contract(rh1, rh2, rvec[0], norb, nelec)) <=
            2.0 * sigma_bound(rh1, rh2, rvec[0], norb, nelec)).all()
    trdm_seen, sigma_seen = set(), set()
    for ws_bytes in sizes:
        ov, d1, d2, rec = p.trdm_rows(ivec[0], ivec[1:], ws_bytes)
        regime = trdm_regime(rec, norb, p.dim)
        trdm_seen.add(regime)
        for i, ket in enumerate(ivec[1:]):
            assert ov[i] == float(np.dot(ivec[0].ravel(), ket.ravel())), (ws_bytes, regime)
            assert np.array_equal(d1[i], host_i[i][0]) and np.array_equal(d2[i], host_i[i][1]), (ws_bytes, regime)
        ov, d1, d2, rec2 = p.trdm_rows(rvec[0], rvec[1:], ws_bytes)
        assert rec2 == rec
        assert np.array_equal(ov, rov) and np.array_equal(d1, r1) and np.array_equal(d2, r2), (ws_bytes, regime)
        sig, rec = p.sigma(ih1, ih2, ivec[0], ws_bytes)
        sregime = sigma_regime(rec, norb, p.dim)
        sigma_seen.add(sregime)
        assert np.array_equal(sig, host_s), (ws_bytes, sregime)
        sig, rec2 = p.sigma(rh1, rh2, rvec[0], ws_bytes)
        assert rec2 == rec and np.array_equal(sig, rsig), (ws_bytes, sregime)
        print(f"workspace norb={norb} nelec={nelec} {ws_bytes} bytes "
              f"({(ws_bytes - p.least) / max(p.full - p.least, 1):.3f} of the way): {regime}; {sregime}")
    return frozenset(trdm_seen), frozenset(sigma_seen)


@pytest.mark.parametrize("norb,nelec", SWEEP_CASES)
def test_every_workspace_size_gives_the_resident_and_the_host_bits(norb, nelec):
    trdm_seen, sigma_seen = sweep(norb, nelec)
    assert "bra_resident=1 ket_blocks=blocks" in trdm_seen and "chunk=ldg" in sigma_seen


def test_the_sweep_reaches_every_regime():
    trdm_seen, sigma_seen = set(), set()
    for norb, nelec in SWEEP_CASES:
        t, s = sweep(norb, nelec)
        trdm_seen |= t
        sigma_seen |= s
    assert trdm_seen == {"bra_resident=0 ket_blocks=1", "bra_resident=0 ket_blocks>1", "bra_resident=1 ket_blocks<blocks",
                         "bra_resident=1 ket_blocks=blocks"}, sorted(trdm_seen)
    assert {"chunk=64", "64<chunk<ldg, short last chunk", "chunk=ldg"} <= sigma_seen, sorted(sigma_seen)


# ---- evc_fci_excite ---------------------------------------------------------------------------------------------
EXCITE_CASES = [(5, (3, 2)), (7, (3, 4)), (13, (2, 2)), (16, (3, 1))]


def excite_windows(dim):
    """(k0, nk): everything from 0; an unaligned window inside; a window across the end."""
    inside = (37, min(dim - 37 - 5, 301))
    assert inside[1] >= 1 and inside[0] + inside[1] < dim
    return [(0, dim), inside, (dim - 13, 77)]


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("norb,nelec", EXCITE_CASES)
def test_excite_is_the_table_walk_bit_for_bit(norb, nelec, layout):
    p = Problem(norb, nelec)
    _, lib, check = library()
    n2, npad, dim = norb * norb, p.npad, p.dim
    c = np.random.default_rng(norb * 100 + layout).standard_normal((p.na, p.nb))
    E = excite_through_tables(c, norb, nelec).reshape(n2, dim)
    assert np.array_equal(E, _HOST._excite_all(c, norb, nelec).reshape(n2, dim))
    dc = p.up(c)
    for k0, nk in excite_windows(dim):
        rows = np.zeros((nk, n2))                      # rows[kk, pq] = D[pq](k0 + kk), zero from dim on
        live = min(nk, dim - k0)
        rows[:live] = E[:, k0:k0 + live].T
        for ld in ([npad] if layout != 2 else [nk, nk + 9]):
            if layout == 2:
                want = np.full((npad, ld), np.nan)
                want[:, :nk] = 0.0
                want[:n2, :nk] = rows.T
                want = want.reshape(-1)[:(npad - 1) * ld + nk]          # the last row ends with its nk-th element
            else:
                want = np.zeros((nk, npad))
                if layout == 0:
                    want[:, :n2] = rows
                else:
                    want[:, :n2] = rows.reshape(nk, norb, norb).transpose(0, 2, 1).reshape(nk, n2)
                want = want.reshape(-1)
            out = Fenced(8 * want.size, p.dev)
            check(lib.evc_fci_excite(norb, p.na, p.nb, p.ta.data_ptr(), p.tb.data_ptr(), dc.data_ptr(), k0, nk, layout,
                                     out.ptr, ld, None), "evc_fci_excite")
            torch.cuda.synchronize()
            assert out.fences_intact(), (k0, nk, ld)
            assert p.record("fci_excite") == EXCITE_KERNELS[layout]
            got = out.doubles()
            assert np.array_equal(got, want, equal_nan=True), (k0, nk, ld, int((got != want).sum()))
            if layout == 2 and ld > nk:
                assert np.isnan(got.reshape(-1)[nk:ld]).all()            # the gap after the first row
            if layout != 2 and npad > n2:
                assert not got.reshape(nk, npad)[:, n2:].any()           # pad columns: zeros, not NaN, not permuted
