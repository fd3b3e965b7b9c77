"""GPU tests of ``evc_cas_expand_rows`` (csrc/cas_expand.hip) on random inputs against a numpy einsum of the expansion
(step 5 of evcont_amd/cas_small.py), called through the C interface with device tensors.

Grid: ncas in {1, 2, 3, 4, 5, 8, 11, 13, 16} (K not a multiple of 4; one, two, three -- 11 alone -- and four MFMA
K-steps, so every instantiation of the step kernel) x n in {ncas, 5, 16, 17, 31, 33, 48, 64}, n >= ncas (ragged and exact
16-tiles, both ends of the range).  Each (ncas, n) is one test that shares its
inputs and its reference.  Up to n = 33, and at (ncas, n) = (16, 64), it runs everything: three kets and one, Qc given and NULL,
the three layouts, a repeated run, a wide pitch.  At the other shapes with n = 48 and 64 the dense block has 5 and 17
million elements, so one ket with Qc is expanded densely for every ncas, and Qc = NULL and the packed layouts only at
ncas = 1 and 16: the core kernel and the packing kernel do
not see ncas, and the loop over the kets does not see n, so no launch shape is left out -- the test after the grid holds
the record of the calls made against ``evc_cas_expand_describe``.

No call here runs in a child process under a time limit of its own: a child costs seconds of start-up per case, against
milliseconds of work, and every loop of the three kernels is bounded by its arguments (a grid-stride walk over a finite
number of tiles, no wait on another block, no atomics), so there is nothing that can spin; scripts that run this file on
a device put the pytest process itself under ``timeout``.

Tolerance (derived, not measured): an element is a sum of products with at most 4 ncas + 8 <= 72 roundings, so it is
held to 128 * 2^-53 times the same formula evaluated with the absolute value of every factor.
Packed rows must have the bits of the host codecs (tests/fci_pack_reference.py) applied to the dense result of the same
inputs; a second run, and the single-ket call on a ket of the three-ket call, must give the same bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from fci_pack_reference import pack_cols, pack_row

pytestmark = pytest.mark.gpu

NCAS = (1, 2, 3, 4, 5, 8, 11, 13, 16)
SHAPES = [(c, n) for c in NCAS for n in sorted({c, 5, 16, 17, 31, 33, 48, 64}) if n >= c]
U = 2.0 ** -53
LAYOUTS = {"full6": 6, "pack2": 2, "sym8": 8}


CALLED = set()          # (n, ncas, layout) of every evc_cas_expand_rows call that Device.call made and that returned 0


def everything(ncas, n):
    """Whether (ncas, n) runs the packed layouts, Qc = NULL and three kets (see the module docstring)."""
    return n <= 33 or (ncas, n) == (16, 64)


def packed_too(ncas, n):
    return n <= 33 or ncas in (1, 16)


@functools.lru_cache(maxsize=None)
def lib():
    from evcont_amd import _lib
    return _lib.load()


def describe(n, ncas, layout):
    buf = C.create_string_buffer(4096)
    assert 0 < lib().evc_cas_expand_describe(n, ncas, LAYOUTS[layout], buf, len(buf)) < len(buf)
    return buf.value.decode().splitlines()


def inputs(ncas, n, nkets):
    rng = np.random.default_rng(9000 + 97 * ncas + n)
    f = lambda *s: rng.standard_normal(s)
    return dict(A=0.5 * f(nkets, n, ncas), B=0.5 * f(nkets, n, ncas), Qc=0.3 * f(nkets, n, n), S=rng.uniform(-1, 1, nkets),
                d1=f(nkets, ncas, ncas), d2=f(nkets, ncas, ncas, ncas, ncas))


def statement(x, i, core, absolute=False):
    """(dm1, dm2) of ket i by the formula; ``absolute``: every factor by its absolute value and every sign a plus."""
    g = np.abs if absolute else (lambda a: a)
    sgn = 1.0 if absolute else -1.0
    A, B, d1, d2, S = g(x["A"][i]), g(x["B"][i]), g(x["d1"][i]), g(x["d2"][i]), g(x["S"][i])
    Qa = A @ d1.T @ B.T
    dm2 = np.einsum("tuvw,pt,qu,rv,sw->pqrs", d2, A, B, A, B, optimize=True)
    if not core:
        return Qa.T.copy(), dm2
    Qc = g(x["Qc"][i])
    e = lambda s, a, b: np.einsum(s, a, b)
    dm2 += S * (4.0 * e("pq,rs->pqrs", Qc, Qc) + sgn * 2.0 * e("ps,rq->pqrs", Qc, Qc))
    dm2 += 2.0 * e("pq,rs->pqrs", Qc, Qa) + 2.0 * e("pq,rs->pqrs", Qa, Qc)
    dm2 += sgn * (e("ps,rq->pqrs", Qc, Qa) + e("ps,rq->pqrs", Qa, Qc))
    return (2.0 * S * Qc + Qa).T, dm2


class Device:
    """The inputs of one shape on the device, and the calls on them."""

    def __init__(self, x, n, ncas):
        self.n, self.ncas = n, ncas
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        self.t = {k: up(v) for k, v in x.items()}
        self.ws = None

    def call(self, kets, core, layout, ld=None):
        """evc_cas_expand_rows on the listed kets: (dm1 (K, n, n), rows (K, ld)) as numpy, from NaN-filled targets."""
        n, ncas, K, t = self.n, self.ncas, len(kets), self.t
        sel = lambda a: a[kets].contiguous()
        A, B, Qc, S, d1, d2 = sel(t["A"]), sel(t["B"]), sel(t["Qc"]), sel(t["S"]), sel(t["d1"]), sel(t["d2"])
        if ld is None:
            ld = n ** 4 if layout == "full6" else (pack_cols(layout, n) + 15) // 16 * 16 + 16
        need = lib().evc_cas_expand_workspace_bytes(n, ncas, K)
        assert need > 0
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(need, dtype=torch.uint8, device="cuda:0")
        dm1 = torch.full((K, n, n), float("nan"), dtype=torch.float64, device="cuda:0")
        rows = torch.full((K, ld), float("nan"), dtype=torch.float64, device="cuda:0")
        rc = lib().evc_cas_expand_rows(n, ncas, K, A.data_ptr(), B.data_ptr(), Qc.data_ptr() if core else None,
                                       S.data_ptr(), d1.data_ptr(), d2.data_ptr(), dm1.data_ptr(), LAYOUTS[layout],
                                       rows.data_ptr(), ld, self.ws.data_ptr(), need,
                                       torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib().evc_last_error()
        torch.cuda.synchronize()
        CALLED.add((n, ncas, layout))
        return dm1.cpu().numpy(), rows.cpu().numpy()


def check_dense(x, kets, core, dm1, rows, n, tag):
    for k, i in enumerate(kets):
        want1, want2 = statement(x, i, core)
        tol1, tol2 = (128.0 * U * b for b in statement(x, i, core, absolute=True))
        e1, e2 = np.abs(dm1[k] - want1), np.abs(rows[k].reshape(n, n, n, n) - want2)
        print(f"cas expand {tag} ket {i} core={int(core)}: dm1 err/tol = {float((e1 / tol1).max()):.3f}  "
              f"dm2 err/tol = {float((e2 / tol2).max()):.3f}  max|dm2| = {float(np.abs(want2).max()):.3e}")
        assert (e1 <= tol1).all() and (e2 <= tol2).all(), (tag, i, core)


def check_packed(dev, kets, core, dm1, dense, n, tag):
    for layout in ("pack2", "sym8"):
        cols = pack_cols(layout, n)
        p1, prow = dev.call(kets, core, layout)
        assert np.array_equal(p1, dm1), (tag, layout)
        for k in range(len(kets)):
            assert np.array_equal(prow[k, :cols], pack_row(layout, dense[k].reshape(n, n, n, n))), (tag, layout, k)
            assert not prow[k, cols:].any(), (tag, layout, k)                     # zeros, not NaN


@pytest.mark.parametrize("ncas,n", SHAPES, ids=[f"{c}-{n}" for c, n in SHAPES])
def test_expand_against_the_einsum(ncas, n):
    tag = f"ncas={ncas} n={n}"
    nkets = 3 if everything(ncas, n) else 1
    x = inputs(ncas, n, nkets)
    dev = Device(x, n, ncas)
    kets = list(range(nkets))
    dm1, rows = dev.call(kets, True, "full6")
    check_dense(x, kets, True, dm1, rows, n, tag)
    again = dev.call(kets, True, "full6")
    assert np.array_equal(again[0], dm1) and np.array_equal(again[1], rows), tag      # run to run
    if nkets > 1:
        for i in (1, 2):
            one1, one2 = dev.call([i], True, "full6")
            assert np.array_equal(one1[0], dm1[i]) and np.array_equal(one2[0], rows[i]), (tag, i)
        # a pitch wider than the block: nothing is written between the rows
        wide1, wide2 = dev.call(kets, True, "full6", ld=n ** 4 + 6)
        assert np.array_equal(wide2[:, :n ** 4], rows) and np.isnan(wide2[:, n ** 4:]).all(), tag
    if packed_too(ncas, n):
        check_packed(dev, kets, True, dm1, rows, n, tag)
        # no core orbitals: Qc = NULL
        f1, frows = dev.call(kets, False, "full6")
        check_dense(x, kets, False, f1, frows, n, tag)
        if everything(ncas, n):
            check_packed(dev, kets, False, f1, frows, n, tag)


def test_describe_lines_of_the_grid_are_all_exercised():
    """Every line ``evc_cas_expand_describe`` gives for a shape and layout of the grid is a line of a call that
    ``Device.call`` made in this session and that succeeded (``CALLED``): this test runs after the grid above, in the
    same process, and fails if the grid was deselected."""
    assert {(n, ncas, "full6") for ncas, n in SHAPES} <= CALLED, "run together with test_expand_against_the_einsum"
    run = set()
    for n, ncas, layout in CALLED:
        run |= {(n if "fci_row_pack" in ln else (n, ncas), ln) for ln in describe(n, ncas, layout)}
    steps = set()
    for ncas, n in SHAPES:
        for layout in LAYOUTS:
            for ln in describe(n, ncas, layout):
                assert (n if "fci_row_pack" in ln else (n, ncas), ln) in run, (ncas, n, layout, ln)
                steps |= {ln.split()[0]}
    assert steps == {"cas_qa_kernel", "cas_core_kernel", "fci_row_pack_kernel<1>", "fci_row_pack_kernel<8>"} | {
        f"cas_step_kernel<{k}>" for k in (1, 2, 3, 4)}


def test_refused_on_the_device_too():
    x = inputs(4, 6, 1)
    dev = Device(x, 6, 4)
    t = dev.t
    ws = torch.empty(lib().evc_cas_expand_workspace_bytes(6, 4, 1), dtype=torch.uint8, device="cuda:0")
    dm1 = torch.zeros((1, 6, 6), dtype=torch.float64, device="cuda:0")
    rows = torch.zeros((1, 6 ** 4), dtype=torch.float64, device="cuda:0")
    args = lambda layout, ld, wsb: (6, 4, 1, t["A"].data_ptr(), t["B"].data_ptr(), None, t["S"].data_ptr(),
                                    t["d1"].data_ptr(), t["d2"].data_ptr(), dm1.data_ptr(), layout, rows.data_ptr(), ld,
                                    ws.data_ptr(), wsb, None)
    for layout, ld, wsb in ((5, 6 ** 4, ws.numel()), (2, 670, ws.numel()), (6, 6 ** 4, ws.numel() - 1)):
        assert lib().evc_cas_expand_rows(*args(layout, ld, wsb)) < 0
        assert lib().evc_last_error().startswith(b"evc_cas_expand_rows")
    torch.cuda.synchronize()
    assert not rows.any().item() and not dm1.any().item()
