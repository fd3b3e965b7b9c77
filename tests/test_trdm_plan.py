"""The K5 / K8 dispatch of a call as ``evc_trdm_plan_describe`` prints it (csrc/gemv_dispatch.hip): a pure function of
the shapes, the batch size, the CU count and the knobs, so every assertion here runs without a GPU.

* the kernel each row of ``tests/dispatch_table.py`` expects for K5 / K8 (confirmed on hardware by
  ``tests/test_gpu_dispatch_map.py``) is the kernel of the plan's last pass;
* the whole pass sequence around the group boundaries, and the workspace sizes, equal those recorded from the commit
  before the plan became a value (``tests/golden/trdm_plan.json``: the pass sequences by a host program linked against
  that commit's launchers with the launches recorded instead of made, the sizes by its library);
* no plan has more spans than the partial buffers are carved for."""
import ctypes as C
import json
import os
import random

import pytest

from dispatch_table import CASES

LAYOUT = {"full6": 6, "pair5": 5, "elec3": 3, "pack2": 2, "sym8": 8}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trdm_plan.json")


@pytest.fixture(scope="module")
def lib():
    from evcont_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def trdm_set(n, T, layout, rows2=None):
    """The integer fields of a set as check_set (csrc/workspace.hip) wants them and the evaluator pads them: ld2 = cols2
    rounded up to 16, ld1 = n^2 rounded up to even.  The pointers only have to pass the NULL / alignment checks of the
    workspace functions; nothing reads them."""
    from evcont_amd._lib import TrdmSet
    n2, ns = n * n, n * (n + 1) // 2
    cols = ns * (ns + 1) // 2 if layout == "sym8" else (n2 * (n2 + 1) // 2 if layout in ("elec3", "pack2") else n2 * n2)
    rows = T * (T + 1) // 2 if layout in ("pair5", "pack2", "sym8") else T * T
    return TrdmSet(n=n, ntrain=T, layout=LAYOUT[layout], rows2=rows if rows2 is None else rows2, row_offset=0,
                   rows2_total=rows, cols2=cols, ld2=(cols + 15) // 16 * 16, ld1=(n2 + 1) // 2 * 2, two_rdm=256,
                   one_rdm=256, s_train=256)


def describe(lib, t, count, cus):
    buf = C.create_string_buffer(1 << 16)
    n = lib.evc_trdm_plan_describe(C.byref(t), count, cus, buf, len(buf))
    assert 0 <= n < len(buf), lib.evc_last_error()
    return buf.value.decode()


def passes(text, stage):
    """[(g0, G, kernel name, [nspans two-body, one-body] or None)] of the stage's lines."""
    out = []
    for line in text.splitlines():
        st, g0, G, rest = line.split(" ", 3)
        if st != stage:
            continue
        spans = None
        if stage == "K5":
            rest, s = rest.rsplit(" nspans=", 1)
            spans = [int(x) for x in s.split(",")]
        out.append((int(g0[3:]), int(G[2:]), rest, spans))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_dispatch_table_rows(lib, case):
    """K5 runs the G geometries of the call; K8 the slots of the gradient call: G, G * len(pairs) for roots_batch,
    len(pairs) for roots."""
    t = trdm_set(case["n"], case["T"], case["layout"])
    slots = {"roots": len(case["pairs"] or []), "roots_batch": case["G"] * len(case["pairs"] or [])}.get(case["api"],
                                                                                                       case["G"])
    expect = case["expect_grad"] if case["energy_only"] else case["expect"]
    k5 = passes(describe(lib, t, case["G"], 256), "K5")
    k8 = passes(describe(lib, t, slots, 256), "K8")
    assert k5[-1][2].startswith(case["expect"]["k5_rows"]), k5
    assert k8[-1][2].startswith(expect["k8_cols"]), k8
    assert sum(p[1] for p in k8 if "slab_kernel" not in p[2] or "lds" in p[2]) == slots


def test_pass_sequences_equal_the_recorded_ones(lib, golden):
    """H30 / T = 20 and n = 6 / T = 3 (sym8) around every group boundary, on a whole device (256 CUs) and on one the
    LDS-staged kernels do not fit (128); the Zundel shape with T = 100, whose one-body problem takes an LDS-staged launch
    of its own (the shape of tests/test_gpu_large_T.py::test_zundel_shape_T100_against_oracle[32], which runs it on the
    GPU); and a 3500-row shard of T = 118, whose one-body problem falls back to the fragment-shaped kernel (run on the
    GPU, on both halves of a T = 118 set, by tests/test_gpu_shard_routes.py::test_sharded_phases[C_fragment_*])."""
    assert {p["count"] for p in golden["plans"]} == {1, 2, 3, 4, 8, 9, 11, 12, 16, 17, 32, 33, 44, 64, 65, 76, 96}
    assert {(p["n"], p["T"], p["cus"]) for p in golden["plans"]} >= {(30, 20, 256), (30, 20, 128), (6, 3, 256), (6, 3, 128)}
    for p in golden["plans"]:
        t = trdm_set(p["n"], p["T"], p["layout"], p["rows2"])
        assert describe(lib, t, p["count"], p["cus"]) == p["text"], p
        if p["cus"] < 250:
            assert "_lds_" not in p["text"], p
    own = {(p["n"], p["T"]): passes(p["text"], "K5") for p in golden["plans"] if p["cus"] == 256 and p["count"] == 32}
    for shape, second in (((28, 100), "gemv_rows_lds_kernel<2,14,1> G=32"), ((13, 118), "gemv_rows_mfma_pipe_kernel<2,7,1,1> G=32")):
        (g0a, Ga, ka, sa), (g0b, Gb, kb, sb) = own[shape]        # two passes with the same geometries
        assert (g0a, Ga) == (g0b, Gb) == (0, 32) and ka.startswith("gemv_rows_lds_kernel") and kb == second
        assert sa[0] > 0 and sa[1] == 0 and sb[0] == 0 and sb[1] > 0


def test_rank_without_rows(lib):
    """A shard with no two-body rows: every K5 pass carries the one-body problem alone, K8 still writes its columns."""
    t = trdm_set(30, 20, "sym8", rows2=0)
    for count in (1, 5, 12, 32, 44):
        text = describe(lib, t, count, 256)
        k5, k8 = passes(text, "K5"), passes(text, "K8")
        assert sum(p[1] for p in k5) == sum(p[1] for p in k8) == count
        assert all(p[3][0] == 0 and p[3][1] > 0 for p in k5) and "_lds_" not in text, text


def carved_spans(rows, cols, small):
    """Spans the workspace carves the partial sums of a (rows, cols) problem for -- written out here from the rule the
    workspace layout has had since the LDS-staged K5 kernel (the finer of the two VALU span plans, or the LDS-staged plan
    with 14-tile row groups in a round of 250 workgroups, 8 for a one-body problem of at most 8 row groups), not read
    from the library: test_workspace_sizes_equal_the_recorded_ones pins the library's carving to the recorded sizes."""
    cdiv = lambda a, b: -(-a // b)
    nchunks, want = cdiv(cols, 512), cdiv(8192, cdiv(rows, 8))
    cps = nchunks // want
    if cps < 2:
        cps = max(1, min(nchunks, 2))
    nrg = cdiv(cdiv(rows, 16), 14)
    spans = max(1, (8 if small and nrg <= 8 else 250) // nrg)
    m = max(1, cdiv(cdiv(cols, 16), 4 * spans))
    return max(cdiv(cols, 512 * cps), cdiv(cols, 64 * m))


def test_partial_buffers_cover_every_plan(lib):
    """About 200 shapes (consistent or not: shards, any width): no K5 pass has more spans than the partial buffers hold
    -- the two-body buffer evc_gemv_rows_ws_bytes / rows spans (which is carved_spans of it), the one-body buffer, carved
    inside the workspace with no size function of its own, carved_spans(T^2, n^2, small)."""
    rng = random.Random(20)
    from evcont_amd._lib import TrdmSet
    for i in range(200):
        rows2 = rng.choice([1, 16, 17, rng.randint(1, 300), rng.randint(1, 12000)])
        cols2 = rng.choice([1, 64, 4096, 200000, 200001, rng.randint(1, 20000), rng.randint(1, 500000)])
        T, n = rng.choice([1, 32, rng.randint(1, 160)]), rng.choice([1, 8, 46, rng.randint(1, 64)])
        count, cus = rng.choice([1, 2, 12, 32, 44, 64, 96, rng.randint(1, 96)]), rng.choice([128, 256])
        t = TrdmSet(n=n, ntrain=T, layout=8, rows2=rows2, row_offset=0, rows2_total=rows2, cols2=cols2,
                    ld2=(cols2 + 15) // 16 * 16, ld1=(n * n + 1) // 2 * 2, two_rdm=256, one_rdm=256, s_train=256)
        cap2 = lib.evc_gemv_rows_ws_bytes(rows2, cols2) // 8 // rows2
        cap1 = carved_spans(T * T, n * n, True)
        assert cap2 == carved_spans(rows2, cols2, False)
        k5 = passes(describe(lib, t, count, cus), "K5")
        assert k5 and sum(p[1] for p in k5 if p[3][0]) == count, (rows2, cols2, T, n, count, cus, k5)
        for g0, G, name, spans in k5:
            assert 0 <= spans[0] <= cap2 and 0 <= spans[1] <= cap1, (rows2, cols2, T, n, count, cus, name, spans, cap2, cap1)


def test_workspace_sizes_equal_the_recorded_ones(lib, golden):
    assert len(golden["workspace"]) >= 60 and {w["layout"] for w in golden["workspace"]} == set(LAYOUT)
    for w in golden["workspace"]:
        t = trdm_set(w["n"], w["T"], w["layout"])
        got = dict(workspace_bytes=lib.evc_workspace_bytes(C.byref(t), w["natm"]),
                   workspace_bytes_batch=lib.evc_workspace_bytes_batch(C.byref(t), w["natm"], w["count"]),
                   workspace_bytes_roots_batch=lib.evc_workspace_bytes_roots_batch(C.byref(t), w["natm"], w["count"],
                                                                                   w["npairs"]),
                   gemv_rows_ws_bytes=lib.evc_gemv_rows_ws_bytes(t.rows2, t.cols2))
        assert got == {k: w[k] for k in got}, w
