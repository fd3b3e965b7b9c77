"""The pair-sharded phases (evc_phase_hamiltonian / _solve / _gradient and their _batch forms) on the
shapes only a shard gives the kernels, every rank emulated on one device by ``tests/shard_emulation.py``:

A  ranks WITHOUT rows (``shard_rows(10, 7, r)`` gives ranks 5 and 6 none; here also the first rank, the one that adds
   the one-body and nuclear terms): every K5 family with the two-body problem absent, every K8 family with ``rows == 0``
   -- the row-split and the column-tiled VALU kernels, the two matrix-core ones, and the one-body slab pass as the only
   K8 pass with work -- which must still store zeros for every column;
B  more than 32 training states on a shard: ``subspace_big_kernel`` (LDS-resident up to T = 128, global beyond) writes
   the weights ``w2`` and their transposed copy ``w2t`` from global row ``r + w2_offset``; a wrong offset changes the forces
   alone;
C  the K5 plans a shard reaches with >= 12 geometries: the two-body problem on the LDS-staged kernel and the one-body
   problem in a launch of its own, fragment-shaped (T = 118: the unsharded set has too many row groups for the LDS-staged
   kernel at all) or LDS-staged (T = 44).

Every case asserts, against ``oracle.energy_with_grad`` on the original pack2 rows at the slots 0, G // 2, G - 1 and both
sides of the 32-geometry group boundary: every rank's energy, the summed gradient, the predicted RDMs where they are
kept (every rank's 1-RDM, the summed 2-RDM), that every output is finite, that an empty rank's 2-RDM is exactly zero,
and that every rank ran the K5 / K8 (and, in B, subspace) kernels the case names.  The ranks' energies are NOT compared
bit for bit: the one-body span plan depends on the kernel the rank's two-body problem takes.

Tolerances: |dE| <= 1e-10, |dgrad| <= 1e-9 and RDMs <= 1e-10 up to T = 64 (tests/test_gpu_dispatch_map.py);
|dE| <= 1e-10, |dgrad| <= 1e-8 from T = 100 on (tests/test_gpu_large_T.py).

``test_plans_of_every_case`` needs no GPU: the pass sequences named here are what ``evc_trdm_plan_describe`` plans for
every rank of every case on 256 CUs, so a change of the dispatch fails the host-side suite before it moves a case onto a
route that is covered elsewhere."""
import numpy as np
import pytest

from test_trdm_plan import describe as describe_host, lib, passes, trdm_set  # noqa: F401  (lib: fixture)

E_TOL = 1e-10


def shard_rows(rows, world, rank):      # evcont_amd.distributed.shard_rows (imports torch.distributed: kept out of the
    chunk = -(-rows // world)           # host-side test's import)
    r0 = min(rows, rank * chunk)
    return r0, min(rows, r0 + chunk)


def edges(rows):
    """The first and the last rank empty: the first is the one that adds the one-body and nuclear terms."""
    return [(0, 0), (0, rows), (rows, rows)]


def world(w):
    return lambda rows: [shard_rows(rows, w, r) for r in range(w)]


def uneven(rows):
    """A one-row shard in the middle."""
    return [(0, 1), (1, 2), (2, rows)]


# ---- the kernels of a plan, by the number of geometries ---------------------------------------------------------------
K5_VALU = {1: ["gemv_rows_kernel<8,1> G=1"], 2: ["gemv_rows_kernel<8,2> G=2"], 4: ["gemv_rows_wr_kernel<8,4,2> G=4"],
           8: ["gemv_rows_wr_kernel<4,8,4> G=8"]}
K5_SMALL = {**K5_VALU, 12: ["gemv_rows_mfma_pipe_kernel<1,4,2,1> G=12"], 13: ["gemv_rows_mfma_pipe_kernel<1,4,2,1> G=13"],
                            33: ["gemv_rows_mfma_pipe_kernel<2,7,1,1> G=32", "gemv_rows_kernel<8,1> G=1"]}
K8_NARROW = {1: ["gemv_cols_rs_kernel<1>"], 2: ["gemv_cols_rs_kernel<2>"], 4: ["gemv_cols_rs_kernel<4>"],
             8: ["gemv_cols_rs_kernel<8>"], 12: ["gemv_cols_mfma_rs_kernel<2,6,1>"], 13: ["gemv_cols_mfma_rs_kernel<2,6,1>"],
             33: ["gemv_cols_mfma_rs_kernel<8,3,2>", "gemv_cols_rs_kernel<1>"]}
# T^2 >= 1024: the one-body problem of fewer than 12 geometries in row slabs, a pass of its own in front
K8_NARROW_SLAB = {G: (["gemv_cols_slab_kernel"] if G < 12 else []) + names for G, names in K8_NARROW.items()}
K8_LDS_SLAB = {12: ["gemv_cols_mfma_rs_kernel<2,6,1>"], 17: ["gemv_cols_lds_slab_kernel<2,1>"]}


def plan_small(nrows, G):
    return K5_SMALL[G], K8_NARROW[G]


def plan_small_bigT(nrows, G):
    return K5_SMALL[G], K8_NARROW_SLAB[G]


def plan_wide(nrows, G):
    """n = 26, pack2: 228 826 columns -> the column-tiled K8 kernels; a rank with rows stages them through LDS."""
    if nrows == 0:
        k5 = {**K5_VALU, 13: ["gemv_rows_mfma_pipe_kernel<1,4,2,1> G=13"], 17: ["gemv_rows_mfma_pipe_kernel<2,3,2,1> G=17"]}
    else:
        k5 = {**K5_VALU, 13: ["gemv_rows_lds_kernel<1,2,4> G=13"], 17: ["gemv_rows_lds_kernel<2,2,4> G=17"]}
    k8 = {1: "gemv_cols_kernel<1>", 4: "gemv_cols_kernel<4>", 13: "gemv_cols_mfma_kernel<1,2,6,1>",
          17: "gemv_cols_mfma_kernel<2,2,4,2>" if nrows == 0 else "gemv_cols_lds_kernel<2,12,12,8>"}
    return k5[G], [k8[G]]


def plan_fragment(nrows, G):
    """T = 118 on half the rows: the two-body problem LDS-staged, the one-body one on the fragment-shaped kernel."""
    gs, own = (1, "gemv_rows_mfma_pipe_kernel<1,4,2,1>") if G <= 16 else (2, "gemv_rows_mfma_pipe_kernel<2,7,1,1>")
    return [f"gemv_rows_lds_kernel<{gs},14,1> G={G}", f"{own} G={G}"], K8_LDS_SLAB[G]


def plan_own_lds(nrows, G):
    """T = 44 on half the rows: both problems LDS-staged, each in a launch of its own."""
    gs = 1 if G <= 16 else 2
    return [f"gemv_rows_lds_kernel<{gs},4,3> G={G}", f"gemv_rows_lds_kernel<{gs},14,1> G={G}"], K8_LDS_SLAB[G]


def case(id, n, T, A, layout, ranges, G, plan, keep=False, nroots=1, subspace=None, device_rows=False, own_spans=None):
    rows = T * T if layout == "full6" else T * (T + 1) // 2
    return dict(id=id, n=n, T=T, A=A, layout=layout, ranges=ranges(rows), rows=rows, G=G, plan=plan, keep=keep,
                nroots=nroots, subspace=subspace, device_rows=device_rows, own_spans=own_spans,
                g_tol=1e-8 if T >= 100 else 1e-9)


CASES = []
# A: ranks without rows
for lname in ("sym8", "pack2", "full6"):
    for rname, rng in (("edges", edges), ("world7", world(7))):
        for G in (1, 2, 4, 8, 13, 33):
            CASES.append(case(f"A_n6_T4_{lname}_{rname}_G{G}", 6, 4, 3, lname, rng, G, plan_small, keep=True))
for G in (1, 4, 13, 17):
    CASES.append(case(f"A_wide_n26_T2_pack2_G{G}", 26, 2, 2, "pack2", lambda rows: [(0, 0), (0, rows)], G, plan_wide))
for G in (2, 13):
    CASES.append(case(f"A_slab_n6_T40_pack2_G{G}", 6, 40, 3, "pack2", lambda rows: [(0, 0), (0, rows)], G, plan_small_bigT))
# B: the weights of more than 32 training states written at an offset
for n, T, lname in [(6, T, l) for T in (33, 40, 64) for l in ("pack2", "sym8")] + [(4, 128, "pack2"), (4, 130, "pack2")]:
    for rname, rng in (("world3", world(3)), ("uneven", uneven)):
        for G in (1, 2, 13):
            CASES.append(case(f"B_n{n}_T{T}_{lname}_{rname}_G{G}", n, T, 3 if n == 6 else 2, lname, rng, G, plan_small_bigT,
                              subspace="subspace_big_kernel<1>" if T <= 128 else "subspace_big_kernel<0>",
                              device_rows=T >= 100))
CASES.append(case("B_n6_T40_sym8_world3_G2_nroots3", 6, 40, 3, "sym8", world(3), 2, plan_small_bigT, nroots=3,
                  subspace="subspace_big_kernel<1>"))
# C: the K5 plans of a shard
for G in (12, 17):
    CASES.append(case(f"C_fragment_n10_T118_pack2_G{G}", 10, 118, 2, "pack2", world(2), G, plan_fragment, device_rows=True,
                      own_spans=([14, 0], [0, 1])))
for G in (12, 17):
    CASES.append(case(f"C_own_lds_n10_T44_pack2_G{G}", 10, 44, 2, "pack2", world(2), G, plan_own_lds, own_spans=([27, 0], [0, 2])))


def check_plan(text, c, nrows, what):
    """The K5 / K8 pass sequences of one rank equal the ones the case names; every K5 pass of a rank without rows carries
    the one-body problem alone."""
    k5, k8 = passes(text, "K5"), passes(text, "K8")
    want5, want8 = c["plan"](nrows, c["G"])
    assert [p[2] for p in k5] == want5, (what, text)
    assert len(k8) == len(want8) and all(p[2].startswith(w) for p, w in zip(k8, want8)), (what, text)
    if nrows == 0:
        assert all(p[3][0] == 0 and p[3][1] > 0 for p in k5), (what, text)
    if c["own_spans"]:
        assert [p[3] for p in k5] == [list(s) for s in c["own_spans"]], (what, text)
    return k5, k8


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["id"])
def test_plans_of_every_case(lib, c):
    """No GPU: the plan of every rank of the case on a whole device (256 CUs)."""
    assert any(r0 == r1 for r0, r1 in c["ranges"]) == c["id"].startswith("A_")
    for r0, r1 in c["ranges"]:
        t = trdm_set(c["n"], c["T"], c["layout"], rows2=r1 - r0)
        check_plan(describe_host(lib, t, c["G"], 256), c, r1 - r0, (c["id"], r0, r1))
    if c["id"].startswith("C_fragment"):
        # why the case needs a shard: the complete set has too many row groups for the LDS-staged K5 kernel
        full = describe_host(lib, trdm_set(c["n"], c["T"], c["layout"]), c["G"], 256)
        assert all("_lds_" not in p[2] for p in passes(full, "K5")), full


# ---- the GPU cases ------------------------------------------------------------------------------------------------------
class Shape:
    """Training set, geometries and oracle results of one (n, T, A): shared by the cases of that shape, never changed."""

    def __init__(self, n, T, A, device_rows, dev):
        from evcont_amd.synthetic import make_device_trdm_rows, make_trdms, pack_rows
        self.n, self.T, self.A, self.dev = n, T, A, dev
        seed = 52000 + 97 * n + 7 * T
        self.seed = seed
        if device_rows:                       # generated on the device, (rows, cols) of the pack2 layout
            S, one, rows = make_device_trdm_rows(n, T, 2, seed, dev)
            self.dev_set = (one, rows, S)
            self.S, self.one, self.two_p, self.two = S.cpu().numpy(), one.cpu().numpy(), rows.cpu().numpy(), None
        else:
            self.S, self.one, self.two = make_trdms(n, T, seed)
            self.two_p = pack_rows(self.two, True, True)
            self.dev_set = None
        self.aos, self.refs = {}, {}

    def ao(self, k):
        from evcont_amd.synthetic import make_device_ao
        if k not in self.aos:
            self.aos[k] = make_device_ao(self.n, self.A, self.seed * 100 + k, self.dev, ip1_rs_symmetric=True)
        return self.aos[k]

    def bundle(self, k):
        from oracle import evcont_oracle as orc
        a, c = self.ao(k), (lambda t: t.cpu().numpy())
        return orc.AOBundle(S=c(a.S), hcore=c(a.hcore), eri=c(a.eri), ipovlp=c(a.ipovlp), dhcore=c(a.dhcore),
                            eri_ip1=c(a.eri_ip1), aoslices=c(a.aoslices), enuc=a.enuc, gnuc=c(a.gnuc))

    def ref(self, k, full6=False):
        """(E, grad, D, Gamma) of geometry k from the oracle on the pack2 rows (full6: on the unpacked t-RDMs, whose
        predicted 2-RDM differs -- tests/test_gpu_dispatch_map.py)."""
        from oracle import evcont_oracle as orc
        if (k, full6) not in self.refs:
            E, g, D, Gm = orc.energy_with_grad(self.bundle(k), self.one, self.two if full6 else self.two_p, self.S,
                                               return_density_matrices=True)
            self.refs[(k, full6)] = (E, g, np.asarray(D), np.asarray(Gm).reshape((self.n,) * 4))
        return self.refs[(k, full6)]

    def roots(self, k, nroots):
        from oracle import evcont_oracle as orc
        if ("roots", k, nroots) not in self.refs:
            self.refs[("roots", k, nroots)] = orc.approximate_multistate_OAO(self.bundle(k), self.one, self.two_p, self.S,
                                                                             nroots=nroots)[0]
        return self.refs[("roots", k, nroots)]


_shape = {}     # the shape of the cases running now (the cases of a shape are neighbours in CASES)


def shape_of(c, dev):
    key = (c["n"], c["T"], c["A"], c["device_rows"])
    if key not in _shape:
        _shape.clear()
        _shape[key] = Shape(*key, dev)
    return _shape[key]


def sym8(G):
    """Mean over the index permutations of real two-electron integrals: the 2-RDM the compressed layout predicts."""
    a = G + np.swapaxes(G, -4, -3)
    a = a + np.swapaxes(a, -2, -1)
    a = a + np.moveaxis(a, (-2, -1), (-4, -3))
    return a / 8.0


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=lambda c: c["id"])
def test_sharded_phases(c):
    """Worst errors over tolerance on an MI355X (256 CUs), per group -- see DESIGN section 6."""
    import torch
    from evcont_amd import cache
    from shard_emulation import run_sharded
    cache.clear()
    dev = torch.device("cuda:0")
    sh = shape_of(c, dev)
    n, T, A, G, lname = c["n"], c["T"], c["A"], c["G"], c["layout"]
    comp = "sym8" if lname == "sym8" else None
    aos = [sh.ao(k) for k in range(G)]
    run_aos = [a.packed_ip1(eri=True) for a in aos] if comp else aos       # the compressed layout: packed inputs
    if sh.dev_set is not None:
        one, rows, S = sh.dev_set
        run = run_sharded(one, rows, S, c["ranges"], run_aos, A, dev, compress=comp, rows_layout=2, keep=c["keep"],
                          nroots=c["nroots"])
    else:
        run = run_sharded(sh.one, sh.two if lname == "full6" else sh.two_p, sh.S, c["ranges"], run_aos, A, dev,
                          compress=comp, keep=c["keep"], nroots=c["nroots"])
    del run_aos
    # the figures first (printed before anything is asserted), NaN counting as the worst error
    slots = sorted({0, G // 2, G - 1} | ({31, 32} if G > 32 else set()))
    worst = dict(dE=0.0, dgrad=0.0, drdm=0.0, empty_g=0.0)

    def note(key, diff):
        d = float(np.max(np.abs(diff)))
        if not d <= worst[key]:
            worst[key] = d
    for k in slots:
        Eo, go, Do, Go = sh.ref(k)
        for e in run.energy:                                                 # (i) every rank's energy
            note("dE", e[k, 0] - Eo)
            if c["nroots"] > 1:
                note("dE", e[k, : c["nroots"]] - sh.roots(k, c["nroots"]))
        note("dgrad", run.grad[k] - go)                                      # (ii) the summed gradient
        if c["keep"]:                                                        # (iv) the predicted RDMs
            if lname == "full6":
                _, _, Do, Go = sh.ref(k, full6=True)
            elif lname == "sym8":
                Go = sym8(Go)
            for d in run.d_pred:
                note("drdm", d[k] - Do)
            note("drdm", run.g_pred[k] - Go)
    for k, (r0, r1) in enumerate(c["ranges"]):
        if c["keep"] and r0 == r1:
            note("empty_g", run.g_pred_rank[k])
    print(f"SHARD_ROUTES {c['id']} dE={worst['dE']:.3e} dgrad={worst['dgrad']:.3e} drdm={worst['drdm']:.3e} "
          f"empty_g={worst['empty_g']:.3e} k5={[r['k5_rows'] for r in run.records]} "
          f"k8={[r['k8_cols'] for r in run.records]} subspace={run.records[-1]['subspace']}")
    # (vi) every rank ran the kernels the case names: its plan on this device, and the record of the last launch
    for (r0, r1), text, rec in zip(c["ranges"], run.plans, run.records):
        k5, k8 = check_plan(text, c, r1 - r0, (c["id"], r0, r1))
        assert rec["k5_rows"].startswith(k5[-1][2]) and rec["k8_cols"].startswith(k8[-1][2]), (r0, r1, rec, text)
        if c["subspace"]:
            assert rec["subspace"].startswith(c["subspace"]), (r0, r1, rec)
    # (iii) finite everywhere, (v) an empty rank's 2-RDM nothing but stored zeros
    for k, (r0, r1) in enumerate(c["ranges"]):
        assert np.all(np.isfinite(run.energy[k][:, : c["nroots"]])) and np.all(np.isfinite(run.grad_rank[k])), (r0, r1)
        if c["keep"]:
            assert np.all(np.isfinite(run.d_pred[k])) and np.all(np.isfinite(run.g_pred_rank[k])), (r0, r1)
            if r0 == r1:
                assert np.all(run.g_pred_rank[k] == 0.0), (r0, r1, float(np.abs(run.g_pred_rank[k]).max()))
    assert np.all(np.isfinite(run.grad))
    assert worst["dE"] <= E_TOL and worst["dgrad"] <= c["g_tol"] and worst["drdm"] <= 1e-10, worst
