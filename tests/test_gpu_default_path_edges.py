"""GPU tests of the default call paths on inputs the rest of the suite never hands them: training pairs whose (a,b) and
(b,a) blocks differ, a later molecule without the integral symmetries the first one had, HIP-graph replay of the
hosted step with producer-pinned inputs, and a call that follows an energy-only call on the same workspace while the
eigensolver of that call may still run on the side stream.  The reference is always the oracle
(oracle/evcont_oracle.py) on the ORIGINAL arrays; |dE| <= 1e-10 Ha, forces <= 1e-9 Ha/Bohr elementwise."""
import numpy as np
import pytest
import torch

from evcont_amd.synthetic import AOArrays, make_ao_arrays, make_trdms, pack_rows
from oracle import evcont_oracle as orc

pytestmark = pytest.mark.gpu
E_TOL, G_TOL = 1e-10, 1e-9


@pytest.fixture(autouse=True)
def _clean_cache():
    assert torch.cuda.is_available()
    from evcont_amd import cache
    import evcont_amd.ab_initio_eigenvector_continuation as evc
    cache.clear()
    evc._auto_decisions.clear()
    yield
    cache.clear()
    evc._auto_decisions.clear()


def bundle(m):
    return orc.AOBundle(m.S, m.hcore, m.eri, m.ipovlp, m.dhcore, m.eri_ip1, m.aoslices, m.enuc, m.gnuc)


def undeclared(m):
    """The same molecule, declaring nothing about its integral symmetries (checked numerically)."""
    m.integral_symmetry = None
    return m


def assert_matches(E, g, Eo, go, what=""):
    assert abs(E - Eo) <= E_TOL, (what, E, Eo)
    np.testing.assert_allclose(g, go, rtol=0, atol=G_TOL, err_msg=str(what))


# ---- 1. training pairs whose (a,b) and (b,a) blocks differ ----------------------------------------------------------
# (30: the pair-transform path; 34: the 64-wide pair64 path, T small -- a 6-index array at N = 34, T = 4 is 170 MB;
#  T = 36: the large-T subspace kernel and the side-stream Loewdin split)
EDGE_SHAPES = [(6, 3, 2), (30, 3, 2), (34, 4, 2), (5, 36, 2)]


def _training(n, T, seed, ndim, bra_ket_symmetric):
    S, one, two = make_trdms(n, T, seed, bra_ket_symmetric=bra_ket_symmetric)
    return S, one, (two if ndim == 6 else pack_rows(two, pair_sym=False, elec_sym=True))


@pytest.mark.parametrize("ndim", [6, 3])
@pytest.mark.parametrize("n,T,A", EDGE_SHAPES)
def test_bra_ket_asymmetric_training_set_on_default_path(n, T, A, ndim):
    """The reference forms Gamma_pred = sum_ab c_a c_b Gamma[a,b] over ALL pairs; the compressed layout keeps a >= b
    with weight 2 c_a c_b, exact only when (b,a) compresses like (a,b).  With integrals that would let "auto" pick the
    compressed layout, every default entry point must still agree with the oracle (energies agree either way: eigh
    reads the lower triangle; the forces do not)."""
    import evcont_amd.ab_initio_gradients_loewdin as gl
    import evcont_amd.ab_initio_eigenvector_continuation as evc
    from evcont_amd import cache, _lib
    from evcont_amd.MD_utils import get_scanner
    S, one, two = _training(n, T, 300 + n + T, ndim, bra_ket_symmetric=False)
    mol = undeclared(make_ao_arrays(n, A, 301 + n + T, ip1_rs_symmetric=True))
    Eo, go, Do, Go = orc.energy_with_grad(bundle(mol), one, two, S, True, True)
    E, g = gl.get_energy_with_grad(mol, one, two, S)
    assert abs(E - Eo) <= E_TOL, (E, Eo)
    np.testing.assert_allclose(g, go, rtol=0, atol=G_TOL, err_msg="forces of the default call")
    assert cache.get(cache.key_of(one, two, S, ("trdms", "sym8"))) is None, "kept the compressed copy"
    E2, g2, D, G = gl.get_energy_with_grad(mol, one, two, S, return_density_matrices=True)
    assert_matches(E2, g2, Eo, go, "return_density_matrices=True")
    np.testing.assert_allclose(D, Do, rtol=0, atol=1e-10)
    np.testing.assert_allclose(G, np.asarray(Go).reshape(G.shape), rtol=0, atol=1e-10)
    e, _ = evc.approximate_ground_state_OAO(mol, one, two, S)
    assert abs(e - orc.approximate_ground_state_OAO(bundle(mol), one, two, S)[0]) <= E_TOL
    sc = get_scanner(mol, one, two, S)
    Es, gs = sc(mol)
    assert sc._hev.t.layout != _lib.LAYOUT_SYM8 and not sc._hev.packed
    assert_matches(Es, gs, Eo, go, "scanner")
    Eh, gh = gl.get_energy_with_grad(mol, one, two, S, hermitian=False)
    Eho, gho = orc.energy_with_grad(bundle(mol), one, two, S, False)
    assert_matches(Eh, gh, Eho, gho, "hermitian=False")


@pytest.mark.parametrize("ndim", [6, 3])
@pytest.mark.parametrize("n,T,A", [(6, 3, 2), (34, 4, 2), (5, 36, 2)])
def test_bra_ket_symmetric_training_set_keeps_the_compressed_path(n, T, A, ndim):
    """Regression guard of the check above: bra<->ket symmetric data (what every container produces) still runs on the
    compressed layout by default, and matches the oracle."""
    import evcont_amd.ab_initio_gradients_loewdin as gl
    import evcont_amd.ab_initio_eigenvector_continuation as evc
    from evcont_amd import cache, _lib
    from evcont_amd.MD_utils import get_scanner
    S, one, two = _training(n, T, 320 + n + T, ndim, bra_ket_symmetric=True)
    mol = undeclared(make_ao_arrays(n, A, 321 + n + T, ip1_rs_symmetric=True))
    Eo, go = orc.energy_with_grad(bundle(mol), one, two, S)
    E, g = gl.get_energy_with_grad(mol, one, two, S)
    assert_matches(E, g, Eo, go)
    ev = evc._evaluator(one, two, S, A, compress="sym8")
    assert ev.t.layout == _lib.LAYOUT_SYM8 and ev._primed, "the default call did not run on the compressed copy"
    assert cache.get(cache.key_of(one, two, S, ("trdms", None))) is None, "the caller's layout was uploaded as well"
    sc = get_scanner(mol, one, two, S)
    Es, gs = sc(mol)
    assert sc._hev.t.layout == _lib.LAYOUT_SYM8 and sc._hev.packed
    assert_matches(Es, gs, Eo, go, "scanner")


def test_explicit_sym8_refuses_bra_ket_asymmetric_data():
    """compress="sym8" and a container's device_trdms("sym8") were asked for the compressed layout: on data it cannot
    represent they raise (with the reason) instead of falling back; symmetric container data is accepted."""
    from evcont_amd import _lib
    from evcont_amd.containers import TRDMContainer
    from evcont_amd.evaluator import DeviceTRDMs, Sym8NotExact
    dev = torch.device("cuda:0")
    n, T = 6, 4
    S, one, two = make_trdms(n, T, 340, bra_ket_symmetric=False)
    for t in (two, pack_rows(two, pair_sym=False, elec_sym=True)):
        with pytest.raises(Sym8NotExact, match="bra<->ket"):
            DeviceTRDMs(one, t, S, dev, compress="sym8")
    cont = TRDMContainer()
    cont.overlap, cont.one_rdm, cont.two_rdm = S, one, two
    with pytest.raises(Sym8NotExact):
        cont.device_trdms("sym8")
    S2, one2, two2 = make_trdms(n, T, 341)
    cont.overlap, cont.one_rdm, cont.two_rdm = S2, one2, two2
    assert cont.device_trdms("sym8").layout == _lib.LAYOUT_SYM8
    assert DeviceTRDMs(one2, two2, S2, dev, compress="sym8").layout == _lib.LAYOUT_SYM8


# ---- 2. a later molecule without the integral symmetries, same training set -----------------------------------------
@pytest.mark.parametrize("n,T,A", [(10, 4, 3), (20, 3, 2)])
def test_later_molecule_without_integral_symmetry(n, T, A):
    """"auto" decides on a training set's first molecule; a later array-level molecule that declares nothing is
    checked again (a random sample of its integrals) and runs on the caller's layout when it lacks the symmetries.
    The mol-level API must fall back and match the oracle; the MD scanner, whose staging is already packed, raises.
    (Molecules that declare integral_symmetry=True -- the pinned, packed inputs bench.py measures -- are not checked
    per call: tests/test_abi_and_host.py::test_auto_decision_follows_every_molecule.)"""
    import evcont_amd.ab_initio_gradients_loewdin as gl
    import evcont_amd.ab_initio_eigenvector_continuation as evc
    from evcont_amd import _lib
    from evcont_amd.MD_utils import get_scanner
    S, one, two = make_trdms(n, T, 360 + n)
    sym = undeclared(make_ao_arrays(n, A, 361 + n, ip1_rs_symmetric=True))
    gen = undeclared(make_ao_arrays(n, A, 362 + n))          # eri 8-fold, eri_ip1 a general tensor
    Eo_s, go_s = orc.energy_with_grad(bundle(sym), one, two, S)
    Eo_g, go_g = orc.energy_with_grad(bundle(gen), one, two, S)
    assert_matches(*gl.get_energy_with_grad(sym, one, two, S), Eo_s, go_s, "first molecule")
    assert evc._evaluator(one, two, S, A, compress="sym8")._primed
    assert_matches(*gl.get_energy_with_grad(gen, one, two, S), Eo_g, go_g, "second molecule")
    assert_matches(*gl.get_energy_with_grad(sym, one, two, S), Eo_s, go_s, "first molecule again")
    e, _ = evc.approximate_ground_state_OAO(gen, one, two, S)
    assert abs(e - orc.approximate_ground_state_OAO(bundle(gen), one, two, S)[0]) <= E_TOL
    sc = get_scanner(sym, one, two, S)
    assert_matches(*sc(sym), Eo_s, go_s, "scanner, first molecule")
    assert sc._hev.packed
    with pytest.raises(_lib.EvcontHipError, match="symmetr"):
        sc(gen)


# ---- 3. HIP-graph replay of the hosted step with producer-pinned inputs ---------------------------------------------
def _pinned_full(m: AOArrays) -> AOArrays:
    """The molecule with eri / eri_ip1 in pinned host tensors of the (unpacked) staging size: the `_direct` route."""
    out = AOArrays(m.S, m.hcore, m.eri, m.ipovlp, m.dhcore, m.eri_ip1, m.aoslices, m.enuc, m.gnuc,
                   integral_symmetry=m.integral_symmetry)
    keep = []
    for k in ("eri", "eri_ip1"):
        src = np.asarray(getattr(m, k))
        t = torch.zeros(src.size, dtype=torch.float64).pin_memory()
        v = t.numpy().reshape(src.shape)
        np.copyto(v, src)
        setattr(out, k, v)
        keep.append(t)
    out._pinned = keep
    return out


@pytest.mark.parametrize("mode", ["sym8", "caller", "sym8_zero_copy"])
def test_hosted_graph_replay_with_producer_pinned_inputs(mode):
    """A captured step keeps the source addresses of its host-to-device copies.  Alternate two producer-pinned molecules
    with one that is staged by copying, so that replays follow a capture made with another source: every result of the
    graph evaluator must equal an eager evaluator's on the same sequence, and the oracle."""
    from evcont_amd.evaluator import DeviceTRDMs
    from evcont_amd.hosted import HostedEvaluator
    dev = torch.device("cuda:0")
    n, T, A = 20, 4, 2
    S, one, two = make_trdms(n, T, 380)
    two_p = pack_rows(two, True, True)
    trd = DeviceTRDMs(one, two_p, S, dev, compress=None if mode == "caller" else "sym8")
    mols = [make_ao_arrays(n, A, 381 + k, ip1_rs_symmetric=True) for k in range(3)]
    ref = [orc.energy_with_grad(bundle(m), one, two_p, S) for m in mols]
    pin = (lambda m: m.pinned_packed()) if mode != "caller" else _pinned_full
    staged = [pin(mols[0]), pin(mols[1]), mols[2]]
    seq = [0, 1, 0, 1, 2, 1, 2, 0]                        # capture at the third call; replays from every source
    zc = mode == "sym8_zero_copy"
    eager = HostedEvaluator(trd, A, mols[0].aoslices, use_graph=False, zero_copy=zc)
    graph = HostedEvaluator(trd, A, mols[0].aoslices, use_graph=True, zero_copy=zc)
    assert eager.packed == (mode != "caller") and eager.zero_copy == zc
    direct_seen = False
    for step, k in enumerate(seq):
        Ee, ge = eager.energy_with_grad(staged[k])
        direct_seen |= eager._direct_slabs is not None or eager._direct["eri"] is not None
        Eg, gg = graph.energy_with_grad(staged[k])
        assert_matches(Eg, gg, Ee, ge, (mode, step, "graph vs eager"))
        assert_matches(Eg, gg, *ref[k], (mode, step, "graph vs oracle"))
        assert_matches(Ee, ge, *ref[k], (mode, step, "eager vs oracle"))
    assert graph.graph is not None
    assert direct_seen == (not zc), "the eager evaluator did not upload from the producer's buffers"


# ---- 4. a pending side-stream eigensolver and the next call on the same workspace -----------------------------------
def _loewdin_ran():
    from evcont_amd import _lib
    return _lib.load().evc_profile_kernel(_lib.PROF_STAGES["loewdin"]).decode()


def _steps(n, A, seed):
    from test_gpu_warm_start import blend
    a0 = make_ao_arrays(n, A, seed, ip1_rs_symmetric=True)
    a1 = make_ao_arrays(n, A, seed + 1, ip1_rs_symmetric=True)
    return [blend(a0, a1, 0.004 * k) for k in range(3)]


def test_call_after_energy_only_call_with_side_stream_eigensolver():
    """N = 10, T = 40: a cold energy-only call puts the eigensolver of S (it writes U and s) on the side stream; the
    warm full calls that follow on the same workspace read and rewrite U and s on the caller's stream and must wait for
    it.  Each sequence runs ONCE: it guards the result of the sequence and cannot force the race."""
    from evcont_amd.evaluator import ContinuationEvaluator, DeviceAO, DeviceTRDMs
    dev = torch.device("cuda:0")
    n, T, A = 10, 40, 2
    S, one, two = make_trdms(n, T, 400)
    two_p = pack_rows(two, True, True)
    geo = _steps(n, A, 401)
    ev = ContinuationEvaluator(DeviceTRDMs(one, two_p, S, dev), A, warm_start=True)
    e, _ = ev.energies(DeviceAO.from_arrays(geo[0], dev))
    assert "side stream" in _loewdin_ran(), _loewdin_ran()
    assert abs(e[0] - orc.approximate_ground_state_OAO(bundle(geo[0]), one, two_p, S)[0]) <= E_TOL
    for k in (1, 2):
        E, g = ev.energy_with_grad(DeviceAO.from_arrays(geo[k], dev))
        assert "side stream" not in _loewdin_ran(), _loewdin_ran()
        assert_matches(E, g, *orc.energy_with_grad(bundle(geo[k]), one, two_p, S), ("call", k))


def test_phase_loewdin_after_energy_only_call_with_side_stream_eigensolver():
    """The same with the batched entry points: evc_phase_loewdin_batch rewrites U and s right after an energy-only
    call whose eigensolver went to the side stream.  Run once (see above)."""
    from evcont_amd.evaluator import BatchedEvaluator, DeviceAOBatch, DeviceTRDMs
    dev = torch.device("cuda:0")
    n, T, A = 10, 40, 2
    S, one, two = make_trdms(n, T, 410)
    two_p = pack_rows(two, True, True)
    geo = _steps(n, A, 411)
    be = BatchedEvaluator(DeviceTRDMs(one, two_p, S, dev), A, 1, warm_start=True)
    be.enqueue(DeviceAOBatch.from_arrays([geo[0]], dev), energy_only=True)
    assert "side stream" in _loewdin_ran(), _loewdin_ran()
    be.synchronize()
    assert abs(float(be.energy[0, 0]) - orc.approximate_ground_state_OAO(bundle(geo[0]), one, two_p, S)[0]) <= E_TOL
    for k in (1, 2):
        aob = DeviceAOBatch.from_arrays([geo[k]], dev)
        be.phase_loewdin(aob)
        E, g = be.energies_with_grads(aob)
        assert_matches(E[0], g[0], *orc.energy_with_grad(bundle(geo[k]), one, two_p, S), ("call", k))
