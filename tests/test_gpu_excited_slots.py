"""GPU tests of the slot branches of the excited-state gradient entries (include/evcont_hip.h evc_phase_gradient_roots
and evc_phase_gradient_roots_batch): the 8-slot int2e_ip1 form and its short last chunk, the tail block behind the n
partners when the chunk count exceeds n, two K8 groups beyond 32 orbitals, pair lists in any order (couplings first,
couplings only, repeated pairs), workspace reuse across pair counts, the list API's split into batches, and the
coupling vectors against finite differences of the eigenvectors (independent of the oracle's identity for them).

Every slot is held to the oracle of tests/test_gpu_excited_forces.py (``Oracle``: F(c) = grad_elec_OAO of
oracle/evcont_oracle.py on the original arrays) and every geometry of a batch to the single-geometry path
(``check_single``).  A case that targets a branch asserts the IP1 record it reaches (``evc_profile_kernel``)."""
import numpy as np
import pytest

from test_gpu_excited_forces import DEV, Oracle, all_pairs, _h6_training, _bent
from test_gpu_excited_forces_batch import _evs, check_batch, check_single, device_inputs, host_case

pytestmark = pytest.mark.gpu

# nroots = 4 on T = 5: four diagonals, then the couplings in the order of all_pairs(4)
PAIRS8 = all_pairs(4)[:8]
PAIRS9 = all_pairs(4)[:9]


def _record(stage):
    from evcont_amd import _lib
    return _lib.load().evc_profile_kernel(_lib.PROF_STAGES[stage]).decode()


def _ip1_chunks(n):
    """csrc/ip1.hip ip1_chunks: ceil(n^3 / 2048), at least n."""
    return max(-(-n ** 3 // 2048), n)


@pytest.mark.parametrize("pairs", [PAIRS8, PAIRS9, all_pairs(4)], ids=["P8", "P9", "P10"])
def test_batch_roots_eight_slots(pairs):
    """sym8 + packed, N = 6, G = 3: 8 or more root pairs of a geometry share one read of its int2e_ip1 rows in chunks of
    8 (P = 8: one full chunk; 9 and 10: a short last chunk of 1 or 2 slots)."""
    n, T, A, nroots, G = 6, 5, 3, 4, 3
    S, one, two_l, aos = host_case(n, T, A, 36, (1100, 1101, 1102), "sym8_packed")
    oracles = [Oracle(a, one, two_l, S, nroots) for a in aos]
    trd, daos, aob = device_inputs("sym8_packed", S, one, two_l, aos, A)
    res = check_batch(_evs(trd, A, G), aob, oracles, nroots, pairs)
    assert _record("ip1") == "ip1_dh_kernel<8> pairs slots=8", _record("ip1")
    check_single(trd, A, daos, res, nroots, pairs)


def test_batch_roots_slots_with_tail_n48():
    """N = 48: ip1_chunks(48) = 54 > 48, so every slot's partials behind the 48 partners are zeroed by the tail block;
    the 8-slot form (P = 10: chunks of 8 + 2) and the 2-slot form (P = 3: 2 + 1) on one evaluator.  A first call with
    the full integral arrays (the chunks form, which fills all 54 partials of every slot) leaves those partials
    nonzero, so a tail the packed calls did not write would fail the oracle."""
    from evcont_amd.evaluator import DeviceAO, DeviceAOBatch
    n, T, A, nroots, G = 48, 5, 3, 4, 2
    assert _ip1_chunks(n) > n
    S, one, two_l, aos = host_case(n, T, A, 70, (4800, 4801), "sym8_packed")
    oracles = [Oracle(a, one, two_l, S, nroots) for a in aos]
    trd, daos, aob = device_inputs("sym8_packed", S, one, two_l, aos, A)
    del two_l
    ev = _evs(trd, A, G)
    check_batch(ev, DeviceAOBatch.stack([DeviceAO.from_arrays(a, DEV) for a in aos]), oracles, nroots, all_pairs(4),
                tol_g=1e-8)
    assert _record("ip1") == "ip1_dh_kernel<8> chunks", _record("ip1")
    for pairs, rec in ((all_pairs(4), "ip1_dh_kernel<8> pairs slots=8"),
                       (all_pairs(2), "ip1_dh_kernel<8> pairs slots=2")):
        res = check_batch(ev, aob, oracles, nroots, pairs, tol_g=1e-8)
        assert _record("ip1") == rec, (_record("ip1"), len(pairs))
        assert _record("pair_transform").startswith("pt64_kernel"), _record("pair_transform")
        check_single(trd, A, daos, res, nroots, pairs)


def test_batch_roots_n40_two_k8_groups_loewdin_big():
    """N = 40, sym8 + packed, G = 12, P = 3: 36 slots, two K8 groups (32 + 4) with the transposed group weights beyond
    32 orbitals, and the energy call of 12 geometries takes loewdin_big_kernel part=0.  Geometries 0, 6 and 11 against
    the oracle, all twelve against the single-geometry path."""
    from evcont_amd import _lib
    import ctypes as C
    n, T, A, nroots, G = 40, 5, 3, 2, 12
    pairs = all_pairs(nroots)
    S, one, two_l, aos = host_case(n, T, A, 70, range(4000, 4000 + G), "sym8_packed")
    picked = (0, G // 2, G - 1)
    oracles = {g: Oracle(aos[g], one, two_l, S, nroots) for g in picked}
    trd, daos, aob = device_inputs("sym8_packed", S, one, two_l, aos, A)
    del two_l
    ws = _lib.load().evc_workspace_bytes_roots_batch(C.byref(trd.cstruct), A, G, len(pairs))
    assert 0 < ws < 8 << 30, ws           # (a few GB: the case stays at N = 40)
    ev = _evs(trd, A, G)
    res = ev.multistate_energies_with_grads(aob, nroots, pairs)
    for g, o in oracles.items():
        np.testing.assert_allclose(res[0][g], o.E, rtol=0, atol=1e-10, err_msg=f"geometry {g}")
        o.align(res[1][g])
        for p, (k, l) in enumerate(pairs):
            np.testing.assert_allclose(res[2][g, p], o.slot(k, l), rtol=0, atol=1e-8, err_msg=f"geometry {g}, {(k, l)}")
    assert _record("loewdin") == "loewdin_big_kernel part=0", _record("loewdin")
    assert _record("pair_transform").startswith("pt64_kernel"), _record("pair_transform")
    assert _record("ip1") == "ip1_dh_kernel<8> pairs slots=2", _record("ip1")
    assert _record("k8_cols").endswith("<4>"), _record("k8_cols")      # the last group: 36 - 32 = 4 slots
    check_single(trd, A, daos, res, nroots, pairs)


ORDERS = {"coupling_first": [(0, 1), (1, 1), (0, 0)], "coupling_only": [(0, 1)], "couplings": [(1, 2), (0, 2)],
          "repeated": [(1, 1), (1, 1), (0, 1), (0, 1)]}


def _repeats_equal(grads, pairs, what):
    for p, kl in enumerate(pairs):
        q = pairs.index(kl)
        if q != p:
            np.testing.assert_array_equal(grads[p], grads[q], err_msg=f"{what}: slots {q} and {p} of pair {kl}")


@pytest.mark.parametrize("lname", ["pack2", "sym8_packed"])
def test_roots_pair_orders(lname):
    """Pair lists that are not diagonal-first: each output slot is the oracle slot of the pair at its position (the
    nuclear term on the diagonal slots alone, wherever they are), and a repeated pair gives bitwise the same vector.
    Single-geometry and batched entries, one evaluator each for all four lists."""
    from evcont_amd.evaluator import ContinuationEvaluator
    from test_gpu_excited_forces import check
    n, T, A, nroots, G = 6, 5, 3, 3, 2
    S, one, two_l, aos = host_case(n, T, A, 36, (1036, 1037), lname)
    oracles = [Oracle(a, one, two_l, S, nroots) for a in aos]
    trd, daos, aob = device_inputs(lname, S, one, two_l, aos, A)
    ev1, evb = ContinuationEvaluator(trd, A), _evs(trd, A, G)
    for name, pairs in ORDERS.items():
        r1 = check(ev1, daos[0], oracles[0], nroots, pairs)
        _repeats_equal(r1[2], pairs, f"{name}, single")
        res = check_batch(evb, aob, oracles, nroots, pairs)
        for g in range(G):
            _repeats_equal(res[2][g], pairs, f"{name}, geometry {g}")
        check_single(trd, A, daos, res, nroots, pairs)


def test_batch_roots_workspace_reuse():
    """One evaluator: P = 10, then P = 3, then P = 10 again; a slot left stale by a larger call would fail its
    oracle."""
    n, T, A, nroots, G = 6, 5, 3, 4, 3
    S, one, two_l, aos = host_case(n, T, A, 36, (1100, 1101, 1102), "sym8_packed")
    oracles = [Oracle(a, one, two_l, S, nroots) for a in aos]
    trd, daos, aob = device_inputs("sym8_packed", S, one, two_l, aos, A)
    ev = _evs(trd, A, G)
    for pairs, rec in ((all_pairs(4), "slots=8"), ([(2, 3), (0, 3), (1, 1)], "slots=2"), (all_pairs(4), "slots=8")):
        check_batch(ev, aob, oracles, nroots, pairs)
        assert _record("ip1").endswith(rec), (_record("ip1"), rec)


def test_list_api_split_into_batches(monkeypatch):
    """get_multistate_energies_with_grads with a workspace budget of two geometries: 5 H6 geometries go in batches of
    2 + 2 + 1 (a short last batch on its own cached evaluator) and give the unsplit call's E, forces and couplings."""
    import ctypes as C
    from evcont_amd import _lib
    from evcont_amd import ab_initio_gradients_loewdin as agl
    from evcont_amd.hchain import s_gaussian_mol
    cont = _h6_training()
    S, one, two = cont.overlap, cont.one_rdm, cont.two_rdm
    mols = [s_gaussian_mol(_bent(seed=s)) for s in (21, 22, 23, 24, 25)]
    made = []
    orig = agl._batched_evaluator

    def recording(t, natm, count):
        made.append((t, count))
        return orig(t, natm, count)

    monkeypatch.setattr(agl, "_batched_evaluator", recording)
    E, grads, h = agl.get_multistate_energies_with_grads(mols, one, two, S, 3, return_couplings=True)
    assert [c for _, c in made] == [5]
    t = made[0][0]
    per_slot = _lib.load().evc_workspace_bytes_roots_batch(C.byref(t.cstruct), 6, 1, 1)
    assert per_slot > 0
    npairs = len(all_pairs(3))
    monkeypatch.setattr(agl, "BATCH_WORKSPACE_BUDGET", per_slot * npairs * 2 + per_slot)
    made.clear()
    E2, grads2, h2 = agl.get_multistate_energies_with_grads(mols, one, two, S, 3, return_couplings=True)
    assert [c for _, c in made] == [2, 2, 1]
    np.testing.assert_allclose(E2, E, rtol=0, atol=1e-12)
    np.testing.assert_allclose(grads2, grads, rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.abs(h2), np.abs(h), rtol=0, atol=1e-12)     # (signs follow the eigenvectors)
    for g in range(len(mols)):
        np.testing.assert_array_equal(h2[g], np.swapaxes(h2[g], 0, 1))


# max |h_kl - h_kl^FD| measured on an MI355X: 6.7e-10 Ha/Bohr (central differences, step 2e-4 Bohr); 15x margin
FD_TOL = 1e-8


def test_couplings_against_finite_differences():
    """For k != l, c_k^T dH/dR c_l = (E_l - E_k) c_k^T S_train dc_l/dR (S_train does not depend on the geometry, c is
    S-normalised): the coupling slots (0,1), (0,2), (1,2) of the H6 training at a bent geometry against central
    differences of the device eigenvectors, through the single and the batched entries.  Every force and coupling
    vector also carries no net force and no net torque (the s-Gaussian basis is rotation-invariant)."""
    from evcont_amd.evaluator import DeviceTRDMs, DeviceAO, DeviceAOBatch, ContinuationEvaluator
    from evcont_amd.hchain import s_gaussian_mol
    cont = _h6_training()
    S, one, two = cont.overlap, cont.one_rdm, cont.two_rdm
    trd = DeviceTRDMs(one, two, S, DEV)
    ev = ContinuationEvaluator(trd, 6)
    R, R2 = _bent(), _bent(seed=12)
    pairs = all_pairs(3)
    E, Cr, g1 = ev.energies_with_grads(DeviceAO.from_arrays(s_gaussian_mol(R), DEV), 3, pairs)
    assert np.min(np.diff(E)) >= 1e-2, E
    evb = _evs(trd, 6, 2)
    Eb, Cb, gb = evb.multistate_energies_with_grads(DeviceAOBatch.from_arrays([s_gaussian_mol(R), s_gaussian_mol(R2)],
                                                                              DEV), 3, pairs)
    np.testing.assert_allclose(Eb[0], E, rtol=0, atol=1e-12)
    sb = np.sign(np.sum(Cb[0] * Cr, axis=1))
    St = np.asarray(S)

    def coeffs(r):
        _, c = ev.energies(DeviceAO.from_arrays(s_gaussian_mol(r, need_grad=False), DEV, energy_only=True), 3)
        return c * np.sign(np.sum(c * Cr, axis=1))[:, None]          # (the sign of c_l(R))

    step = 2e-4
    dC = np.zeros((6, 3, 3, St.shape[0]))
    for a in range(6):
        for x in range(3):
            Rp, Rm = R.copy(), R.copy()
            Rp[a, x] += step
            Rm[a, x] -= step
            dC[a, x] = (coeffs(Rp) - coeffs(Rm)) / (2 * step)
    dev, size = 0.0, {}
    for p, (k, l) in enumerate(pairs):
        if k == l:
            continue
        h_fd = (E[l] - E[k]) * np.einsum("t,ts,axs->ax", Cr[k], St, dC[:, :, l])
        size[(k, l)] = float(np.abs(h_fd).max())
        dev = max(dev, float(np.abs(g1[p] - h_fd).max()), float(np.abs(gb[0, p] * sb[k] * sb[l] - h_fd).max()))
    print(f"coupling vs finite differences: max deviation {dev:.2e} Ha/Bohr; max |h_kl| {size}")
    # (roots 0 and 2 couple, |h_02| ~ 0.05 Ha/Bohr; h_01 and h_12 vanish by symmetry and are held to zero the same way)
    assert max(size.values()) > 1e-2, size
    assert dev < FD_TOL, dev
    for what, grads, Rg in (("single", g1, R), ("batch 0", gb[0], R), ("batch 1", gb[1], R2)):
        for p in range(len(pairs)):
            assert np.abs(grads[p].sum(axis=0)).max() < 1e-8, (what, pairs[p])
            assert np.abs(np.cross(Rg, grads[p]).sum(axis=0)).max() < 1e-8, (what, pairs[p])
