"""GPU tests of the CI-vector rotation under an orbital transformation: evc_fci_rotate (csrc/fci_rotate.hip) called
directly with fenced, NaN-poisoned buffers, DeviceFCI.transform_ci, and the canonical-basis route of FCI_EVCont_obj.

The reference is fci_small.transform_ci (T_a^T c T_b with fci_small.minor_matrix, numpy.linalg.det; the matrices are
formed once per shape and shared); for signed permutations the expected array is built by
moving entries (tests/test_fci_rotate_host.py: permuted_by_strings), so that comparison is bit for bit.

The rounding bound, per element, for unit-norm rows of T (orthogonal u):
    2 * 2^-53 * |c|_2 * [ (na + nb) + (sqrt(na) + sqrt(nb)) * 8 k^3 ],      k = the larger electron count
first term: the two dot products; second: the error of an LU determinant carried through them.  For a general u the
same, times max(1, |T_a|_2 |T_b|_2) of the host matrices."""
import functools
import re

import numpy as np
import pytest
import torch

from evcont_amd.fci_small import _strings, minor_matrix
from evcont_amd.hchain import hydrogen_chain
from test_fci_rotate_closure import ROTATE_RECORD
from test_fci_rotate_host import general_u, permuted_by_strings, random_orthogonal, signed_permutation
from test_gpu_fci_abi import Fenced, library

pytestmark = pytest.mark.gpu

SHAPES = [(1, (1, 0)), (2, (1, 1)), (4, (2, 2)), (5, (3, 2)), (6, (5, 4)), (7, (0, 7)), (8, (4, 4)),
          (9, (8, 1)), (10, (8, 2)), (9, (7, 2)), (10, (5, 5)),
          (10, (9, 1)), (12, (10, 2)), (16, (15, 1)),
          (12, (6, 6))]
LARGEST = (16, (8, 1))          # exact test only: the host has no determinants to compute
PANEL_DOUBLES = 1 << 19


def minor_order(norb, k):
    """(instantiation, complement route) for k electrons of one spin."""
    if k == 0 or k == norb:
        return 1, 0
    return (k, 0) if k <= 8 else (norb - k, 1)


def panels(ns):
    width = min(ns, max(64, PANEL_DOUBLES // ns // 64 * 64))
    return -(-ns // width)


def expected_record(norb, nelec, na, nb):
    (ka, ca), (kb, cb) = minor_order(norb, nelec[0]), minor_order(norb, nelec[1])
    return (f"fci_minor_kernel<{ka}> + fci_minor_kernel<{kb}> comp={ca},{cb} panels={panels(na)},{panels(nb)} + "
            "fci_rotate_gemm_kernel")


def test_the_shapes_reach_every_instantiation_and_route():
    orders = {minor_order(n, k) for n, ne in SHAPES + [LARGEST] for k in ne}
    assert {o for o, c in orders if not c} == set(range(1, 9))
    assert {o for o, c in orders if c} >= {1, 2}                              # complementary minors
    assert any(0 in ne for _, ne in SHAPES) and any(n in ne for n, ne in SHAPES)
    assert any(ne[0] != ne[1] for _, ne in SHAPES)
    assert panels(924) == 2 and panels(12870) == 202 and panels(252) == 1     # (12, (6, 6)) and LARGEST are panelled


class Problem:
    def __init__(self, norb, nelec):
        self.lib_mod, self.lib, self.check = library()
        self.dev = torch.device("cuda:0")
        self.norb, self.nelec = norb, nelec
        sa, sb = _strings(norb, nelec[0]), _strings(norb, nelec[1])
        self.na, self.nb = len(sa), len(sb)
        self.sa = torch.tensor(sa, dtype=torch.int32, device=self.dev)
        self.sb = torch.tensor(sb, dtype=torch.int32, device=self.dev)
        self.least = self.lib.evc_fci_rotate_workspace_bytes(norb, nelec[0], nelec[1], self.na, self.nb, 1)
        self.full = self.lib.evc_fci_rotate_workspace_bytes(norb, nelec[0], nelec[1], self.na, self.nb, 0)
        assert 0 < self.least <= self.full
        self.want_record = expected_record(norb, nelec, self.na, self.nb)
        assert re.fullmatch(ROTATE_RECORD, self.want_record)

    def record(self):
        return self.lib.evc_profile_kernel(self.lib_mod.FCI_PROF_ROTATE).decode()

    def call(self, c, ua, ub, ws_bytes, out=None, na=None, norb=None):
        """rc, output (na, nb), the input as it is afterwards"""
        ua = np.ascontiguousarray(ua, dtype=np.float64)
        ub = ua if ub is None else np.ascontiguousarray(ub, dtype=np.float64)
        dc = torch.from_numpy(np.ascontiguousarray(c, dtype=np.float64).reshape(-1)).to(self.dev)
        ws = Fenced(ws_bytes, self.dev, front=False)
        res = Fenced(8 * self.na * self.nb, self.dev)
        rc = self.lib.evc_fci_rotate(self.norb if norb is None else norb, self.nelec[0], self.nelec[1],
                                     self.na if na is None else na, self.nb, self.sa.data_ptr(), self.sb.data_ptr(),
                                     ua.ctypes.data, ub.ctypes.data, dc.data_ptr(),
                                     dc.data_ptr() if out == "alias" else res.ptr, ws.ptr, ws_bytes, None)
        torch.cuda.synchronize()
        assert ws.fences_intact() and res.fences_intact(), ws_bytes
        return rc, res.doubles().reshape(self.na, self.nb), dc.cpu().numpy().reshape(self.na, self.nb)

    def rotate(self, c, ua, ub=None, ws_bytes=None):
        rc, out, after = self.call(c, ua, ub, self.full if ws_bytes is None else ws_bytes)
        self.check(rc, "evc_fci_rotate")
        assert self.record() == self.want_record, (self.record(), self.want_record)
        assert np.array_equal(after, c)                                     # the input is not written
        return out


@functools.lru_cache(maxsize=None)
def problem(norb, nelec):
    return Problem(norb, nelec)


def integer_ci(na, nb, seed):
    return np.random.default_rng(seed).integers(-3, 4, size=(na, nb)).astype(np.float64)


def normal_ci(na, nb, seed):
    return np.random.default_rng(seed).standard_normal((na, nb))


@pytest.mark.parametrize("norb,nelec", SHAPES + [LARGEST])
def test_signed_permutation_bit_for_bit(norb, nelec):
    p = problem(norb, nelec)
    u, perm, sign = signed_permutation(norb, seed=10 * norb + nelec[0])
    c = integer_ci(p.na, p.nb, seed=norb)
    assert np.array_equal(p.rotate(c, u), permuted_by_strings(c, norb, nelec, perm, sign))
    u2, perm2, sign2 = signed_permutation(norb, seed=10 * norb + nelec[0] + 500)
    assert np.array_equal(p.rotate(c, u, u2), permuted_by_strings(c, norb, nelec, perm, sign, perm2, sign2))
    if (norb, nelec) == LARGEST:                                            # least grant: 202 panels of T_a
        assert p.least < p.full // 50
        assert np.array_equal(p.rotate(c, u, u2, ws_bytes=p.least),
                              permuted_by_strings(c, norb, nelec, perm, sign, perm2, sign2))


def bound(c, norb, nelec, na, nb, amplification=1.0):
    # k is the electron count, also where the complement route factors minors of the smaller order norb - k: there the
    # term stands for the host inverse and det(u) as well, whose error (a 16 x 16 Gauss-Jordan) is not modelled apart.
    # That makes the bound loose at those shapes (8 * 15^3 at (16, (15, 1))); what pins the complement route down to
    # the bit is test_signed_permutation_bit_for_bit, which runs at every one of them.
    k = max(nelec)
    return (2.0 * 2.0 ** -53 * np.linalg.norm(c) * ((na + nb) + (np.sqrt(na) + np.sqrt(nb)) * 8.0 * k ** 3)
            * max(1.0, amplification))


@functools.lru_cache(maxsize=None)
def host_minors(kind, norb, k, seed):
    u = random_orthogonal(norb, seed) if kind == "orthogonal" else general_u(norb, seed)
    return u, minor_matrix(u, norb, k)


def rounded_case(norb, nelec, kind, pair):
    p = problem(norb, nelec)
    c = normal_ci(p.na, p.nb, seed=7 * norb + nelec[1])
    ua, Ta = host_minors(kind, norb, nelec[0], 100 + norb)
    ub, Tb = host_minors(kind, norb, nelec[1], (300 if pair else 100) + norb)
    want = Ta.T @ c @ Tb
    got = p.rotate(c, ua, ub if pair else None)
    amp = 1.0 if kind == "orthogonal" else np.linalg.norm(Ta, 2) * np.linalg.norm(Tb, 2)
    allowed = bound(c, norb, nelec, p.na, p.nb, amp)
    err = np.abs(got - want).max()
    print(f"rotate {kind}{' pair' if pair else ''} norb={norb} nelec={nelec}: max error {err:.3e}, allowed {allowed:.3e} "
          f"({err / allowed:.4f} of it), amplification {amp:.3g}")
    assert err <= allowed


@pytest.mark.parametrize("norb,nelec", SHAPES)
def test_random_orthogonal_u_within_the_rounding_bound(norb, nelec):
    rounded_case(norb, nelec, "orthogonal", pair=False)


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("norb,nelec", SHAPES)
def test_general_u_within_the_rounding_bound(norb, nelec, pair):
    rounded_case(norb, nelec, "general", pair)


@pytest.mark.parametrize("norb,nelec", [(12, (6, 6)), (10, (8, 2))])
def test_every_grant_gives_the_same_bits(norb, nelec):
    p = problem(norb, nelec)
    c = normal_ci(p.na, p.nb, seed=3)
    ua, ub = random_orthogonal(norb, 1), general_u(norb, 2)
    sizes = sorted(b for b in {p.least, p.least + 1, (p.least + p.full) // 2, p.full - 1, p.full, p.full + 4096}
                   if b >= p.least)
    if (norb, nelec) == (12, (6, 6)):                     # two panels per T; at (10, (8, 2)) the two grants coincide
        assert p.least < p.full and len(sizes) == 6
    for u2 in (None, ub):
        ref = p.rotate(c, ua, u2, ws_bytes=p.full)
        assert np.isfinite(ref).all()
        for ws_bytes in sizes:
            assert np.array_equal(p.rotate(c, ua, u2, ws_bytes=ws_bytes), ref), ws_bytes
    # one matrix for both spins, given once or twice
    assert np.array_equal(p.rotate(c, ua, ua.copy()), p.rotate(c, ua))


def test_refusals_launch_nothing():
    _, lib, _ = library()
    p = problem(10, (9, 1))
    c = normal_ci(p.na, p.nb, seed=5)
    u = random_orthogonal(10, 9)
    p.rotate(c, u)                                  # leaves the record of a call that ran
    singular = u.copy()
    singular[:, 3] = singular[:, 7]
    cases = {"norb = 17": dict(ua=u, norb=17),
             "a wrong na": dict(ua=u, na=p.na + 1),
             "out == c": dict(ua=u, out="alias"),
             "a grant one byte short": dict(ua=u, ws_bytes=p.least - 1),
             "singular u with nine electrons": dict(ua=singular)}
    for name, kw in cases.items():
        ws_bytes = kw.pop("ws_bytes", p.full)
        ua = kw.pop("ua")
        rc, out, after = p.call(c, ua, None, ws_bytes, **kw)
        msg = lib.evc_last_error().decode()
        assert rc < 0 and msg.startswith("evc_fci_rotate"), (name, rc, msg)
        assert np.isnan(out).all() and np.array_equal(after, c), name        # nothing ran
        assert p.record() == p.want_record, name                              # ... and nothing was noted
        print(f"refused {name}: {msg}")
    assert lib.evc_fci_rotate_workspace_bytes(17, 1, 1, 17, 17, 0) == 0
    assert lib.evc_fci_rotate_workspace_bytes(10, 9, 1, 11, 10, 1) == 0
    # the same singular u is no obstacle to minors that are computed directly
    q = problem(10, (8, 2))
    cq = normal_ci(q.na, q.nb, seed=6)
    assert np.isfinite(q.rotate(cq, singular)).all()


def test_device_fci_transform_ci_takes_arrays_tensors_and_pairs():
    from evcont_amd._lib import EvcontHipError
    from evcont_amd.fci_device import DeviceFCI
    norb, nelec = 6, (3, 2)
    p = problem(norb, nelec)
    c = normal_ci(p.na, p.nb, seed=8)
    ua, ub = random_orthogonal(norb, 3), general_u(norb, 4)
    s = DeviceFCI()
    direct = p.rotate(c, ua, ub)
    got = s.transform_ci(c, nelec, (ua, ub))
    assert isinstance(got, np.ndarray) and got.shape == (p.na, p.nb) and np.array_equal(got, direct)
    assert np.array_equal(s.transform_ci(torch.from_numpy(c), nelec, (ua, ub)), direct)
    assert np.array_equal(s.transform_ci(c, nelec, ua), p.rotate(c, ua))
    with pytest.raises(EvcontHipError):
        s.transform_ci(c, nelec, ua[:, :5])


# ---- physics -------------------------------------------------------------------------------------------------------
def both_bases(mol):
    from evcont_amd.electron_integral_utils import get_basis, get_integrals
    oao, can = get_basis(mol), get_basis(mol, "canonical")
    u = np.einsum("ji,jk,kl->il", can, mol.S, oao)
    return get_integrals(mol, oao), get_integrals(mol, can), u


@pytest.mark.parametrize("natm", [6, 8])
def test_canonical_solve_rotated_is_the_oao_solve(natm):
    """H6: the dense host route; H8: the device Davidson.  At both sizes the Davidson solver needs fewer sigma vectors
    in the canonical basis."""
    from evcont_amd.fci_device import DeviceFCI
    mol = hydrogen_chain(natm, 1.8, need_grad=False)
    (h1o, h2o), (h1c, h2c), u = both_bases(mol)
    nsigma = {}
    dav = {}
    for name, (h1, h2) in (("OAO", (h1o, h2o)), ("canonical", (h1c, h2c))):
        s = DeviceFCI(eigensolver="davidson")
        dav[name] = s.kernel(h1, h2, natm, mol.nelec)
        assert s.converged is True
        nsigma[name] = s.davidson_info["nsigma"]
    if natm == 6:
        dense = DeviceFCI()
        assert dense.dense_limit >= 400
        (e_o, c_o), (e_c, c_c) = dense.kernel(h1o, h2o, natm, mol.nelec), dense.kernel(h1c, h2c, natm, mol.nelec)
        limit = 1e-12
    else:
        (e_o, c_o), (e_c, c_c) = dav["OAO"], dav["canonical"]
        limit = 1e-8                                       # a residual of 1e-10 over the gap
    rotated = DeviceFCI().transform_ci(c_c, mol.nelec, u)
    defect = 1.0 - abs(np.vdot(c_o, rotated))
    print(f"H{natm}: |dE|={abs(e_o - e_c):.2e}, 1 - |<c_OAO|T c_can>| = {defect:.2e}, sigma vectors {nsigma}")
    assert abs(e_o - e_c) <= 1e-10
    assert defect <= limit
    assert nsigma["canonical"] < nsigma["OAO"], nsigma


def test_container_grown_in_the_canonical_basis_on_the_device():
    from evcont_amd.FCI_EVCont import FCI_EVCont_obj
    from evcont_amd.ab_initio_gradients_loewdin import get_energy_with_grad
    from evcont_amd.fci_device import DeviceFCI
    can = FCI_EVCont_obj(cisolver=DeviceFCI(eigensolver="davidson"), cibasis="canonical", nroots=2, roots_train=[0, 1])
    oao = FCI_EVCont_obj(cisolver=DeviceFCI(eigensolver="davidson"), cibasis="OAO", nroots=2, roots_train=[0, 1])
    for d in (1.5, 2.0, 2.8):
        can.append_to_rdms(hydrogen_chain(6, d, need_grad=False))
        oao.append_to_rdms(hydrogen_chain(6, d, need_grad=False))
    assert can.cisolver.converged is True and len(can.fcivecs) == 6
    m = hydrogen_chain(6, 1.8)
    Ec, gc = get_energy_with_grad(m, can.one_rdm, can.two_rdm, can.overlap)
    Eo, go = get_energy_with_grad(m, oao.one_rdm, oao.two_rdm, oao.overlap)
    print(f"H6 container, canonical against OAO: |dE|={abs(Ec - Eo):.2e} |dg|={np.abs(gc - go).max():.2e}")
    assert abs(Ec - Eo) <= 1e-9 and np.abs(gc - go).max() <= 1e-8
    # the prediction does not depend on the signs of the training states: flip states 1 and 4
    s = np.ones(6)
    s[[1, 4]] = -1.0
    ss = s[:, None] * s[None, :]
    Ef, gf = get_energy_with_grad(m, ss[:, :, None, None] * can.one_rdm, ss[:, :, None, None, None, None] * can.two_rdm,
                                  ss * can.overlap)
    assert abs(Ef - Eo) <= 1e-9 and np.abs(gf - go).max() <= 1e-8
