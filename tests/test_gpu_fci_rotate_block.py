"""GPU tests of ``evc_fci_rotate_block`` (csrc/fci_rotate.hip): several CI vectors under one orbital transformation, the
panels of the minors formed once.  Vector v of a block call must have the bits ``evc_fci_rotate`` gives on that vector,
for the resident and the least workspace, from run to run; the record of stage 12 names the number of vectors; every
refusal comes before a launch.

Shapes: (4,(2,2)); (5,(3,2)), unequal spins; (8,(4,4)), 70 strings = a ragged 64-tile; (10,(9,1)), the complement route;
(12,(6,6)), two panels per T, where the least grant is the smaller one."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_fci_rotate_host import general_u, permuted_by_strings, random_orthogonal, signed_permutation
from test_gpu_fci_abi import Fenced
from test_gpu_fci_rotate import Problem, integer_ci, normal_ci

pytestmark = pytest.mark.gpu

SHAPES = [(4, (2, 2)), (5, (3, 2)), (8, (4, 4)), (10, (9, 1)), (12, (6, 6))]
NVEC = (1, 2, 3, 5)


@functools.lru_cache(maxsize=None)
def problem(norb, nelec):
    return Problem(norb, nelec)


def grants(p, nvec):
    least = p.lib.evc_fci_rotate_block_workspace_bytes(p.norb, p.nelec[0], p.nelec[1], p.na, p.nb, nvec, 1)
    full = p.lib.evc_fci_rotate_block_workspace_bytes(p.norb, p.nelec[0], p.nelec[1], p.na, p.nb, nvec, 0)
    assert 0 < least <= full
    return least, full


def block(p, cs, ua, ub, ws_bytes, nvec=None, out="fresh", null=None, na=None):
    """rc, the outputs (nvec, na, nb) from NaN-filled targets, the inputs as they are afterwards"""
    ua = np.ascontiguousarray(ua, dtype=np.float64)
    ub = ua if ub is None else np.ascontiguousarray(ub, dtype=np.float64)
    dcs = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.float64).reshape(-1)).to(p.dev) for c in cs]
    ws = Fenced(max(ws_bytes, 16), p.dev, front=False)
    res = [Fenced(8 * p.na * p.nb, p.dev) for _ in cs]
    n = len(cs)
    cp = (C.c_void_p * n)(*[t.data_ptr() for t in dcs])
    outs = [r.ptr for r in res]
    if out == "alias":                          # the last output is the first input
        outs[-1] = dcs[0].data_ptr()
    elif out == "twice" and n > 1:
        outs[-1] = outs[0]
    if null == "vector":
        outs[-1] = None
    op = (C.c_void_p * n)(*outs)
    rc = p.lib.evc_fci_rotate_block(p.norb, p.nelec[0], p.nelec[1], p.na if na is None else na, p.nb, p.sa.data_ptr(),
                                    p.sb.data_ptr(), ua.ctypes.data, ub.ctypes.data, n if nvec is None else nvec,
                                    None if null == "c" else cp, op, ws.ptr, ws_bytes, None)
    torch.cuda.synchronize()
    assert ws.fences_intact() and all(r.fences_intact() for r in res), ws_bytes
    return (rc, np.stack([r.doubles().reshape(p.na, p.nb) for r in res]),
            [t.cpu().numpy().reshape(p.na, p.nb) for t in dcs])


def singles(p, cs, ua, ub):
    return np.stack([p.rotate(c, ua, ub) for c in cs])


@pytest.mark.parametrize("norb,nelec", SHAPES)
def test_block_has_the_bits_of_the_single_call(norb, nelec):
    p = problem(norb, nelec)
    ua, ub = random_orthogonal(norb, 1), general_u(norb, 2)
    cs = [normal_ci(p.na, p.nb, seed=40 + v) for v in range(max(NVEC))]
    for u2 in (None, ub):                                   # one T for both spins where they agree, and u_a != u_b
        want = singles(p, cs, ua, u2)
        assert np.isfinite(want).all()
        for nvec in NVEC:
            least, full = grants(p, nvec)
            for ws_bytes in sorted({least, full}):
                rc, got, after = block(p, cs[:nvec], ua, u2, ws_bytes)
                p.check(rc, "evc_fci_rotate_block")
                assert np.array_equal(got, want[:nvec]), (nvec, ws_bytes)
                assert all(np.array_equal(a, c) for a, c in zip(after, cs))            # the inputs are not written
                assert p.record() == p.want_record + f" vecs={nvec}", p.record()
        rc, again, _ = block(p, cs[:3], ua, u2, grants(p, 3)[1])                        # run to run
        assert rc == 0 and np.array_equal(again, want[:3])
    if (norb, nelec) == (12, (6, 6)):
        assert grants(p, 3)[0] < grants(p, 3)[1]            # the least grant is the panelled form here
    # the single call's record is what it was
    p.rotate(cs[0], ua)
    assert p.record() == p.want_record


def test_more_vectors_than_one_product_launch_takes():
    p = problem(5, (3, 2))
    ua, ub = random_orthogonal(5, 3), general_u(5, 4)
    cs = [normal_ci(p.na, p.nb, seed=70 + v) for v in range(19)]               # 16 + 3
    rc, got, _ = block(p, cs, ua, ub, grants(p, 19)[0])
    p.check(rc, "evc_fci_rotate_block")
    assert p.record().endswith(" vecs=19")
    assert np.array_equal(got, singles(p, cs, ua, ub))


@pytest.mark.parametrize("norb,nelec", SHAPES)
def test_signed_permutation_of_integer_vectors_is_exact(norb, nelec):
    p = problem(norb, nelec)
    u, perm, sign = signed_permutation(norb, seed=10 * norb + nelec[0])
    u2, perm2, sign2 = signed_permutation(norb, seed=10 * norb + nelec[0] + 500)
    cs = [integer_ci(p.na, p.nb, seed=norb + v) for v in range(3)]
    for ws_bytes in sorted(set(grants(p, 3))):
        rc, got, _ = block(p, cs, u, u2, ws_bytes)
        p.check(rc, "evc_fci_rotate_block")
        for v, c in enumerate(cs):
            assert np.array_equal(got[v], permuted_by_strings(c, norb, nelec, perm, sign, perm2, sign2)), v


def test_refusals_launch_nothing():
    p = problem(10, (9, 1))
    cs = [normal_ci(p.na, p.nb, seed=5 + v) for v in range(2)]
    u = random_orthogonal(10, 9)
    least, full = grants(p, 2)
    p.rotate(cs[0], u)                              # leaves the record of a call that ran
    singular = u.copy()
    singular[:, 3] = singular[:, 7]
    cases = {"nvec = 0": dict(nvec=0),
             "a null array": dict(null="c"),
             "a null vector": dict(null="vector"),
             "an output that is an input": dict(out="alias"),
             "one output twice": dict(out="twice"),
             "a grant one byte short": dict(ws_bytes=least - 1),
             "a wrong na": dict(na=p.na + 1),
             "singular u with nine electrons": dict(ua=singular)}
    for name, kw in cases.items():
        ws_bytes = kw.pop("ws_bytes", full)
        ua = kw.pop("ua", u)
        rc, out, after = block(p, cs, ua, None, ws_bytes, **kw)
        msg = p.lib.evc_last_error().decode()
        assert rc < 0 and msg.startswith("evc_fci_rotate_block:"), (name, rc, msg)
        assert np.isnan(out).all() and all(np.array_equal(a, c) for a, c in zip(after, cs)), name       # nothing ran
        assert p.record() == p.want_record, name                                                       # nothing noted
        print(f"refused {name}: {msg}")
    size = p.lib.evc_fci_rotate_block_workspace_bytes
    assert size(10, 9, 1, p.na, p.nb, 0, 0) == 0 and size(17, 1, 1, 17, 17, 2, 0) == 0
    assert size(10, 9, 1, p.na + 1, p.nb, 2, 1) == 0
    # one vector: the sizes of the single call
    assert size(10, 9, 1, p.na, p.nb, 1, 0) == p.full and size(10, 9, 1, p.na, p.nb, 1, 1) == p.least


def test_device_fci_transform_ci_block():
    from evcont_amd.fci_device import DeviceFCI
    norb, nelec = 6, (3, 2)
    p = problem(norb, nelec)
    ua, ub = random_orthogonal(norb, 3), general_u(norb, 4)
    cs = [normal_ci(p.na, p.nb, seed=8 + v) for v in range(3)]
    s = DeviceFCI()
    got = s.transform_ci_block(cs, nelec, (ua, ub))
    assert len(got) == 3 and all(isinstance(g, np.ndarray) and g.shape == (p.na, p.nb) for g in got)
    for g, c in zip(got, cs):
        assert np.array_equal(g, s.transform_ci(c, nelec, (ua, ub)))
    outs, na, nb = s._rotate_block(cs[:2], nelec, ua)
    assert (na, nb) == (p.na, p.nb) and all(torch.is_tensor(o) and o.is_cuda for o in outs)
    assert np.array_equal(outs[1].cpu().numpy().reshape(na, nb), s.transform_ci(cs[1], nelec, ua))
