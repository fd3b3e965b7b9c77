"""Host-side tests of the block row call (include/evcont_hip.h: evc_fci_trdm_rows_block,
evc_fci_rows_block_workspace_bytes): both symbols are declared, exported and bound under ABI 10 with 14 profile stages,
fci.hip still has one row routine and one product launch site, the workspace size is that of the single call for one
bra and does not decrease with the bras, and every refusal comes before any launch (fake pointers, no device), with the
function's name in front.  tests/test_gpu_fci_rows_block.py runs the call."""
import ctypes as C
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("evc_fci_trdm_rows_block", "evc_fci_rows_block_workspace_bytes")


def read(*parts):
    with open(os.path.join(REPO, *parts)) as f:
        return f.read()


def library():
    from evcont_amd import _lib, build
    build.build()
    return _lib, _lib.load()


def test_declared_exported_and_bound():
    _lib, lib = library()
    hdr = read("include", "evcont_hip.h")
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"^(?:int|size_t)\s+" + name + r"\(", hdr, re.M), name
        assert len(re.findall(r"\b" + name + r"\b", hdr.split("#define EVC_LAYOUT_FULL6")[0])) == 1, name   # ABI comment
        assert getattr(lib, name) is not None
    assert _lib.ABI_VERSION == 10 and lib.evc_abi_version() == 10
    assert re.search(r"constexpr int kProfStages = 14;", read("evcont_amd", "csrc", "pipeline.hpp"))
    assert _lib.FCI_PROF_PACK == 13 and _lib.FCI_PROF_STAGES["fci_trdm"] == 9


def test_one_row_routine_and_one_product_launch_site():
    fci = read("evcont_amd", "csrc", "fci.hip")
    assert len(re.findall(r"\bstatic int fci_trdm_rows_run\(", fci)) == 1
    assert len(re.findall(r"\blaunch_trdm\(trt", fci)) == 1
    for name in ("evc_fci_trdm_rows", "evc_fci_trdm_rows_packed", "evc_fci_trdm_rows_block"):
        start = fci.index(f'extern "C" int {name}(')
        body = fci[start:fci.index('extern "C"', start + 10)]
        assert len(re.findall(r"\bfci_trdm_rows_run\(", body)) == 1, name
        assert "<<<" not in body and "launch_trdm(" not in body, name
    kernels = set(re.findall(r"__global__[^;{]*?\bvoid\s+(fci_trdm\w+)\s*\(", fci))
    assert kernels == {"fci_trdm_kernel", "fci_trdm_reduce1_kernel", "fci_trdm_reduce2_kernel"}, kernels
    notes = re.findall(r'note_kernel\(EVC_PROF_FCI_TRDM,\s*((?:"[^"]*"\s*)+)', fci)
    fmts = sorted("".join(re.findall(r'"([^"]*)"', n)) for n in notes)
    assert len(fmts) == 2 and fmts[1] == fmts[0] + " bras=%d", fmts


def test_workspace_bytes():
    _, lib = library()
    size = lib.evc_fci_rows_block_workspace_bytes
    for norb, na, nb in ((2, 2, 2), (6, 20, 20), (9, 36, 9), (10, 252, 252), (13, 78, 13), (16, 16, 16)):
        for minimal in (0, 1):
            one = size(norb, na, nb, 1, minimal)
            assert one == lib.evc_fci_workspace_bytes(norb, na, nb, minimal) > 0
            prev = one
            for nbras in range(2, 17):
                cur = size(norb, na, nb, nbras, minimal)
                assert cur >= prev > 0, (norb, nbras, minimal)
                prev = cur
            assert size(norb, na, nb, 16, 0) > size(norb, na, nb, 1, 0)
            assert size(norb, na, nb, 16, 0) >= size(norb, na, nb, 16, 1)
    for bad in ((0, 4, 4, 1), (17, 4, 4, 1), (4, 0, 4, 1), (4, 4, 12871, 1), (4, 4, 4, 0), (4, 4, 4, 17), (4, 4, 4, -1)):
        assert size(*bad, 0) == 0 and size(*bad, 1) == 0, bad


def test_refusals_need_no_device():
    """Every refused argument is caught on the host, before anything is launched: rc < 0 and a message."""
    _, lib = library()
    norb, na, nb = 4, 6, 6
    dim, n2 = na * nb, norb * norb
    full = lib.evc_fci_rows_block_workspace_bytes(norb, na, nb, 3, 0)
    least = lib.evc_fci_rows_block_workspace_bytes(norb, na, nb, 3, 1)
    vec = lambda i: (1 << 24) + i * 8 * dim                # fake device addresses, one vector apart
    good = dict(norb=norb, na=na, nb=nb, ta=4096, tb=8192, bras=[vec(2), vec(3), vec(4)], nbras=3,
                kets=[vec(0), vec(1), vec(2), vec(3), vec(4)], counts=[3, 4, 5], ovlp=1 << 28, dm1=1 << 29, dm2=1 << 30,
                ws=1 << 32, ws_bytes=full)
    total = sum(good["counts"])

    def call(**kw):
        a = dict(good, **kw)
        bras = None if a["bras"] is None else (C.c_void_p * len(a["bras"]))(*a["bras"])
        kets = None if a["kets"] is None else (C.c_void_p * len(a["kets"]))(*a["kets"])
        counts = None if a["counts"] is None else (C.c_int * len(a["counts"]))(*a["counts"])
        return lib.evc_fci_trdm_rows_block(a["norb"], a["na"], a["nb"], a["ta"], a["tb"], bras, a["nbras"], kets, counts,
                                           a["ovlp"], a["dm1"], a["dm2"], a["ws"], a["ws_bytes"], None)

    last = vec(4)
    cases = [
        (dict(norb=0), b"norb"), (dict(norb=17), b"norb"), (dict(na=0), b"na="), (dict(nb=12871), b"nb="),
        (dict(ta=None), b"null"), (dict(tb=None), b"null"), (dict(bras=None), b"null"), (dict(kets=None), b"null"),
        (dict(counts=None), b"null"), (dict(ovlp=None), b"null"), (dict(dm1=None), b"null"), (dict(dm2=None), b"null"),
        (dict(ws=None), b"null"),
        (dict(bras=[vec(2), None, vec(4)]), b"bras[1] is null"),
        (dict(kets=[vec(0), vec(1), vec(2), None, vec(4)]), b"kets[3] is null"),
        (dict(nbras=0), b"nbras=0"), (dict(nbras=17), b"nbras=17"), (dict(nbras=-1), b"nbras=-1"),
        (dict(counts=[0, 4, 5]), b"nkets_of[0]=0"), (dict(counts=[3, 4, 4097]), b"nkets_of[2]=4097"),
        (dict(counts=[3, -1, 5]), b"nkets_of[1]=-1"),
        (dict(counts=[4, 3, 5]), b"must not decrease"), (dict(counts=[3, 5, 4]), b"must not decrease"),
        (dict(ws=(1 << 32) + 8), b"aligned"),
        (dict(ws_bytes=4096), b"workspace of"), (dict(ws_bytes=0), b"workspace of"),
        # an output that shares a byte with an input vector: its first, its last, from below and from above
        (dict(dm2=vec(0)), b"dm2 overlaps"),
        (dict(dm2=last + 8 * (dim - 1)), b"dm2 overlaps"),
        (dict(dm2=vec(0) - 8 * (total * n2 * n2 - 1)), b"dm2 overlaps kets[0]"),
        (dict(dm1=vec(1)), b"dm1 overlaps"), (dict(dm1=vec(0) - 8 * (total * n2 - 1)), b"dm1 overlaps kets[0]"),
        (dict(ovlp=vec(3) + 8), b"ovlp overlaps"), (dict(ovlp=vec(0) - 8 * (total - 1)), b"ovlp overlaps kets[0]"),
        (dict(bras=[vec(2), vec(3), 1 << 29]), b"dm1 overlaps bras[2]"),
    ]
    for kw, word in cases:
        assert call(**kw) < 0, kw
        msg = lib.evc_last_error()
        assert msg.startswith(b"evc_fci_trdm_rows_block") and word in msg, (kw, msg)
    assert 4096 < lib.evc_fci_workspace_bytes(norb, na, nb, 1) <= least <= full
