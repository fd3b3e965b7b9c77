"""Host-side closure for csrc/cas_expand.hip, modelled on tests/test_fci_pack_closure.py: the file launches through
``cas_launch(kernel, ...)`` only, every kernel it defines is launched and named by ``evc_cas_expand_describe``, the three
entry points are declared, exported and bound, nothing pinned moved (ABI version, profile stages), and every invalid
argument is refused before any launch; tests/test_gpu_cas_expand.py holds the kernels to the description."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "evcont_amd", "csrc")
SYMBOLS = ("evc_cas_expand_workspace_bytes", "evc_cas_expand_rows", "evc_cas_expand_describe")
PREFIX = b"evc_cas_expand_rows"


def source(name="cas_expand.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.fixture(scope="module")
def lib():
    from evcont_amd import build, _lib
    build.build()
    return _lib.load()


def describe(lib, n, ncas, layout):
    buf = C.create_string_buffer(4096)
    k = lib.evc_cas_expand_describe(n, ncas, layout, buf, len(buf))
    assert 0 < k < len(buf)
    return buf.value.decode().splitlines()


def test_every_kernel_of_cas_expand_is_launched_through_the_wrapper():
    src = source()
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src))
    launched = set(re.findall(r"\bcas_launch\(\s*(\w+)\s*[<,]", src))
    assert defined == launched == {"cas_qa_kernel", "cas_step_kernel", "cas_core_kernel"}, sorted(defined ^ launched)
    assert "<<<" not in src and "hipLaunchKernelGGL" not in src
    assert len(re.findall(r"\bhipLaunchKernel\(", src)) == 1
    assert "note_fci_row_pack" not in src and "note_kernel" not in src       # no profile stage is touched
    assert len(re.findall(r"\blaunch_fci_row_pack\(", src)) == 1
    assert sorted(int(k) for k in re.findall(r"cas_step<(\d)>\(", src)) == [1, 2, 3, 4]


def test_symbols_are_declared_exported_and_bound(lib):
    from evcont_amd import _lib, build
    with open(os.path.join(REPO, "include", "evcont_hip.h")) as f:
        hdr = f.read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert re.search(rf"\b{name}\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)), name
    assert "cas_expand.hip" in build.SOURCES
    assert re.search(r"#define\s+EVC_ABI_VERSION\s+10\b", hdr) and _lib.ABI_VERSION == 10
    assert lib.evc_abi_version() == 10
    assert re.search(r"constexpr int kProfStages = 14;", source("pipeline.hpp"))


def test_describe_names_every_kernel(lib):
    from evcont_amd import _lib
    seen = set()
    for ncas, ks in ((1, 1), (4, 1), (5, 2), (8, 2), (9, 3), (13, 4), (16, 4)):
        for layout, pack in ((_lib.LAYOUT_FULL6, None), (_lib.LAYOUT_PACK2, 1), (_lib.LAYOUT_SYM8, 8)):
            lines = describe(lib, 17, ncas, layout)
            names = [ln.split()[0] for ln in lines]
            assert names == (["cas_qa_kernel"] + [f"cas_step_kernel<{ks}>"] * 4 + ["cas_core_kernel"]
                             + ([f"fci_row_pack_kernel<{pack}>"] if pack else [])), lines
            seen |= {re.sub(r"<.*", "", x) for x in names}
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", source()))
    assert defined <= seen
    # rows of the four steps: c^3, n c^2, n^2 c, n^3; the last step's grid covers its 16-row tiles four to a block
    lines = describe(lib, 30, 10, _lib.LAYOUT_FULL6)
    assert [int(re.search(r"rows=(\d+)", ln).group(1)) for ln in lines[1:5]] == [1000, 3000, 9000, 27000]
    assert "grid=422" in lines[4]
    buf = C.create_string_buffer(8)
    assert lib.evc_cas_expand_describe(30, 10, _lib.LAYOUT_FULL6, buf, 8) > 8 and len(buf.value) == 7     # truncated
    assert lib.evc_cas_expand_describe(30, 31, _lib.LAYOUT_FULL6, buf, 8) < 0
    assert lib.evc_cas_expand_describe(30, 10, 5, buf, 8) < 0
    assert lib.evc_cas_expand_describe(30, 10, 6, None, 8) < 0


def test_argument_validation_without_gpu(lib):
    from evcont_amd import _lib
    ws = lib.evc_cas_expand_workspace_bytes
    assert ws(6, 4, 3) >= 8 * (3 * 36 + 6 ** 3 * 4 + 36 * 16 + 6 ** 4)
    assert ws(64, 16, 512) > 8 * 64 ** 4
    for bad in ((65, 4, 1), (6, 17, 1), (20, 17, 1), (6, 0, 1), (3, 4, 1), (6, 4, 0), (6, 4, 513)):
        assert ws(*bad) == 0, bad
    n, ncas, nk = 6, 4, 2
    need = ws(n, ncas, nk)
    p = 256                                            # stands for a device pointer: nothing is launched
    full, pack2, sym8 = _lib.LAYOUT_FULL6, _lib.LAYOUT_PACK2, _lib.LAYOUT_SYM8

    def call(n=n, ncas=ncas, nk=nk, A=p, B=p, Qc=p, ov=p, d1=p, d2=p, dm1=p, layout=full, rows=p, ld=n ** 4, ws_ptr=p,
             wsb=need):
        return lib.evc_cas_expand_rows(n, ncas, nk, A, B, Qc, ov, d1, d2, dm1, layout, rows, ld, ws_ptr, wsb, None)

    refused = [dict(A=None), dict(B=None), dict(ov=None), dict(d1=None), dict(d2=None), dict(dm1=None), dict(rows=None),
               dict(ws_ptr=None),                                                          # null pointers
               dict(n=65, ld=65 ** 4), dict(ncas=17), dict(n=20, ncas=17, ld=20 ** 4), dict(n=3, ld=81),   # n, ncas
               dict(nk=0), dict(nk=513),
               dict(layout=5), dict(layout=3), dict(layout=0),                             # unknown layouts
               dict(ld=n ** 4 - 1),                                                        # dense row too short
               dict(layout=pack2, ld=670), dict(layout=sym8, ld=232), dict(layout=sym8, ld=224),   # 666 / 231 columns
               dict(A=264), dict(Qc=8), dict(rows=24), dict(ws_ptr=260),                   # alignment
               dict(wsb=need - 1), dict(wsb=0)]
    for kw in refused:
        assert call(**kw) < 0, kw
        assert lib.evc_last_error().startswith(PREFIX), (kw, lib.evc_last_error())
    assert b"null pointer" in (call(A=None), lib.evc_last_error())[1]
    assert b"layout=5" in (call(layout=5), lib.evc_last_error())[1]
    assert b"ld=670" in (call(layout=pack2, ld=670), lib.evc_last_error())[1]
    assert b"workspace" in (call(wsb=need - 1), lib.evc_last_error())[1]
