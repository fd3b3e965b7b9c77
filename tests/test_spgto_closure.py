"""Host-side closure for csrc/spgto.hip (device AO integrals of s and p Gaussian shells), modelled on
tests/test_sgto_closure.py: the calls are declared in the header, bound in ``_lib`` and exported, the file is built,
every kernel it defines is launched through ``gto_launch`` of csrc/gto_shells.hpp (by the shared host templates, from
the kernel list of the route description ``SpRoute``) and through nothing else, the calls add neither a profile
stage nor an ABI version, sgto.hip keeps its four kernels, and every refusal happens on the host."""
import ctypes as C
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "evcont_amd", "csrc")
CALLS = ("evc_spgto_workspace_bytes", "evc_spgto_integrals_batch", "evc_spgto_dipole_batch")
KERNELS = {"spgto_pair_kernel", "spgto_one_kernel", "spgto_nuc_kernel", "spgto_two_kernel", "spgto_dipole_kernel"}


def source(name="spgto.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_calls_are_declared_bound_and_built():
    from evcont_amd import _lib, build
    build.build()
    lib = _lib.load()
    with open(os.path.join(REPO, "include", "evcont_hip.h")) as f:
        hdr = f.read()
    for name in CALLS:
        assert f"{name}(" in hdr, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name in hdr[:hdr.index("#define EVC_LAYOUT_FULL6")], "listed as additive in the ABI comment"
    # the outputs are the struct of evc_sgto_integrals_batch, unchanged
    assert "const evc_sgto_outputs *out" in hdr[hdr.index("int evc_spgto_integrals_batch("):]
    assert C.sizeof(_lib.SgtoOutputs) == 8 * 8
    assert "spgto.hip" in build.SOURCES and "sgto.hip" in build.SOURCES


def test_every_kernel_is_launched_through_gto_launch():
    src, core = source(), source("gto_shells.hpp")
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src))
    # the launches are in the host templates of the shared header, which take their kernels from the route description
    route = src[src.index("struct SpRoute {"):]
    listed = dict(re.findall(r"\b(k\w+) = (\w+_kernel)\b", route[:route.index("\n};\n")]))
    passed = [re.findall(r"\bR::(k\w+)", first) for first in re.findall(r"(?<!void )\bgto_launch\(([^,]*),", core)]
    assert all(passed) and {m for ms in passed for m in ms} == set(listed), (passed, listed)
    launched = set(listed.values())
    assert defined == launched == KERNELS, sorted(defined ^ launched)
    assert "<<<" not in src and "hipLaunchKernelGGL" not in src and "hipLaunchKernel(" not in src
    assert "<<<" not in core and "hipLaunchKernelGGL" not in core
    assert len(re.findall(r"\bhipLaunchKernel\(", core)) == 1
    helper = core[core.index("static void gto_launch("):]
    assert "hipLaunchKernel(" in helper[:helper.index("\n}\n")]
    assert "atomic" not in src.lower()


def test_no_new_profile_stage_no_new_abi_version_and_sgto_as_it_was():
    from evcont_amd import _lib
    assert re.search(r"constexpr int kProfStages = 14;", source("pipeline.hpp"))
    with open(os.path.join(REPO, "include", "evcont_hip.h")) as f:
        assert re.search(r"#define\s+EVC_ABI_VERSION\s+10\b", f.read())
    assert _lib.ABI_VERSION == 10
    assert "note_kernel" not in source() and "EVC_PROF_" not in source()
    assert set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", source("sgto.hip"))) == \
        {"sgto_pair_kernel", "sgto_one_kernel", "sgto_nuc_kernel", "sgto_two_kernel"}


def test_refusals_need_no_device():
    """Every refused argument is caught on the host, before anything is launched: rc < 0 and a message that names the
    function."""
    from evcont_amd import _lib, build
    build.build()
    lib = _lib.load()
    i32 = lambda *v: np.array(v, dtype=np.int32)
    f64 = lambda *v: np.array(v, dtype=np.float64)
    # water-like: O with s(3), s(3), p(3); two H with s(3)
    sa, sl, so = i32(0, 0, 0, 1, 2), i32(0, 0, 1, 0, 0), i32(0, 3, 6, 9, 12, 15)
    ex, co = f64(*([3.4, 0.6, 0.2] * 5)), f64(*([0.2, 0.5, 0.4] * 5))
    out = _lib.SgtoOutputs(*([256] * 8))
    need = lib.evc_spgto_workspace_bytes(3, 5, 15, 7, 2)
    assert need >= 2 * 15 * 15 * 8
    good = dict(natm=3, nshell=5, count=2, coords=256, charges=256, sa=sa, sl=sl, so=so, ex=ex, co=co,
                out=C.byref(out), flags=0, ws=256, ws_bytes=need)
    ptr = lambda a: None if a is None else a.ctypes.data

    def call(**kw):
        a = dict(good, **kw)
        return lib.evc_spgto_integrals_batch(a["natm"], a["nshell"], a["count"], a["coords"], a["charges"], ptr(a["sa"]),
                                             ptr(a["sl"]), ptr(a["so"]), ptr(a["ex"]), ptr(a["co"]), a["out"],
                                             a["flags"], a["ws"], a["ws_bytes"], None)

    no_grad = _lib.SgtoOutputs(256, 256, 256, 256, None, None, None, None)
    no_eri = _lib.SgtoOutputs(256, 256, 256, None, 256, 256, 256, 256)
    many = 17                                     # 17 shells of 8 primitives: 136 primitives
    nine = i32(0, 9, 10, 11, 12, 13)              # a shell of 9 primitives
    wide = 22                                     # 22 p shells: 66 functions
    cases = (
        (dict(natm=0), b"natm"), (dict(natm=65), b"natm"), (dict(nshell=0), b"nshell"), (dict(nshell=65), b"nshell"),
        (dict(count=0), b"count"), (dict(count=65536), b"count"),
        (dict(coords=None), b"null"), (dict(charges=None), b"null"), (dict(sa=None), b"null"), (dict(sl=None), b"null"),
        (dict(so=None), b"null"), (dict(ex=None), b"null"), (dict(co=None), b"null"), (dict(out=None), b"null"),
        (dict(ws=None), b"null"), (dict(out=C.byref(no_eri)), b"null"), (dict(out=C.byref(no_grad)), b"null"),
        (dict(sl=i32(0, 0, 2, 0, 0)), b"l=2"), (dict(sl=i32(0, -1, 1, 0, 0)), b"l=-1"),
        (dict(sa=i32(0, 0, 0, 1, 3)), b"shell_atom"), (dict(sa=i32(0, 0, 0, -1, 2)), b"shell_atom"),
        (dict(sa=i32(0, 1, 0, 1, 2)), b"ascending"),
        (dict(so=i32(1, 3, 6, 9, 12, 15)), b"shell_prim_offset"), (dict(so=i32(0, 3, 3, 9, 12, 15)), b"primitives"),
        (dict(so=nine), b"primitives"),
        (dict(nshell=many, natm=many, sa=i32(*range(many)), sl=i32(*([0] * many)), so=i32(*range(0, 8 * many + 1, 8)),
              ex=f64(*([1.0] * 8 * many)), co=f64(*([1.0] * 8 * many))), b"primitives"),
        (dict(nshell=wide, natm=wide, sa=i32(*range(wide)), sl=i32(*([1] * wide)), so=i32(*range(wide + 1)),
              ex=f64(*([1.0] * wide)), co=f64(*([1.0] * wide))), b"nao"),
        (dict(ex=f64(*([3.4, 0.0, 0.2] * 5))), b"exponent"), (dict(ex=f64(*([3.4, -1.0, 0.2] * 5))), b"exponent"),
        (dict(flags=2), b"flags"), (dict(flags=64), b"flags"),
        (dict(ws_bytes=need - 1), b"workspace"), (dict(ws=264), b"aligned"),
    )
    for kw, word in cases:
        assert call(**kw) < 0, kw
        msg = lib.evc_last_error()
        assert word in msg and b"evc_spgto_integrals_batch" in msg, (kw, msg)
    assert call(flags=_lib.FLAG_ENERGY_ONLY, out=C.byref(no_grad), natm=0) < 0       # (no_grad is fine with the flag)
    for args in ((0, 5, 15, 7, 1), (65, 5, 15, 7, 1), (3, 0, 15, 7, 1), (3, 65, 65, 65, 1), (3, 5, 129, 7, 1),
                 (3, 5, 15, 65, 1), (3, 5, 15, 7, 0), (3, 5, 15, 7, 65536)):
        assert lib.evc_spgto_workspace_bytes(*args) == 0, args
        assert b"evc_spgto_workspace_bytes" in lib.evc_last_error()
    o = f64(0.0, 0.0, 0.0)
    dip = lambda **kw: lib.evc_spgto_dipole_batch(
        kw.get("natm", 3), 5, 2, kw.get("coords", 256), ptr(kw.get("sa", sa)), ptr(sl), ptr(so), ptr(kw.get("ex", ex)),
        ptr(co), kw.get("origin", o.ctypes.data), kw.get("dip", 256), None)
    for kw, word in ((dict(natm=65), b"natm"), (dict(coords=None), b"null"), (dict(origin=None), b"null"),
                     (dict(dip=None), b"null"), (dict(sa=i32(0, 1, 0, 1, 2)), b"ascending"),
                     (dict(ex=f64(*([3.4, 0.0, 0.2] * 5))), b"exponent")):
        assert dip(**kw) < 0, kw
        assert word in lib.evc_last_error() and b"evc_spgto_dipole_batch" in lib.evc_last_error(), kw
