"""Host-side closure for csrc/spdfgto.hip (device AO integrals of s, p, d and f shells), modelled on
tests/test_spdgto_closure.py: the four calls are declared in the header, bound in ``_lib`` and exported, the file is
built, every kernel it defines is launched through ``gto_launch`` of csrc/gto_shells.hpp (by the shared host templates,
from the kernel list of the route description ``SpdfRoute``, and the dipole-gradient kernel from the file itself) and
through nothing else, the calls add neither a profile stage nor an ABI version, the older routes keep their kernels and
their refusal of l = 3, and every refusal happens on the host."""
import ctypes as C
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "evcont_amd", "csrc")
CALLS = ("evc_spdfgto_workspace_bytes", "evc_spdfgto_integrals_batch", "evc_spdfgto_dipole_batch",
         "evc_spdfgto_dipole_grad_batch")
KERNELS = {"spdfgto_pair_kernel", "spdfgto_one_kernel", "spdfgto_nuc_kernel", "spdfgto_two_kernel",
           "spdfgto_dipole_kernel", "spdfgto_dipole_grad_kernel"}
GLOBAL = r"__global__[^;{]*?\bvoid\s+(\w+)\s*\("


def source(name="spdfgto.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_calls_are_declared_bound_and_built():
    from evcont_amd import _lib, build
    build.build()
    lib = _lib.load()
    with open(os.path.join(REPO, "include", "evcont_hip.h")) as f:
        hdr = f.read()
    twins = {"evc_spdfgto_dipole_grad_batch": "evc_gto_dipole_grad_batch"}
    for name in CALLS:
        assert f"{name}(" in hdr, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name in hdr[:hdr.index("#define EVC_LAYOUT_FULL6")], "listed as additive in the ABI comment"
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[twins.get(name, name.replace("spdfgto", "spdgto"))], name
    assert "const evc_sgto_outputs *out" in hdr[hdr.index("int evc_spdfgto_integrals_batch("):]
    assert "spdfgto.hip" in build.SOURCES and "spdgto.hip" in build.SOURCES


def test_every_kernel_is_launched_through_gto_launch():
    src, core = source(), source("gto_shells.hpp")
    defined = set(re.findall(GLOBAL, src))
    route = src[src.index("struct SpdfRoute {"):]
    listed = dict(re.findall(r"\b(k\w+) = (\w+_kernel)\b", route[:route.index("\n};\n")]))
    spd = source("spdgto.hip")
    spd_route = spd[spd.index("struct SpdRoute {"):]
    assert set(listed) == set(dict(re.findall(r"\b(k\w+) = (\w+_kernel)\b", spd_route[:spd_route.index("\n};\n")])))
    passed = [re.findall(r"\bR::(k\w+)", first) for first in re.findall(r"(?<!void )\bgto_launch\(([^,]*),", core)]
    assert all(passed) and {m for ms in passed for m in ms} == set(listed), (passed, listed)
    # the dipole-gradient kernel: launched from the file itself, through the same helper
    own = re.findall(r"(?<!void )\bgto_launch\((\w+),", src)
    assert own == ["spdfgto_dipole_grad_kernel"]
    assert defined == set(listed.values()) | set(own) == KERNELS, sorted(defined ^ KERNELS)
    assert "<<<" not in src and "hipLaunchKernelGGL" not in src and "hipLaunchKernel(" not in src
    assert len(re.findall(r"\bhipLaunchKernel\(", core)) == 1
    assert "atomic" not in src.lower() and "mfma" not in src.lower().replace("no mfma", "")
    assert "static constexpr int kMaxL = 3;" in route and "static constexpr int kMaxL = 2;" in spd_route


def test_no_new_profile_stage_no_new_abi_version_and_the_other_files_as_they_were():
    from evcont_amd import _lib
    assert re.search(r"constexpr int kProfStages = 14;", source("pipeline.hpp"))
    with open(os.path.join(REPO, "include", "evcont_hip.h")) as f:
        assert re.search(r"#define\s+EVC_ABI_VERSION\s+10\b", f.read())
    assert _lib.ABI_VERSION == 10
    assert "note_kernel" not in source() and "EVC_PROF_" not in source()
    for name, stems in (("spdgto.hip", "pair one nuc two dipole"), ("spgto.hip", "pair one nuc two dipole"),
                        ("sgto.hip", "pair one nuc two")):
        route = name[:-4]
        assert set(re.findall(GLOBAL, source(name))) == {f"{route}_{s}_kernel" for s in stems.split()}, name
    assert set(re.findall(GLOBAL, source("field.hip"))) == {"field_sgrad_kernel", "field_grad_kernel", "field_fold_kernel"}
    core = source("gto_shells.hpp")
    assert "GTO_HD void spd_mono(" in core and "spdf_mono" not in core


def test_refusals_need_no_device():
    """Every refused argument is caught on the host, before anything is launched: rc < 0 and a message that names the
    function.  l = 3 passes the shape check, an f shell counts seven functions, and the l <= 2 calls still refuse it."""
    from evcont_amd import _lib, build
    build.build()
    lib = _lib.load()
    i32 = lambda *v: np.array(v, dtype=np.int32)
    f64 = lambda *v: np.array(v, dtype=np.float64)
    # O with s(3), p(3), f(3); two H with s(3)
    sa, sl, so = i32(0, 0, 0, 1, 2), i32(0, 1, 3, 0, 0), i32(0, 3, 6, 9, 12, 15)
    ex, co = f64(*([3.4, 0.6, 0.2] * 5)), f64(*([0.2, 0.5, 0.4] * 5))
    out = _lib.SgtoOutputs(*([256] * 8))
    need = lib.evc_spdfgto_workspace_bytes(3, 5, 15, 13, 2)
    assert need >= 2 * 15 * 15 * 8
    good = dict(natm=3, nshell=5, count=2, coords=256, charges=256, sa=sa, sl=sl, so=so, ex=ex, co=co,
                out=C.byref(out), flags=0, ws=256, ws_bytes=need)
    ptr = lambda a: None if a is None else a.ctypes.data

    def call(**kw):
        a = dict(good, **kw)
        return lib.evc_spdfgto_integrals_batch(a["natm"], a["nshell"], a["count"], a["coords"], a["charges"], ptr(a["sa"]),
                                               ptr(a["sl"]), ptr(a["so"]), ptr(a["ex"]), ptr(a["co"]), a["out"],
                                               a["flags"], a["ws"], a["ws_bytes"], None)

    no_grad = _lib.SgtoOutputs(256, 256, 256, 256, None, None, None, None)
    no_eri = _lib.SgtoOutputs(256, 256, 256, None, 256, 256, 256, 256)
    many = 17                                     # 17 shells of 8 primitives: 136 primitives
    nine = i32(0, 9, 10, 11, 12, 13)              # a shell of 9 primitives
    wide = 10                                     # ten f shells: 70 functions
    cases = (
        (dict(natm=0), b"natm"), (dict(natm=65), b"natm"), (dict(nshell=0), b"nshell"), (dict(nshell=65), b"nshell"),
        (dict(count=0), b"count"), (dict(count=65536), b"count"),
        (dict(coords=None), b"null"), (dict(charges=None), b"null"), (dict(sa=None), b"null"), (dict(sl=None), b"null"),
        (dict(so=None), b"null"), (dict(ex=None), b"null"), (dict(co=None), b"null"), (dict(out=None), b"null"),
        (dict(ws=None), b"null"), (dict(out=C.byref(no_eri)), b"null"), (dict(out=C.byref(no_grad)), b"null"),
        (dict(sl=i32(0, 0, 4, 0, 0)), b"l=4"), (dict(sl=i32(0, -1, 1, 0, 0)), b"l=-1"),
        (dict(sa=i32(0, 0, 0, 1, 3)), b"shell_atom"), (dict(sa=i32(0, 0, 0, -1, 2)), b"shell_atom"),
        (dict(sa=i32(0, 1, 0, 1, 2)), b"ascending"),
        (dict(so=i32(1, 3, 6, 9, 12, 15)), b"shell_prim_offset"), (dict(so=i32(0, 3, 3, 9, 12, 15)), b"primitives"),
        (dict(so=nine), b"primitives"),
        (dict(nshell=many, natm=many, sa=i32(*range(many)), sl=i32(*([0] * many)), so=i32(*range(0, 8 * many + 1, 8)),
              ex=f64(*([1.0] * 8 * many)), co=f64(*([1.0] * 8 * many))), b"primitives"),
        (dict(nshell=wide, natm=wide, sa=i32(*range(wide)), sl=i32(*([3] * wide)), so=i32(*range(wide + 1)),
              ex=f64(*([1.0] * wide)), co=f64(*([1.0] * wide))), b"nao=70"),
        (dict(ex=f64(*([3.4, 0.0, 0.2] * 5))), b"exponent"), (dict(ex=f64(*([3.4, -1.0, 0.2] * 5))), b"exponent"),
        (dict(flags=2), b"flags"), (dict(flags=64), b"flags"),
        (dict(ws_bytes=need - 1), b"workspace"), (dict(ws=264), b"aligned"),
    )
    for kw, word in cases:
        assert call(**kw) < 0, kw
        msg = lib.evc_last_error()
        assert word in msg and b"evc_spdfgto_integrals_batch" in msg, (kw, msg)
    # l = 3 is accepted by the shape check: with the f shell in place the first thing wrong is the workspace
    assert call(ws_bytes=need - 1) < 0 and b"l=" not in lib.evc_last_error()
    assert call(flags=_lib.FLAG_ENERGY_ONLY, out=C.byref(no_grad), natm=0) < 0       # (no_grad is fine with the flag)
    for args in ((0, 5, 15, 13, 1), (65, 5, 15, 13, 1), (3, 0, 15, 13, 1), (3, 65, 65, 65, 1), (3, 5, 129, 13, 1),
                 (3, 5, 15, 65, 1), (3, 5, 15, 36, 1), (3, 5, 15, 13, 0), (3, 5, 15, 13, 65536)):
        assert lib.evc_spdfgto_workspace_bytes(*args) == 0, args
        assert b"evc_spdfgto_workspace_bytes" in lib.evc_last_error()
    assert lib.evc_spdfgto_workspace_bytes(3, 5, 15, 35, 1) > 0                      # seven functions per shell
    assert lib.evc_spdgto_workspace_bytes(3, 5, 15, 26, 1) == 0                      # the s + p + d call: five
    o = f64(0.0, 0.0, 0.0)
    for fn in ("evc_spdfgto_dipole_batch", "evc_spdfgto_dipole_grad_batch"):
        dip = lambda **kw: getattr(lib, fn)(
            kw.get("natm", 3), 5, 2, kw.get("coords", 256), ptr(kw.get("sa", sa)), ptr(kw.get("sl", sl)), ptr(so),
            ptr(kw.get("ex", ex)), ptr(co), kw.get("origin", o.ctypes.data), kw.get("dip", 256), None)
        for kw, word in ((dict(natm=65), b"natm"), (dict(coords=None), b"null"), (dict(origin=None), b"null"),
                         (dict(dip=None), b"null"), (dict(sa=i32(0, 1, 0, 1, 2)), b"ascending"),
                         (dict(sl=i32(0, 1, 4, 0, 0)), b"l=4"), (dict(sl=i32(0, 1, -1, 0, 0)), b"l=-1"),
                         (dict(ex=f64(*([3.4, 0.0, 0.2] * 5))), b"exponent")):
            assert dip(**kw) < 0, (fn, kw)
            assert word in lib.evc_last_error() and fn.encode() in lib.evc_last_error(), (fn, kw)
    assert lib.evc_spdfgto_dipole_grad_batch(3, 5, 2, 260, ptr(sa), ptr(sl), ptr(so), ptr(ex), ptr(co), o.ctypes.data, 256,
                                             None) < 0 and b"misaligned" in lib.evc_last_error()
    # the routes for l <= 2 keep refusing the f shell
    assert lib.evc_spdgto_integrals_batch(3, 5, 2, 256, 256, ptr(sa), ptr(sl), ptr(so), ptr(ex), ptr(co), C.byref(out), 0,
                                          256, need, None) < 0 and b"l=3" in lib.evc_last_error()
    assert lib.evc_gto_dipole_grad_batch(3, 5, 2, 256, ptr(sa), ptr(sl), ptr(so), ptr(ex), ptr(co), o.ctypes.data, 256,
                                         None) < 0 and b"l=3" in lib.evc_last_error()
