"""Host-side closure for csrc/sgto.hip (device AO integrals of s-Gaussian molecules), modelled on
tests/test_fci_pack_closure.py: the two calls are declared in the header, bound in ``_lib`` and exported, the file is
built, every kernel it defines is launched through ``gto_launch`` of csrc/gto_shells.hpp, the one place of the shell
routes that calls the runtime, and through nothing else, the call adds neither a profile stage nor an ABI version, and
every local header a source includes is a dependency of the build."""
import ctypes as C
import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "evcont_amd", "csrc")
CALLS = ("evc_sgto_workspace_bytes", "evc_sgto_integrals_batch")


def source(name="sgto.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_calls_are_declared_bound_and_built():
    from evcont_amd import _lib, build
    with open(os.path.join(REPO, "include", "evcont_hip.h")) as f:
        hdr = f.read()
    for name in CALLS:
        assert f"{name}(" in hdr, name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"typedef struct evc_sgto_outputs \{", hdr)
    fields = re.search(r"typedef struct evc_sgto_outputs \{(.*?)\} evc_sgto_outputs;", hdr, re.S).group(1)
    assert re.findall(r"double \*(\w+);", fields) == [f[0] for f in _lib.SgtoOutputs._fields_]
    assert C.sizeof(_lib.SgtoOutputs) == 8 * 8
    assert "sgto.hip" in build.SOURCES
    # an edit to a header rebuilds what includes it: every local header named in csrc is in build.HEADERS
    known = {os.path.normpath(os.path.join(CSRC, h)) for h in build.HEADERS}
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")):
        with open(path) as f:
            for inc in re.findall(r'(?m)^\s*#\s*include\s+"([^"]+)"', f.read()):
                assert os.path.normpath(os.path.join(CSRC, inc)) in known, (os.path.basename(path), inc)


def test_every_kernel_is_launched_through_gto_launch():
    src, core = source(), source("gto_shells.hpp")
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src))
    launched = set(re.findall(r"\bgto_launch\(\s*(\w+)\s*[<,]", src))
    assert defined == launched == {"sgto_pair_kernel", "sgto_one_kernel", "sgto_nuc_kernel", "sgto_two_kernel"}, \
        sorted(defined ^ launched)
    assert "<<<" not in src and "hipLaunchKernelGGL" not in src and "hipLaunchKernel(" not in src
    assert "<<<" not in core and "hipLaunchKernelGGL" not in core
    assert len(re.findall(r"\bhipLaunchKernel\(", core)) == 1
    helper = core[core.index("static void gto_launch("):]
    assert "hipLaunchKernel(" in helper[:helper.index("\n}\n")]
    assert "atomic" not in src.lower()


def test_no_new_profile_stage_and_no_new_abi_version():
    from evcont_amd import _lib
    assert re.search(r"constexpr int kProfStages = 14;", source("pipeline.hpp"))
    with open(os.path.join(REPO, "include", "evcont_hip.h")) as f:
        assert re.search(r"#define\s+EVC_ABI_VERSION\s+10\b", f.read())
    assert _lib.ABI_VERSION == 10
    assert "note_kernel" not in source() and "EVC_PROF_" not in source()


def test_refusals_need_no_device():
    """Every refused argument is caught on the host, before anything is launched: rc < 0 and a message."""
    from evcont_amd import _lib, build
    build.build()
    lib = _lib.load()
    ex = (C.c_double * 3)(3.42525091, 0.62391373, 0.16885540)
    co = (C.c_double * 3)(0.15432897, 0.53532814, 0.44463454)
    out = _lib.SgtoOutputs(*([256] * 8))
    need = lib.evc_sgto_workspace_bytes(4, 3, 2)
    assert need >= 2 * 3 * 3 * 10 * 5 * 8
    good = dict(natm=4, nprim=3, count=2, coords=256, charges=256, ex=ex, co=co, out=C.byref(out), flags=0, ws=256,
                ws_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        return lib.evc_sgto_integrals_batch(a["natm"], a["nprim"], a["count"], a["coords"], a["charges"], a["ex"],
                                            a["co"], a["out"], a["flags"], a["ws"], a["ws_bytes"], None)

    bad_ex = (C.c_double * 3)(3.4, 0.0, 0.1)
    no_grad = _lib.SgtoOutputs(256, 256, 256, 256, None, None, None, None)
    no_eri = _lib.SgtoOutputs(256, 256, 256, None, 256, 256, 256, 256)
    for kw, word in ((dict(natm=0), b"natm"), (dict(natm=97), b"natm"), (dict(nprim=0), b"nprim"),
                     (dict(nprim=9), b"nprim"), (dict(count=0), b"count"), (dict(coords=None), b"null"),
                     (dict(charges=None), b"null"), (dict(ex=None), b"null"), (dict(co=None), b"null"),
                     (dict(out=None), b"null"), (dict(ws=None), b"null"), (dict(out=C.byref(no_eri)), b"null"),
                     (dict(out=C.byref(no_grad)), b"null"), (dict(flags=2), b"flags"), (dict(flags=64), b"flags"),
                     (dict(ex=bad_ex), b"exponent"), (dict(ws_bytes=need - 1), b"workspace"),
                     (dict(natm=65, flags=_lib.FLAG_ERI_S4, ws_bytes=1 << 40), b"natm <= 64")):
        assert call(**kw) < 0, kw
        assert word in lib.evc_last_error(), (kw, lib.evc_last_error())
    assert lib.evc_sgto_workspace_bytes(97, 3, 1) == 0 and lib.evc_sgto_workspace_bytes(4, 9, 1) == 0
    assert lib.evc_sgto_workspace_bytes(4, 3, 0) == 0
