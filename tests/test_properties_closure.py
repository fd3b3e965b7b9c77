"""Host-side closure for csrc/properties.hip (observables of continuation states, s-Gaussian dipole integrals), modelled
on tests/test_sgto_closure.py: the three calls are declared in the header, bound in ``_lib`` and exported, the file is
built, every kernel it defines is launched through ``prop_launch`` and through nothing else, the calls add neither a
profile stage nor an ABI version, and every refusal happens on the host with a message that names the function."""
import ctypes as C
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "evcont_amd", "csrc")
CALLS = ("evc_properties_workspace_bytes", "evc_properties_roots_batch", "evc_sgto_dipole_batch")


def source(name="properties.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def header():
    with open(os.path.join(REPO, "include", "evcont_hip.h")) as f:
        return f.read()


def test_calls_are_declared_bound_and_built():
    from evcont_amd import _lib, build
    hdr = header()
    for name in CALLS:
        assert f"{name}(" in hdr, name
        assert name in _lib.SIGNATURES, name
    out = re.search(r"typedef struct evc_property_outputs \{(.*?)\} evc_property_outputs;", hdr, re.S).group(1)
    assert re.findall(r"double \*(\w+);", out) == [f[0] for f in _lib.PropertyOutputs._fields_]
    assert C.sizeof(_lib.PropertyOutputs) == 5 * 8
    inp = re.search(r"typedef struct evc_property_inputs \{(.*?)\} evc_property_inputs;", hdr, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[3\])?;", inp) == [f[0] for f in _lib.PropertyInputs._fields_]
    assert C.sizeof(_lib.PropertyInputs) == 8 + 5 * 8 + 3 * 8
    assert _lib.PropertyInputs.origin.offset == 48
    assert "properties.hip" in build.SOURCES


def test_every_kernel_is_launched_through_prop_launch():
    src = source()
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src))
    launched = set(re.findall(r"\bprop_launch\(\s*(\w+)\s*[<,]", src))
    assert defined == launched == {"prop_d1_kernel", "prop_ao_kernel", "prop_sdip_kernel"}, sorted(defined ^ launched)
    assert "<<<" not in src and "hipLaunchKernelGGL" not in src
    assert len(re.findall(r"\bhipLaunchKernel\(", src)) == 1
    helper = src[src.index("static void prop_launch("):]
    assert "hipLaunchKernel(" in helper[:helper.index("\n}\n")]
    assert "atomic" not in src.lower()


def test_no_new_profile_stage_and_no_new_abi_version():
    from evcont_amd import _lib
    assert re.search(r"constexpr int kProfStages = 14;", source("pipeline.hpp"))
    assert re.search(r"#define\s+EVC_ABI_VERSION\s+10\b", header())
    assert _lib.ABI_VERSION == 10
    assert "note_kernel" not in source() and "EVC_PROF_" not in source()


def test_chunks_of_the_row_sum_depend_on_T_alone():
    """The rule the GPU tests read (tests/test_gpu_properties.py): T^2 rows above ``kPropRowsMin`` are split."""
    src = source()
    assert int(re.search(r"constexpr int kPropRowsMin = (\d+);", src).group(1)) == 256
    assert int(re.search(r"constexpr int kPropMaxChunks = (\d+);", src).group(1)) == 64
    assert int(re.search(r"constexpr int kPropGroup = (\d+);", src).group(1)) == 32


def test_refusals_need_no_device():
    """Every refused argument is caught on the host, before anything is launched: rc < 0 and a message that starts
    with the function's name.  Placeholder pointers: nothing is dereferenced on the device side."""
    import numpy as np
    from evcont_amd import _lib, build
    build.build()
    lib = _lib.load()
    who = b"evc_properties_roots_batch"

    def trdm(n=5, T=3):
        P, n2 = T * (T + 1) // 2, n * n
        M = n2 * (n2 + 1) // 2
        return _lib.TrdmSet(n=n, ntrain=T, layout=2, rows2=P, row_offset=0, rows2_total=P, cols2=M, ld2=(M + 15) // 16 * 16,
                            ld1=n2 + (n2 & 1), two_rdm=256, one_rdm=256, s_train=256)

    natm, count = 2, 2
    pairs = np.array([[0, 0], [0, 1], [1, 1]], dtype=np.int32)
    t = trdm()
    per_geo = lib.evc_workspace_bytes(C.byref(t), natm)
    need = lib.evc_properties_workspace_bytes(5, 3, natm, count, 3)
    assert per_geo > 0 and need >= 1 * count * 3 * 25 * 8
    # T = 17: 289 rows are two chunks of the row sum
    assert lib.evc_properties_workspace_bytes(5, 17, natm, count, 3) >= 2 * count * 3 * 25 * 8

    def inputs(**kw):
        a = dict(natm=natm, count=count, S=256, dip=256, aoslices=256, charges=256, coords=256)
        a.update(kw)
        return _lib.PropertyInputs(origin=(C.c_double * 3)(0.0, 0.0, 0.0), **a)

    def outputs(**kw):
        a = dict(d_oao=256, d_ao=256, dipole=256, mulliken=256, loewdin=256)
        a.update(kw)
        return _lib.PropertyOutputs(**a)

    good = dict(t=t, inp=inputs(), coeffs=256, nvec=2, pairs=pairs, npairs=3, out=outputs(), ws=256,
                ws_bytes=count * per_geo, scratch=256, scratch_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        ref = lambda x: None if x is None else C.byref(x)
        p = a["pairs"]
        return lib.evc_properties_roots_batch(ref(a["t"]), ref(a["inp"]), a["coeffs"], a["nvec"],
                                              None if p is None else p.ctypes.data, a["npairs"], ref(a["out"]), a["ws"],
                                              a["ws_bytes"], a["scratch"], a["scratch_bytes"], None)

    misordered = np.array([[1, 0], [0, 0], [1, 1]], dtype=np.int32)
    beyond = np.array([[0, 0], [0, 2], [1, 1]], dtype=np.int32)
    no_one = trdm()
    no_one.one_rdm = None
    cases = (
        (dict(t=None), b"null"), (dict(inp=None), b"null"), (dict(coeffs=None), b"null"), (dict(pairs=None), b"null"),
        (dict(out=None), b"null"), (dict(ws=None), b"null"), (dict(scratch=None), b"null"),
        (dict(inp=inputs(dip=None)), b"null"), (dict(inp=inputs(charges=None)), b"null"),
        (dict(inp=inputs(coords=None)), b"null"), (dict(inp=inputs(S=None)), b"null"),
        (dict(inp=inputs(aoslices=None)), b"null"), (dict(t=no_one), b"one_rdm"),
        (dict(t=trdm(n=97)), b"n=97"), (dict(t=trdm(T=513)), b"ntrain=513"),
        (dict(pairs=misordered), b"pair 0"), (dict(pairs=beyond), b"pair 1"), (dict(nvec=0), b"nvec"),
        (dict(nvec=4), b"nvec"), (dict(npairs=0), b"npairs"), (dict(inp=inputs(count=0)), b"count"),
        (dict(inp=inputs(count=1366)), b"count"), (dict(npairs=4097, inp=inputs(count=1)), b"npairs"),
        (dict(inp=inputs(natm=0)), b"natm"),
        (dict(ws=264), b"misaligned"), (dict(scratch=264), b"misaligned"), (dict(coeffs=260), b"misaligned"),
        (dict(inp=inputs(S=260)), b"misaligned"), (dict(out=outputs(dipole=260)), b"misaligned"),
        (dict(scratch_bytes=need - 1), b"scratch"), (dict(ws_bytes=count * per_geo - 1), b"ws of"),
    )
    for kw, word in cases:
        assert call(**kw) < 0, kw
        msg = lib.evc_last_error()
        assert msg.startswith(who) and word in msg, (kw, msg)
    # an input is required only by the outputs that read it
    assert lib.evc_properties_workspace_bytes(97, 3, 2, 1, 1) == 0 and lib.evc_properties_workspace_bytes(5, 513, 2, 1, 1) == 0
    assert lib.evc_properties_workspace_bytes(5, 3, 2, 4097, 1) == 0 and lib.evc_properties_workspace_bytes(5, 3, 2, 1, 0) == 0
    assert lib.evc_last_error().startswith(b"evc_properties_workspace_bytes")

    # evc_sgto_dipole_batch: the limits and refusals of evc_sgto_integrals_batch
    ex = (C.c_double * 3)(3.42525091, 0.62391373, 0.16885540)
    co = (C.c_double * 3)(0.15432897, 0.53532814, 0.44463454)
    bad_ex = (C.c_double * 3)(3.4, 0.0, 0.1)
    org = (C.c_double * 3)(0.0, 0.0, 0.0)
    good = dict(natm=4, nprim=3, count=2, coords=256, ex=ex, co=co, origin=org, dip=256)

    def sdip(**kw):
        a = dict(good, **kw)
        return lib.evc_sgto_dipole_batch(a["natm"], a["nprim"], a["count"], a["coords"], a["ex"], a["co"], a["origin"],
                                         a["dip"], None)

    for kw, word in ((dict(natm=0), b"natm"), (dict(natm=97), b"natm"), (dict(nprim=0), b"nprim"), (dict(nprim=9), b"nprim"),
                     (dict(count=0), b"count"), (dict(coords=None), b"null"), (dict(ex=None), b"null"),
                     (dict(co=None), b"null"), (dict(origin=None), b"null"), (dict(dip=None), b"null"),
                     (dict(ex=bad_ex), b"exponent"), (dict(dip=260), b"misaligned")):
        assert sdip(**kw) < 0, kw
        msg = lib.evc_last_error()
        assert msg.startswith(b"evc_sgto_dipole_batch") and word in msg, (kw, msg)
