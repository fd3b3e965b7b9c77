"""Host-side closure for csrc/fci_spin.hip (S^2 on device CI vectors), modelled on tests/test_sgto_closure.py: the two calls
are declared in the header, bound in ``_lib`` and exported, the file is built, every kernel it defines is launched through
``spin_launch`` and through nothing else and named in exactly one record of EVC_PROF_FCI_SOLVE, the calls add neither a
profile stage nor an ABI version, and every refusal comes on the host, without a device."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "evcont_amd", "csrc")
CALLS = ("evc_fci_spin_apply", "evc_fci_spin_diag")
# entry point -> the record it leaves, as a regular expression (tests/test_gpu_fci_spin.py holds the library to them)
SPIN_RECORDS = {
    "evc_fci_spin_apply": r"fci_spin_apply_kernel beta=[01] tiles=\d+",
    "evc_fci_spin_diag": r"fci_spin_diag_kernel",
}


def source(name="fci_spin.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_calls_are_declared_bound_and_built():
    from evcont_amd import _lib, build
    with open(os.path.join(REPO, "include", "evcont_hip.h")) as f:
        hdr = f.read()
    for name in CALLS:
        assert f"int {name}(" in hdr, name
        assert name in _lib.SIGNATURES, name
    assert "fci_spin.hip" in build.SOURCES
    build.build()
    lib = _lib.load()
    for name in CALLS:
        assert getattr(lib, name) is not None


def test_every_kernel_is_launched_through_spin_launch_and_recorded_once():
    src = source()
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src))
    launched = set(re.findall(r"\bspin_launch\(\s*(\w+)\s*[<,]", src))
    assert defined == launched == {"fci_spin_apply_kernel", "fci_spin_diag_kernel"}, sorted(defined ^ launched)
    assert "<<<" not in src and "hipLaunchKernelGGL" not in src
    assert len(re.findall(r"\bhipLaunchKernel\(", src)) == 1
    helper = src[src.index("static void spin_launch("):]
    assert "hipLaunchKernel(" in helper[:helper.index("\n}\n")]
    assert "atomic" not in re.sub(r"//[^\n]*", "", src).lower()             # outside the comments
    records = re.findall(r'note_kernel\(EVC_PROF_FCI_SOLVE,\s*"([^"]*)"', src)
    for kernel in defined:
        assert sum(kernel in r for r in records) == 1, (kernel, records)
    for entry, rec in SPIN_RECORDS.items():
        start = src.index(f'extern "C" int {entry}(')
        end = src.find('extern "C"', start + 1)
        body = src[start:end if end > 0 else len(src)]
        notes = [n for n in re.findall(r'note_kernel\(EVC_PROF_FCI_SOLVE,\s*"([^"]*)"', body) if "_kernel" in n]
        assert len(notes) == 1, entry
        assert re.fullmatch(rec, re.sub(r"%l*d", "1", notes[0])), (entry, notes[0])
    # the kernels stay out of fci_solve.hip, whose kernel set tests/test_fci_solve_closure.py holds closed
    assert "fci_spin" not in source("fci_solve.hip")


def test_no_new_profile_stage_and_no_new_abi_version():
    from evcont_amd import _lib
    assert re.search(r"constexpr int kProfStages = 14;", source("pipeline.hpp"))
    with open(os.path.join(REPO, "include", "evcont_hip.h")) as f:
        assert re.search(r"#define\s+EVC_ABI_VERSION\s+10\b", f.read())
    assert _lib.ABI_VERSION == 10 and _lib.FCI_PROF_SOLVE == 11


def test_refusals_need_no_device():
    """Every refused argument is caught on the host, before anything is launched: rc < 0 and a message."""
    from evcont_amd import _lib, build
    build.build()
    lib = _lib.load()
    dim = 6 * 6
    good = dict(norb=4, na=6, nb=6, ta=4096, tb=4096, c=1 << 20, out=(1 << 20) + 8 * dim, hd=1 << 20)

    def apply(**kw):
        a = dict(good, **kw)
        return lib.evc_fci_spin_apply(a["norb"], a["na"], a["nb"], a["ta"], a["tb"], a["c"], 1.0, 0.0, 0.0, a["out"], None)

    def diag(**kw):
        a = dict(good, **kw)
        return lib.evc_fci_spin_diag(a["norb"], a["na"], a["nb"], a["ta"], a["tb"], 1.0, 0.0, a["hd"], None)

    shapes = ((dict(norb=0), b"norb"), (dict(norb=17), b"norb"), (dict(na=0), b"na="), (dict(na=12871), b"na="),
              (dict(nb=0), b"nb="), (dict(nb=12871), b"nb="), (dict(ta=None), b"null"), (dict(tb=None), b"null"))
    for kw, word in shapes + ((dict(c=None), b"null"), (dict(out=None), b"null"), (dict(out=good["c"]), b"alias"),
                              (dict(out=good["c"] + 8 * (dim - 1)), b"alias"),
                              (dict(out=good["c"] - 8 * (dim - 1)), b"alias")):
        assert apply(**kw) < 0, kw
        msg = lib.evc_last_error()
        assert word in msg and b"evc_fci_spin_apply" in msg, (kw, msg)
    for kw, word in shapes + ((dict(hd=None), b"null"),):
        assert diag(**kw) < 0, kw
        msg = lib.evc_last_error()
        assert word in msg and b"evc_fci_spin_diag" in msg, (kw, msg)
