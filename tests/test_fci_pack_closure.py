"""Host-side closure for csrc/fci_pack.hip, modelled on tests/test_fci_rotate_closure.py: that file launches through
``pack_launch(kernel, ...)`` only, every kernel it defines is launched and named in the one record of the stage
EVC_PROF_FCI_PACK (13) that evc_fci_trdm_rows_packed leaves, and both new calls are declared and bound;
tests/test_gpu_fci_rows_packed.py holds the library to that record."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "evcont_amd", "csrc")

PACK_RECORD = r"fci_row_pack_kernel<([18])> rows=(\d+) cols=(\d+) ld=(\d+)"


def source(name="fci_pack.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_every_kernel_of_fci_pack_is_launched_and_recorded():
    src = source()
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src))
    launched = set(re.findall(r"\bpack_launch\(\s*(\w+)\s*[<,]", src))
    assert defined == launched == {"fci_row_pack_kernel"}, sorted(defined ^ launched)
    assert "<<<" not in src and "hipLaunchKernelGGL" not in src          # no launch site outside pack_launch
    assert len(re.findall(r"\bhipLaunchKernel\(", src)) == 1
    assert set(re.findall(r"\w+_kernel\b", PACK_RECORD)) == launched
    assert sorted(int(k) for k in re.findall(r"pack_launch\(\s*fci_row_pack_kernel<\s*(\d+)\s*>", src)) == [1, 8]


def test_one_record_for_stage_13():
    notes = re.findall(r'note_kernel\(EVC_PROF_FCI_PACK,\s*((?:"[^"]*"\s*)+)', source())
    assert len(notes) == 1
    fmt = "".join(re.findall(r'"([^"]*)"', notes[0]))
    assert re.fullmatch(PACK_RECORD, re.sub(r"%l*d", "8", fmt)), fmt
    with open(os.path.join(REPO, "include", "evcont_hip.h")) as f:
        assert re.search(r"#define\s+EVC_PROF_FCI_PACK\s+13\b", f.read())
    assert re.search(r"constexpr int kProfStages = 14;", source("pipeline.hpp"))
    from evcont_amd import _lib
    assert _lib.FCI_PROF_PACK == 13 and _lib.ABI_VERSION == 10


def test_both_entry_points_share_the_row_call_and_are_bound():
    from evcont_amd import _lib, build
    fci = source("fci.hip")
    assert len(re.findall(r"\bstatic int fci_trdm_rows_run\(", fci)) == 1
    for name in ("evc_fci_trdm_rows", "evc_fci_trdm_rows_packed"):
        start = fci.index(f'extern "C" int {name}(')
        body = fci[start:fci.index('extern "C"', start + 10)]
        assert len(re.findall(r"\bfci_trdm_rows_run\(", body)) == 1, name
        assert "fci_trdm_kernel" not in body and "launch_trdm(" not in body, name     # the product lives in one place
    assert len(re.findall(r"\blaunch_trdm\(trt", fci)) == 1
    assert {"evc_fci_trdm_rows_packed", "evc_fci_rows_packed_workspace_bytes"} <= set(_lib.SIGNATURES)
    assert "fci_pack.hip" in build.SOURCES
    with open(os.path.join(REPO, "include", "evcont_hip.h")) as f:
        hdr = f.read()
    assert "evc_fci_trdm_rows_packed(" in hdr and "evc_fci_rows_packed_workspace_bytes(" in hdr
