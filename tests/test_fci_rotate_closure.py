"""Host-side closure for csrc/fci_rotate.hip, modelled on tests/test_fci_solve_closure.py: that file launches through
``rotate_launch(kernel, ...)`` only, and every kernel it defines is launched and named in the one record of the stage
EVC_PROF_FCI_ROTATE (12) that evc_fci_rotate leaves; tests/test_gpu_fci_rotate.py holds the library to that record."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "evcont_amd", "csrc")

ROTATE_RECORD = (r"fci_minor_kernel<([1-8])> \+ fci_minor_kernel<([1-8])> comp=([01]),([01]) panels=(\d+),(\d+) "
                 r"\+ fci_rotate_gemm_kernel")


def source():
    with open(os.path.join(CSRC, "fci_rotate.hip")) as f:
        return f.read()


def test_every_kernel_of_fci_rotate_is_launched_and_recorded():
    src = source()
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src))
    launched = set(re.findall(r"\brotate_launch\(\s*(\w+)\s*[<,]", src))
    assert defined == launched == {"fci_minor_kernel", "fci_rotate_gemm_kernel"}, sorted(defined ^ launched)
    assert "<<<" not in src and "hipLaunchKernelGGL" not in src          # no launch site outside rotate_launch
    assert len(re.findall(r"\bhipLaunchKernel\(", src)) == 1
    assert set(re.findall(r"\w+_kernel\b", ROTATE_RECORD)) == launched


def test_only_the_minors_up_to_order_eight_are_instantiated():
    orders = sorted(int(k) for k in re.findall(r"rotate_launch\(\s*fci_minor_kernel<\s*(\d+)\s*>", source()))
    assert orders == list(range(1, 9))


def test_the_entry_point_notes_one_record_for_stage_12():
    src = source()
    start = src.index('extern "C" int evc_fci_rotate(')
    body = src[start:]
    notes = re.findall(r'note_kernel\(EVC_PROF_FCI_ROTATE,\s*((?:"[^"]*"\s*)+)', body)
    assert len(notes) == 1
    fmt = "".join(re.findall(r'"([^"]*)"', notes[0]))
    assert re.fullmatch(ROTATE_RECORD, re.sub(r"%l*d", "7", fmt).replace("comp=7,7", "comp=1,0")), fmt
    with open(os.path.join(REPO, "include", "evcont_hip.h")) as f:
        assert re.search(r"#define\s+EVC_PROF_FCI_ROTATE\s+12\b", f.read())
    from evcont_amd import _lib
    assert _lib.FCI_PROF_ROTATE == 12 and _lib.ABI_VERSION == 10
