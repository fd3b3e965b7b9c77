"""Host-side closure for csrc/fci_solve.hip, the counterpart of tests/test_dispatch_closure.py for the eigensolver's
vector kernels: that file launches through ``solve_launch(kernel, ...)`` only, and every kernel it launches is named in a
record of the stage EVC_PROF_FCI_SOLVE listed here; tests/test_gpu_fci_davidson.py holds the library to these records."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "evcont_amd", "csrc")

# entry point -> the record it leaves, as a regular expression
SOLVE_RECORDS = {
    "evc_fci_hdiag": r"fci_hdiag_prep_kernel \+ fci_hdiag_string_kernel strings=\d+ \+ fci_hdiag_det_kernel",
    "evc_fci_dots": r"fci_dots_kernel nx=\d+ ny=\d+ groups=\d+ blocks=\d+ \+ fci_solve_reduce_kernel",
    "evc_fci_combine": r"fci_combine_kernel m=\d+ k=\d+ groups=\d+",
    "evc_fci_davidson_correction": r"fci_correction_kernel m=\d+ k=\d+ groups=\d+ blocks=\d+ \+ fci_solve_reduce_kernel",
}


def source():
    with open(os.path.join(CSRC, "fci_solve.hip")) as f:
        return f.read()


def test_every_kernel_of_fci_solve_is_launched_and_recorded():
    src = source()
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src))
    launched = set(re.findall(r"\bsolve_launch\(\s*(\w+)\s*,", src))
    assert len(defined) >= 7 and defined == launched, sorted(defined ^ launched)
    assert "<<<" not in src and "hipLaunchKernelGGL" not in src          # no launch site outside solve_launch
    assert len(re.findall(r"\bhipLaunchKernel\(", src)) == 1
    named = set()
    for rec in SOLVE_RECORDS.values():
        named.update(re.findall(r"\w+_kernel\b", rec))
    assert named == launched, sorted(named ^ launched)


def test_every_record_is_noted_by_its_entry_point():
    src = source()
    for entry, rec in SOLVE_RECORDS.items():
        start = src.index(f'extern "C" int {entry}(')
        end = src.find('extern "C"', start + 1)
        body = src[start:end if end > 0 else len(src)]
        notes = re.findall(r'note_kernel\(EVC_PROF_FCI_SOLVE,\s*"([^"]*)"', body)
        assert len(notes) == 1, entry
        sample = re.sub(r"%l*d", "7", notes[0])
        assert re.fullmatch(rec, sample), (entry, sample)
