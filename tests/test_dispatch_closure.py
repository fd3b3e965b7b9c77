"""Host-side closure of the dispatch table: every kernel the library launches (a ``hipLaunchKernelGGL`` or a
``name<<<`` / ``name<...><<<`` in ``evcont_amd/csrc/*.hip``) occurs as an expected name in ``tests/dispatch_table.py``
or ``tests/fci_dispatch_table.py``, or is exempted below with the test that covers it.  Adding a kernel branch without a
table row fails ``pytest -m "not gpu"``; so does an instantiation in the full-CI switches of ``fci.hip`` that no tested
orbital count launches."""
import glob
import os
import re

import fci_dispatch_table as fci
from dispatch_table import CASES, KNOB_CASES, STAGES

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "evcont_amd", "csrc")

# Kernels no stage record names, each with what runs it.
EXEMPT = {
    # every gradient call, around the recorded stages (tests/test_gpu_dispatch_map.py checks the gradients they produce)
    "grad_prep_kernel": "tests.test_gpu_dispatch_map::test_dispatch_case (every gradient row but the unpack8_prep ones)",
    "grad_final_kernel": "tests.test_gpu_dispatch_map::test_dispatch_case (every gradient row)",
    # the summing launch of K5 when the span plan has more than 64 spans (wide matrices), and of the phase API
    "rows_reduce_kernel": "tests.test_gpu_bench_config::test_k5_row_groups_wide_matrix, "
                          "tests.test_gpu_batch (phase calls)",
    # row-slab K8 of the one-body matrix (T*T >= 1024, fewer than 12 geometries): launched before the recorded K8
    # kernel of the same stage
    "gemv_cols_slab_kernel": "tests.test_gpu_dispatch_map::test_dispatch_case[n6_T32_sym8_packed_G2_nroots3]",
    "gemv_cols_slab_reduce_kernel": "tests.test_gpu_dispatch_map::test_dispatch_case[n6_T32_sym8_packed_G2_nroots3]",
    # caller-supplied coefficients (non-Hermitian branch, evc_phase_set_coeffs)
    "pair_weights_kernel": "tests.test_gpu_large_T (energy_with_grad_nonhermitian)",
    # stand-alone C ABI helpers outside the energy+force pipeline
    "gemv_rows_reduce_kernel": "tests.test_gpu_parity::test_gemv_rows_cols (evc_gemv_rows)",
    "unpack_kernel": "tests.test_gpu_parity::test_pack_unpack_bitexact (evc_unpack_pair_sym)",
    "loewdin_trafo_grad_kernel": "tests.test_gpu_api::test_gradient_module_blocks (csrc/response.hip)",
    "dx_tensor_kernel": "tests.test_gpu_api::test_gradient_module_blocks (csrc/response.hip)",
    "one_el_grad_kernel": "tests.test_gpu_api::test_gradient_module_blocks (csrc/response.hip)",
    "contract_kernel": "tests.test_gpu_api::test_gradient_module_blocks (csrc/response.hip)",
    # full-CI entry points (csrc/fci.hip): launched around the recorded kernels by every evc_fci_trdm_rows /
    # evc_fci_sigma call
    "fci_trdm_reduce1_kernel": "tests.test_gpu_fci_shapes::test_every_orbital_count (every t-RDM call)",
    "fci_trdm_reduce2_kernel": "tests.test_gpu_fci_shapes::test_every_orbital_count (every t-RDM call)",
    "fci_sigma_prep_kernel": "tests.test_gpu_fci_shapes::test_every_orbital_count (every sigma call)",
}


def launched_kernels():
    names = set()
    for p in glob.glob(os.path.join(CSRC, "*.hip")):
        with open(p) as f:
            src = f.read()
        names.update(re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_]\w*)", src))
        names.update(re.findall(r"\b([A-Za-z_]\w*)\s*(?:<[^<>;(){}]*>)?\s*<<<", src))
    return names


def fci_source():
    with open(os.path.join(CSRC, "fci.hip")) as f:
        return f.read()


def function_body(src, signature):
    """The text between the braces of the function whose definition starts with ``signature``."""
    start = src.index(signature)
    i = src.index("{", start)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        if depth == 0:
            return src[i + 1:j]
        j += 1


def fci_table_names():
    """Kernel names in the expected records of tests/fci_dispatch_table.py."""
    out = {"fci_sigma_gather_kernel"}       # the second half of every sigma record
    for n in fci.TILINGS:
        out.update(re.findall(r"[A-Za-z_]\w*_kernel\b", fci.trdm_record(n, 1) + fci.sigma_record(n)))
    for rec in fci.EXCITE_KERNELS.values():
        out.update(re.findall(r"[A-Za-z_]\w*_kernel\b", rec))
    return out


def table_names():
    out = set()
    for c in CASES + KNOB_CASES:
        for exp in (c["expect"], c["expect_grad"] or {}):
            for s in exp.values():
                out.update(re.findall(r"[A-Za-z_]\w*_kernel\b", s))
    return out


def test_table_is_well_formed():
    ids = [c["id"] for c in CASES + KNOB_CASES]
    assert len(ids) == len(set(ids))
    for c in CASES + KNOB_CASES:
        assert c["layout"] in ("full6", "pair5", "elec3", "pack2", "sym8"), c["id"]
        assert not c["packed"] or (c["layout"] == "sym8" and c["n"] <= 64), c["id"]
        assert c["api"] in ("single", "batch", "roots", "roots_batch"), c["id"]
        assert c["api"] in ("batch", "roots_batch") or c["G"] == 1, c["id"]
        if c["api"] in ("roots", "roots_batch"):     # root pairs k <= l < nroots, no flags of the other entries
            assert c["pairs"] and all(0 <= k <= l < c["nroots"] for k, l in c["pairs"]), c["id"]
            assert not (c["energy_only"] or c["warm"] or c["keep"]), c["id"]
        else:
            assert c["pairs"] is None, c["id"]
        assert (c["expect_grad"] is not None) == c["energy_only"], c["id"]
        assert bool(c["env"]) == bool(c["covered_by"]), c["id"]
        assert 1 <= c["nroots"] <= c["T"], c["id"]
        if c["energy_only"]:    # an energy-only call launches nothing of the gradient side
            assert all(c["expect"][k] == "" for k in ("k8_cols", "ip1", "y2")), c["id"]
        for exp in (c["expect"], c["expect_grad"]):
            assert exp is None or set(exp) == set(STAGES), c["id"]


def test_knob_rows_name_existing_tests():
    here = os.path.dirname(os.path.abspath(__file__))
    for c in KNOB_CASES:
        mod, test = c["covered_by"].split("::")
        with open(os.path.join(here, mod.split(".")[-1] + ".py")) as f:
            src = f.read()
        assert f"def {test.split('[')[0]}(" in src, c["covered_by"]
        for k, v in c["env"].items():
            assert f'"{k}": "{v}"' in src, (c["id"], k)


def test_every_ip1_slot_count_is_in_the_table():
    """Every multi-slot instance of the int2e_ip1 pair-block form, 2, 4, ... kIp1MaxSlots slots per block
    (csrc/kernels.hpp, csrc/ip1.hip ip1_kslots), is the expected IP1 record of some row."""
    with open(os.path.join(CSRC, "kernels.hpp")) as f:
        m = re.search(r"constexpr\s+int\s+kIp1MaxSlots\s*=\s*(\d+)\s*;", f.read())
    assert m, "kIp1MaxSlots not found in csrc/kernels.hpp"
    kmax = int(m.group(1))
    assert kmax >= 2 and kmax & (kmax - 1) == 0, kmax
    records = {exp["ip1"] for c in CASES + KNOB_CASES for exp in (c["expect"], c["expect_grad"] or {}) if exp}
    found = {int(r) for rec in records for r in re.findall(r"\bslots=(\d+)$", rec)}
    want = {1 << k for k in range(1, kmax.bit_length())}
    assert want <= found, f"IP1 slot counts without a dispatch-table row: {sorted(want - found)}"
    assert found <= want, f"IP1 slot counts the library cannot launch: {sorted(found - want)}"


def test_every_launched_kernel_is_in_the_table():
    launched = launched_kernels()
    assert len(launched) >= 40, sorted(launched)    # the parse found the launch sites
    assert {"fci_trdm_kernel", "fci_sigma_gemm_kernel", "fci_excite_det_kernel", "fci_excite_orb_kernel"} <= launched
    listed = table_names() | fci_table_names()
    missing = sorted(launched - listed - set(EXEMPT))
    assert not missing, f"kernels with neither a dispatch-table row nor an exemption: {missing}"
    stale = sorted((listed | set(EXEMPT)) - launched)
    assert not stale, f"names in the table / exemption list that no launch site has: {stale}"
    assert not (listed & set(EXEMPT)), sorted(listed & set(EXEMPT))


def test_fci_table_is_well_formed():
    assert sorted(fci.TILINGS) == list(range(1, 17))
    assert {c[0] for c in fci.SHAPE_CASES} == set(fci.TILINGS)        # every orbital count has a GPU case
    for n, t in fci.TILINGS.items():
        nt = t["npad"] // 16
        rt, nbw = t["trdm"]
        assert t["npad"] % 16 == 0 and n * n <= t["npad"] < n * n + 16, n
        nq = {1: 1, 4: 2}[t["quadrants"]]
        assert (nq * nbw - 1) * rt < nt <= nq * nbw * rt, n           # the tiling covers the edge, no idle wave row
        assert (t["sigma_nbw"] - 1) * t["sigma"] < nt <= t["sigma_nbw"] * t["sigma"] and t["sigma"] <= 4, n


def test_every_fci_instantiation_is_launched_by_a_tested_orbital_count():
    """The switches of launch_trdm and evc_fci_sigma against the table: a ``case`` added without an orbital count in
    tests/fci_dispatch_table.py that launches it fails here, and so does a table row the switch cannot serve."""
    src = fci_source()
    body = function_body(src, "static void launch_trdm(")
    cases = re.findall(r"(case\s+(\d+)|default)\s*:\s*launch_trdm_t<\s*(\d+)\s*,\s*(\d+)\s*>", body)
    assert len(cases) == len(re.findall(r"\bcase\b|\bdefault\b", body)) >= 7, body
    assert len(re.findall(r"launch_trdm_t<\s*\d", src)) == len(cases)      # none is launched from elsewhere
    for _, code, rt, nbw in cases:
        assert not code or int(code) == int(rt) * 10 + int(nbw), (code, rt, nbw)
    switch = {(int(rt), int(nbw)) for _, _, rt, nbw in cases}
    assert switch == fci.trdm_instantiations(), (sorted(switch), sorted(fci.trdm_instantiations()))
    body = function_body(src, 'extern "C" int evc_fci_sigma(')
    cases = re.findall(r"(case\s+(\d+)|default)\s*:\s*launch_sigma_gemm_t<\s*(\d+)\s*>", body)
    assert len(cases) == len(re.findall(r"\bcase\b|\bdefault\b", body)) >= 4, body
    assert len(re.findall(r"launch_sigma_gemm_t<\s*\d", src)) == len(cases)
    for _, code, rt in cases:
        assert not code or int(code) == int(rt), (code, rt)
    switch = {int(rt) for _, _, rt in cases}
    assert switch == fci.sigma_instantiations(), (sorted(switch), sorted(fci.sigma_instantiations()))
