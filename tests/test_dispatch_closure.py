"""Host-side closure of the dispatch table: every kernel the library launches (a ``hipLaunchKernelGGL`` in
``evcont_amd/csrc/*.hip``) occurs as an expected name in ``tests/dispatch_table.py``, or is exempted below with the
test that covers it.  Adding a kernel branch without a table row fails ``pytest -m "not gpu"``."""
import glob
import os
import re

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
    # no caller reaches it: the pipeline asks launch_unpack8 for lead_half=1 only together with the unpacked 2-RDM,
    # which takes unpack8_kernel
    "unpack8_half_kernel": "unreachable from the entry points",
}


def launched_kernels():
    names = set()
    for p in glob.glob(os.path.join(CSRC, "*.hip")):
        with open(p) as f:
            src = f.read()
        names.update(re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_]\w*)", src))
    return names


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
    listed = table_names()
    missing = sorted(launched - listed - set(EXEMPT))
    assert not missing, f"kernels with neither a dispatch-table row nor an exemption: {missing}"
    stale = sorted((listed | set(EXEMPT)) - launched)
    assert not stale, f"names in the table / exemption list that no launch site has: {stale}"
    assert not (listed & set(EXEMPT)), sorted(listed & set(EXEMPT))
