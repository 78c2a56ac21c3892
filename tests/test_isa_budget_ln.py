"""Register / scratch budget of k_ln_pack (the fused LayerNorm producer), read from the cross-compiled gfx950 ISA
(no GPU needed), in the manner of tests/test_isa_budget_wpv.py: every instance keeps its row in registers -- no scratch, no AGPRs,
at most 96 VGPRs -- and at least four waves per SIMD."""
import importlib.util
import os
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSTANCES = ["k_ln_pack<1, 32>", "k_ln_pack<1, 64>", "k_ln_pack<2, 64>", "k_ln_pack<4, 64>", "k_ln_pack<8, 64>"]   # this build: 31 / 31 / 28 / 47 / 75 VGPRs


@pytest.fixture(scope="module")
def kernels():
    spec = importlib.util.spec_from_file_location("isa_report", os.path.join(ROOT, "tools", "isa_report.py"))
    rep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rep)
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as d:
        res = rep.resources(open(rep.compile_asm(d)).read().split("\n"))
    names = rep.demangle(list(res))
    return {names[k].replace("void p4v::", "").split("(")[0]: r for k, r in res.items() if "k_ln_pack" in names[k]}


@pytest.mark.parametrize("name", INSTANCES)
def test_ln_pack_instances_keep_their_row_in_registers(kernels, name):
    assert sorted(kernels) == sorted(INSTANCES), sorted(kernels)
    k = kernels[name]
    assert k["ScratchSize"] == 0 and k.get("NumAgprs", 0) == 0, k
    assert k["NumVgprs"] <= 96 and k["Occupancy"] >= 4, k
