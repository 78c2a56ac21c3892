"""Register / scratch budget of k_lin_res (the fused block output), read from the cross-compiled gfx950 ISA (no GPU
needed), in the manner of tests/test_isa_budget_ln.py: both instances keep the accumulators and the residual pieces in registers -- no
scratch -- within 128 registers, so that two workgroups (four waves per SIMD) share a CU."""
import importlib.util
import os
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSTANCES = ["k_lin_res<false>", "k_lin_res<true>"]


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
    return {names[k].replace("void p4v::", "").split("(")[0]: r for k, r in res.items() if "k_lin_res" in names[k]}


@pytest.mark.parametrize("name", INSTANCES)
def test_lin_res_instances_have_no_scratch(kernels, name):
    assert sorted(kernels) == sorted(INSTANCES), sorted(kernels)
    k = kernels[name]
    assert k["ScratchSize"] == 0 and k["NumVgprs"] + k.get("NumAgprs", 0) <= 128 and k["Occupancy"] >= 4, k
