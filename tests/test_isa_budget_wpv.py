"""Register / scratch budget of k_wattn_qkpv (the one-kernel window attention core), read from the cross-compiled gfx950 ISA (no
GPU needed), in the manner of tests/test_isa_budget_pv.py: the four instances keep a window's score rows and their accumulators
in registers -- no scratch, no AGPRs -- and at least two waves per SIMD."""
import importlib.util
import os
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#               TWIN, NT: the resident scores alone are 16 NT VGPRs      (this build: 90 / 90 / 197 / 197)
WPV_MAX_VGPRS = {"k_wattn_qkpv<false, 2>": 128, "k_wattn_qkpv<true, 2>": 128, "k_wattn_qkpv<false, 5>": 256, "k_wattn_qkpv<true, 5>": 256}


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
    return {names[k].replace("void p4v::", "").split("(")[0]: r for k, r in res.items() if "k_wattn_qkpv" in names[k]}


@pytest.mark.parametrize("name", sorted(WPV_MAX_VGPRS))
def test_window_instances_keep_their_score_rows_in_registers(kernels, name):
    k = kernels[name]
    assert k["ScratchSize"] == 0 and k.get("NumAgprs", 0) == 0, k
    assert k["NumVgprs"] <= WPV_MAX_VGPRS[name] and k["Occupancy"] >= 2, k
