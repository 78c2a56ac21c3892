"""Register / scratch budget of k_attn_qkpv (the one-kernel attention core), read from the cross-compiled gfx950 ISA (no GPU
needed), in the manner of tests/test_isa_budget_qkv.py: the four instances keep their accumulators in registers -- no scratch --
and at least two waves per SIMD; k_attn_qk, which the new kernel shares no code with, kept the counts it had."""
import importlib.util
import os
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#                 instance                          VGPRs  waves per SIMD      (of the build before k_attn_qkpv)
QK_BEFORE = {"k_attn_qk<true, false>": (66, 7), "k_attn_qk<false, false>": (68, 7),
             "k_attn_qk<true, true>": (80, 6), "k_attn_qk<false, true>": (80, 6)}
#            TWIN, NDT: the accumulators alone are 16 NDT (32 NDT) VGPRs
PV_MAX_VGPRS = {"k_attn_qkpv<false, 2>": 128, "k_attn_qkpv<true, 2>": 168, "k_attn_qkpv<false, 4>": 168, "k_attn_qkpv<true, 4>": 256}


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
    return {names[k].replace("void p4v::", "").split("(")[0]: r for k, r in res.items() if "k_attn_qk" in names[k]}


@pytest.mark.parametrize("name", sorted(PV_MAX_VGPRS))
def test_one_kernel_instances_keep_their_accumulators_in_registers(kernels, name):
    k = kernels[name]
    assert k["ScratchSize"] == 0 and k.get("NumAgprs", 0) == 0, k
    assert k["NumVgprs"] <= PV_MAX_VGPRS[name] and k["Occupancy"] >= 2, k


def test_k_attn_qk_did_not_move(kernels):
    got = {n: (kernels[n]["NumVgprs"], kernels[n]["Occupancy"]) for n in QK_BEFORE}
    assert got == QK_BEFORE and all(kernels[n]["ScratchSize"] == 0 for n in QK_BEFORE), got
