"""Register / scratch / LDS budget of k_qkv_heads (the fused qkv forward's producer), read from the cross-compiled gfx950 ISA
(no GPU needed), in the manner of tests/test_isa_budget.py: no scratch, at most 128 VGPRs and at most 80 KB of LDS per
512-thread workgroup, so that two workgroups fit a CU.  The kernel's LDS is dynamic: the static part comes from the ISA, the
dynamic part from the launch in p4v_api.hip (four staging tiles of SW_BM rows x SW_ROW bytes)."""
import importlib.util
import os
import re
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ptq4vit_amd", "csrc")


@pytest.fixture(scope="module")
def kernel():
    spec = importlib.util.spec_from_file_location("isa_report", os.path.join(ROOT, "tools", "isa_report.py"))
    rep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rep)
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as d:
        lines = open(rep.compile_asm(d)).read().split("\n")
    res = rep.resources(lines)
    names = rep.demangle(list(res))
    mine = [k for k in res if names[k].startswith("p4v::k_qkv_heads(")]
    assert len(mine) == 1, [names[k] for k in res if "qkv" in names[k]]
    out = dict(res[mine[0]])
    # the static LDS of the same kernel: "; LDSByteSize: N bytes/workgroup" behind its label
    at = next(i for i, l in enumerate(lines) if l.startswith(mine[0] + ":"))
    for l in lines[at:]:
        m = re.match(r"^; LDSByteSize: (\d+)", l)
        if m:
            out["StaticLds"] = int(m.group(1))
            break
    return out


def _dynamic_lds():
    hdr = open(os.path.join(CSRC, "p4v_kernels.h")).read()
    m = re.search(r"SW_BM = (\d+), SW_BN = (\d+), SW_BKB = (\d+), SW_ROW = (\d+);", hdr)
    tile = int(m.group(1)) * int(m.group(4))
    assert re.search(r"SW_TILE_BYTES = SW_BM \* SW_ROW;", hdr)
    api = open(os.path.join(CSRC, "p4v_api.hip")).read()
    launch = re.search(r"Kern1<QkvHeadsParams, k_qkv_heads>::desc\(\), dim3\([^;]*?\), dim3\((\d+)\), ([^,]*SW_TILE_BYTES[^,]*),", api)
    assert launch, "the launch of k_qkv_heads in p4v_api.hip"
    factor = eval(launch.group(2).replace("SW_TILE_BYTES", "1"), {"__builtins__": {}})
    return int(launch.group(1)), factor * tile


def test_qkv_heads_fits_two_workgroups_per_cu(kernel):
    threads, dynamic = _dynamic_lds()
    assert threads == 512
    assert kernel["ScratchSize"] == 0, kernel
    assert kernel["NumVgprs"] + kernel.get("NumAgprs", 0) <= 128, kernel
    assert kernel["StaticLds"] + dynamic <= 80 * 1024, (kernel, dynamic)
    assert dynamic == 40960
    assert kernel["Occupancy"] >= 4, kernel          # (512 threads = 2 waves per SIMD per workgroup: two workgroups)
