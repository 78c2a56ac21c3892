"""Register / scratch budget of the window instances of k_attn_qk (the fused window attention forward), read from
the cross-compiled gfx950 ISA like tests/test_isa_budget.py (no GPU needed; the same tools/isa_report.py report).

The kernel takes its key fragments straight from global memory and hides that latency with resident waves: it lives on its
occupancy.  The window instances carry two more address streams (the bias row and the mask row of the lane's query), which
costs registers: at most ONE wave per SIMD below the non-window instance of the same TWIN, in the same compile, and no scratch.
Measured figures of all four instances: DESIGN.md s5.10."""
import re

import pytest

from tests.test_isa_budget import resources  # noqa: F401 -- the fixture: one compile of the library's kernels to assembly


def _instances(resources):  # noqa: F811
    out = {}
    for name, v in resources.items():
        m = re.search(r"\bk_attn_qk<(true|false)(?:, (true|false))?>", name)
        if m:
            out[(m.group(1) == "true", m.group(2) == "true")] = v
    return out


def test_window_instances_exist_without_scratch(resources):  # noqa: F811
    inst = _instances(resources)
    assert set(inst) == {(False, False), (True, False), (False, True), (True, True)}, sorted(inst)
    for key, v in inst.items():
        assert v.get("ScratchSize", 0) == 0, (key, v)


@pytest.mark.parametrize("twin", [False, True], ids=["plain", "twin"])
def test_window_instance_keeps_the_occupancy_within_one_wave(resources, twin):  # noqa: F811
    inst = _instances(resources)
    base, win = inst[(twin, False)], inst[(twin, True)]
    print(f"[isa] k_attn_qk<{twin}>: {base['NumVgprs']} VGPRs, occupancy {base['Occupancy']}; window: {win['NumVgprs']} VGPRs, occupancy {win['Occupancy']}")
    assert win["NumVgprs"] + win.get("NumAgprs", 0) <= 256
    assert win["Occupancy"] >= base["Occupancy"] - 1, (base, win)
