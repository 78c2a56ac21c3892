"""GPU: which sweep kernel a pass runs on (csrc/p4v_api.hip, plan_sweep; DESIGN.md s5 "pass -> kernel") -- the smallest shape per
kernel family (tests/sweep_plan_cases.py), by the launch records of one calibration each.

Asserted: the family and the stage of every sweep record, in order, and grid_x of the first.  The expected values are what the
commit BEFORE plan_sweep existed (run_pass choosing the kernel inline) produced for the same table on an MI355X
(tools/plan_dump.py --gpu, profiles/r15_plan_parent.json); they are literals, not derived from the code under test.  A case that
changes family here means a selection predicate changed: that is a behaviour change, not a refactor.
"""
import pytest
import torch

from tests.sweep_plan_cases import CASES, run_case

pytestmark = pytest.mark.gpu

# case -> ([(kernel, stage)] of every sweep record, grid_x of the first)
EXPECTED = {
    "linear_k192_n128": ([("k_sweep6", "full")] * 2, 2),                       # weight search, activation search
    "linear_k128_n128": ([("k_sweep4/5", "full")] * 2, 1),
    "linear_k1024_n64": ([("k_sweep7", "full")] * 2, 100),
    # post-GELU: the weight search on the twin instance, the fold of the negative plane (a store pass), the activation search
    "postgelu_k1024_n64": ([("k_sweep7 (twin)", "full"), ("k_sweep2", "full"), ("k_sweep7", "full")], 100),
    "linear_k1088_n64": ([("k_sweep2g", "full"), ("k_sweep2", "full")], 1),    # weight search: pairs; activation search
    "linear_k192_n120_nV3": ([("k_sweep<int8>", "full")] * 2, 1),
    "matmul_qk_49": ([("k_sweep9", "full")] * 2, 1),
    "matmul_qk_120": ([("k_sweep8", "full")] * 2, 1),
    "matmul_sos_49": ([("k_sos_split", "full"), ("k_sweep2", "full")], 1),     # the split search, then B on the twin k_sweep2
    "conv_patch16_a32": ([("k_sweep<float>", "full")], 1),
    "bound_650x96_k192": ([("k_sweep6", "A"), ("k_bound", "B1"), ("k_sweep6", "A"), ("k_bound", "B1")], 2),
    "mmblk_qk_hessian_vA2hA2_vB2hB3": ([("k_sweep_seg", "full")] * 20, 1),
}


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    return engine


def test_every_case_has_an_expectation():
    assert sorted(EXPECTED) == sorted(name for name, _, _ in CASES)


@pytest.mark.parametrize("name,run,pruned", CASES, ids=[c[0] for c in CASES])
def test_pass_runs_on_the_planned_kernel_family(eng, name, run, pruned):
    res, recs, launches, _ = run_case(eng, run, prune=pruned)
    families, grid_x = EXPECTED[name]
    print(f"[sweep plan] {name}: {recs} ({launches['issued']} launches)")
    assert [r[:2] for r in recs] == families, (name, recs)
    assert recs[0][2] == grid_x, (name, recs[0])
    assert all(torch.isfinite(t.float()).all() for t in res[:2]), name
