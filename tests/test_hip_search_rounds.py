"""GPU: the search rounds of csrc/p4v_api.hip (search_rounds under linear_impl, matmul_impl and conv_impl: pass memo, table slots,
pass builders; the step loop of MatMulBlocksCall) -- the smallest shape per path (tests/search_round_cases.py), three search
rounds each.

Asserted per case: the (kernel, stage) sequence of the launch records and the pass memo's (hits, misses) of the default call
(no tables: memo on) and of the call with score tables (no memo: every pass runs).  The expected values are what the commit BEFORE
the drivers were rebuilt around MemoSide / SearchRounds / LinearCall / MatMulCall produced for the same table on an MI355X
(tools/plan_dump.py --gpu, profiles/r16_calls_parent_gpu.json); they are literals, not derived from the code under test.  The
last four cases (MatMul with sub-blocks, which has no memo: (0, 0) in every mode; the rectangular dilated Conv) were added when
the Conv and sub-block calls became ConvCall / MatMulBlocksCall on one round driver; their literals are what the commit before
THAT change produced (profiles/r28_calls_parent_gpu.json).  A sequence that changes here means a pass was added, dropped or
moved, a counter that changes means the memo restored or recorded something else: a behaviour change, not a refactor.
Also asserted: the intervals of the default call are bit-equal to those of the call with score tables and of the call with the
memo switched off (desc.reserved bit 1) -- restoring a recorded selection is exact.
"""
import pytest
import torch

from tests.search_round_cases import CASES, MODES, run_case

pytestmark = pytest.mark.gpu

# case -> mode -> ([(kernel, stage), count] runs of the launch records, (memo hits, memo misses))
EXPECTED = {
    "linear_hessian_k192_n128": {
        "default": ([(("k_sweep6", "full"), 4)], (2, 4)),
        "scores": ([(("k_sweep6", "full"), 6)], (0, 0)),
    },
    "postgelu_hessian_k192_n128": {
        "default": ([(("k_sweep2", "full"), 2), (("k_sweep6", "full"), 1), (("k_sweep2", "full"), 1)], (3, 3)),
        "scores": ([(("k_sweep2", "full"), 2), (("k_sweep6", "full"), 1)] * 3, (0, 0)),
    },
    "postgelu_hessian_k1024_n64": {
        "default": ([(("k_sweep7 (twin)", "full"), 1), (("k_sweep2", "full"), 1), (("k_sweep7", "full"), 1)] * 2, (2, 4)),
        "scores": ([(("k_sweep7 (twin)", "full"), 1), (("k_sweep2", "full"), 1), (("k_sweep7", "full"), 1)] * 3, (0, 0)),
    },
    "linear_hessian_k192_n128_nH2_na2": {
        "default": ([(("k_sweep<float>", "full"), 12)], (0, 0)),
        "scores": ([(("k_sweep<float>", "full"), 12)], (0, 0)),
    },
    "bound_650x96_k192": {
        "default": ([(("k_sweep6", "A"), 1), (("k_bound", "B1"), 1)] * 6, (0, 6)),
        "scores": ([(("k_sweep6", "full"), 6)], (0, 0)),
    },
    "linear_cosine_k192_n128": {
        "default": ([(("k_sweep6", "full"), 3)], (3, 3)),
        "scores": ([(("k_sweep6", "full"), 6)], (0, 0)),
    },
    "linear_cosine_k1024_n64": {
        "default": ([(("k_sweep7", "full"), 3)], (3, 3)),
        "scores": ([(("k_sweep7", "full"), 6)], (0, 0)),
    },
    "linear_cosine_k192_n120_nV3": {
        "default": ([(("k_sweep2", "full"), 4)], (2, 4)),
        "scores": ([(("k_sweep2", "full"), 6)], (0, 0)),
    },
    "linblk_cos_v2h2a3_w4a4": {
        "default": ([(("k_sweep_seg", "full"), 15)], (0, 0)),
        "scores": ([(("k_sweep_seg", "full"), 15)], (0, 0)),
    },
    "matmul_qk_49_hessian": {
        "default": ([(("k_sweep9", "full"), 3)], (3, 3)),
        "scores": ([(("k_sweep9", "full"), 6)], (0, 0)),
    },
    "matmul_qk_49_cosine": {
        "default": ([(("k_sweep2", "full"), 4)], (2, 4)),
        "scores": ([(("k_sweep2", "full"), 6)], (0, 0)),
    },
    "matmul_sos_49_hessian": {
        "default": ([(("k_sos_split", "full"), 1), (("k_sweep2", "full"), 1)], (4, 2)),
        "scores": ([(("k_sos_split", "full"), 1), (("k_sweep2", "full"), 1)] * 3, (0, 0)),
    },
    "matmul_sos_49_cosine": {
        "default": ([(("k_sweep<float>", "full"), 2)], (4, 2)),
        "scores": ([(("k_sweep<float>", "full"), 6)], (0, 0)),
    },
    "conv_cw_hessian_a32": {
        "default": ([(("k_sweep<float>", "full"), 1)], (2, 1)),
        "scores": ([(("k_sweep<float>", "full"), 3)], (0, 0)),
    },
    "conv_cw_hessian_a8": {
        "default": ([(("k_sweep<float>", "full"), 4)], (2, 4)),
        "scores": ([(("k_sweep<float>", "full"), 6)], (0, 0)),
    },
    "conv_lw_cosine": {
        "default": ([(("k_sweep<float>", "full"), 1)], (2, 1)),
        "scores": ([(("k_sweep<float>", "full"), 3)], (0, 0)),
    },
    "mmblk_qk_hessian_vA2hA2_vB2hB3": {
        "default": ([(("k_sweep_seg", "full"), 30)], (0, 0)),
        "scores": ([(("k_sweep_seg", "full"), 30)], (0, 0)),
    },
    "mmblk_sos_hessian_vB2hB2": {
        "default": ([(("k_sos_split", "full"), 1), (("k_sweep_seg", "full"), 4)] * 3, (0, 0)),
        "scores": ([(("k_sos_split", "full"), 1), (("k_sweep_seg", "full"), 4)] * 3, (0, 0)),
    },
    "mmblk_empty_block": {
        "default": ([(("k_sweep_seg", "full"), 24)], (0, 0)),
        "scores": ([(("k_sweep_seg", "full"), 24)], (0, 0)),
    },
    "convgeo_a_cw_hessian_a8_rect_dil": {
        "default": ([(("k_sweep<float>", "full"), 4)], (2, 4)),
        "scores": ([(("k_sweep<float>", "full"), 6)], (0, 0)),
    },
}

# The cases whose memo must restore for the test to mean anything.  On the parent, by the selections of the "scores" call: the
# dense Linear restores w_interval and a_interval in round 3 (the other Linear seeds were chosen the same way: both post-GELU
# layers and the three cosine layers restore on both sides); the split search restores split + A_interval in rounds 2 and 3
# and B_interval in rounds 2 and 3; the a_bit 32 Conv restores w_interval in rounds 2 and 3 (its input is never searched).
RESTORES = ("linear_hessian_k192_n128", "matmul_sos_49_hessian", "conv_cw_hessian_a32")


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    return engine


def _runs(recs):
    out = []
    for r in recs:
        if out and out[-1][0] == r[:2]:
            out[-1][1] += 1
        else:
            out.append([r[:2], 1])
    return [(k, n) for k, n in out]


def test_every_case_has_an_expectation():
    assert sorted(EXPECTED) == sorted(name for name, _ in CASES)
    assert all(sorted(EXPECTED[name]) == ["default", "scores"] for name in EXPECTED)
    assert all(EXPECTED[name]["default"][1][0] >= 1 for name in RESTORES)


@pytest.mark.parametrize("name,run", CASES, ids=[c[0] for c in CASES])
def test_rounds_launch_and_memoise_as_before(eng, name, run):
    got = {mode: run_case(eng, run, mode) for mode in MODES}
    for mode in MODES:
        print(f"[search rounds] {name} {mode}: memo {got[mode]['memo']} {_runs(got[mode]['records'])}")
    for mode in ("default", "scores"):
        runs, memo = EXPECTED[name][mode]
        assert _runs(got[mode]["records"]) == runs, (name, mode)
        assert got[mode]["memo"] == memo, (name, mode)
    assert got["scores"]["memo"] == (0, 0) and got["nomemo"]["memo"] == (0, 0), name
    for other in ("scores", "nomemo"):
        assert len(got["default"]["intervals"]) == len(got[other]["intervals"])
        for a, b in zip(got["default"]["intervals"], got[other]["intervals"]):
            assert torch.equal(a, b), (name, other, a, b)
    eng.release_workspace()
