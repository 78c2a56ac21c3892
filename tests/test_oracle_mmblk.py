"""MatMul row / column sub-blocks (n_V, n_H > 1) on the CPU: the numpy oracle against the reference's own fixtures
(tests/golden/mmblk_*.npz, tools/gen_golden_mmblk.py), the exchange slot of such a module, the block geometry.

Bar as in tests/test_oracle_golden.py: every score table the reference fed to argmax within SCORE_RTOL, selections equal or
near-ties by the reference's own scores, and -- with no differing selection -- intervals bit-identical and the quantised
output to fp32 GEMM noise."""
import numpy as np
import pytest
import torch

from oracle.ptq4vit_oracle import MatMulOracle
from tests.helpers import assert_argmax_tie_aware, assert_scores_close, golden_names, load_golden

NAMES = golden_names("mmblk_")


def test_the_eight_fixtures_are_present():
    assert len(NAMES) == 8 and sum(n.startswith("mmblk_ptqsl_") for n in NAMES) == 2, NAMES


@pytest.mark.parametrize("name", NAMES)
def test_matmul_blocks_oracle_matches_reference(name):
    g = load_golden(name)
    p = dict(g["params"])
    batching = p.pop("kind") == "matmul"
    o = MatMulOracle(batching=batching, **p)
    res = o.calibration_step2(g["A"], g["B"], g["out"], g["grad"] if p["metric"] == "hessian" else None)
    assert len(o.trace) == len(g["scores"]), f"{name}: {len(o.trace)} searches vs {len(g['scores'])}"
    flips = 0
    for i, ((tag, mine), ref) in enumerate(zip(o.trace, g["scores"])):
        assert_scores_close(mine, ref, what=f"{name}[{i}:{tag}]")
        flips += assert_argmax_tie_aware(np.argmax(mine.reshape(ref.shape), axis=0), ref, what=f"{name}[{i}:{tag}]")
    if flips == 0:
        np.testing.assert_array_equal(np.asarray(res["A_interval"]).reshape(-1), g["A_interval"].reshape(-1))
        np.testing.assert_array_equal(res["B_interval"], g["B_interval"])
        if p["sos"]:
            assert float(res["split"]) == float(g["split"])
        np.testing.assert_allclose(o.quant_forward(g["A"], g["B"]), g["quant_forward"], rtol=1e-4, atol=1e-5)


def test_fixture_interval_shapes_and_the_empty_block():
    for name in NAMES:
        g = load_golden(name)
        p = g["params"]
        H = g["A"].shape[1]
        nGB = p.get("n_G_B", 1) if p["kind"] == "ptqsl_matmul" else H
        assert g["B_interval"].shape == (1, nGB, 1, p.get("n_V_B", 1), 1, p.get("n_H_B", 1), 1), name
        if not p["sos"]:
            nGA = p.get("n_G_A", 1) if p["kind"] == "ptqsl_matmul" else H
            assert g["A_interval"].shape == (1, nGA, 1, p.get("n_V_A", 1), 1, p.get("n_H_A", 1), 1), name
    g = load_golden("mmblk_empty_block")
    # M = 5 in 4 row blocks of 2: the fourth holds padding only; N = 5 in 4 column blocks likewise
    assert np.all(g["A_interval"][0, :, 0, 3] == 0) and np.all(g["A_interval"][0, :, 0, :3] > 0)
    assert np.all(g["B_interval"][0, :, 0, 0, 0, 3] == 0) and np.all(g["B_interval"][0, :, 0, 0, 0, :3] > 0)
    assert not any(np.isnan(t).any() for t in g["scores"]) and not np.isnan(g["quant_forward"]).any()


def test_slot_capacity_counts_sub_block_intervals():
    from ptq4vit_amd.quant_layers.matmul import PTQSLBatchingQuantMatMul, SoSPTQSLBatchingQuantMatMul
    from ptq4vit_amd.utils.shard import _slot_capacity
    assert _slot_capacity(PTQSLBatchingQuantMatMul()) == 2 * 128 + 2                      # (1, 1, 1, 1): unchanged
    assert _slot_capacity(SoSPTQSLBatchingQuantMatMul()) == 2 * 128 + 2
    m = PTQSLBatchingQuantMatMul(n_V_A=2, n_H_A=3, n_V_B=4, n_H_B=1)
    assert _slot_capacity(m) == 128 * 6 + 128 * 4 + 2
    s = SoSPTQSLBatchingQuantMatMul(n_V_A=2, n_H_A=2, n_V_B=2, n_H_B=2)               # the class forces n_V_A = n_H_A = 1
    assert _slot_capacity(s) == 128 + 128 * 4 + 2
    m._p4v_interval_slots = 77
    assert _slot_capacity(m) == 77


def test_padding_parameters_of_ragged_and_empty_blocks():
    """Reference matmul.py:109-122: blocks of ceil(dim / n), the rest is zero padding -- a whole block of it where
    (n - 1) * ceil(dim / n) >= dim."""
    from ptq4vit_amd.quant_layers.matmul import PTQSLBatchingQuantMatMul, PTQSLQuantMatMul
    m = PTQSLBatchingQuantMatMul(n_V_A=2, n_H_A=2, n_V_B=2, n_H_B=3)
    m._get_padding_parameters(torch.zeros(4, 3, 13, 8), torch.zeros(4, 3, 8, 13))
    assert (m.n_G_A, m.n_G_B) == (3, 3)
    assert (m.crb_rows_A, m.crb_cols_A, m.pad_rows_A, m.pad_cols_A) == (7, 4, 1, 0)          # rows 7 / 6
    assert (m.crb_rows_B, m.crb_cols_B, m.pad_rows_B, m.pad_cols_B) == (4, 5, 0, 2)          # columns 5 / 5 / 3
    e = PTQSLQuantMatMul(n_G_A=2, n_G_B=2, n_V_A=4, n_H_B=4)
    e._get_padding_parameters(torch.zeros(2, 3, 5, 8), torch.zeros(2, 3, 8, 5))
    assert (e.crb_groups_A, e.pad_groups_A) == (2, 1)                                        # 2 groups of 3 heads: a padding head
    assert (e.crb_rows_A, e.pad_rows_A) == (2, 3) and e.pad_rows_A >= e.crb_rows_A           # rows 2 / 2 / 1 / 0: an empty block
    assert (e.crb_cols_B, e.pad_cols_B) == (2, 3)
    # the torch formulation of quant_forward crops the padding again, whatever the empty block's interval is
    e.A_interval = torch.ones(1, 2, 1, 4, 1, 1, 1)
    e.A_interval[..., 3, :, :, :] = 0
    x = torch.randn(2, 3, 5, 8)
    q = e.quant_input_A(x)
    assert q.shape == x.shape and torch.isfinite(q).all()
