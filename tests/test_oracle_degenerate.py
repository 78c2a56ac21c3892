"""Zero and non-positive initial intervals on Linear and MatMul, on the CPU: both restatements of the reference (the numpy oracle,
the torch port) against the reference's own runs (tests/golden/degen_*.npz, oracle/gen_golden.py::gen_degenerate).

NaN pattern entry by entry, finite entries within SCORE_RTOL, intervals bit for bit including the sign of a zero, the NaN
pattern of the quantised output.  Every test first asserts the fixture's own premise (tests/degen_cases.py)."""
import os

import numpy as np
import pytest

from oracle.ptq4vit_oracle import LinearOracle, MatMulOracle
from tests.degen_cases import (LINEAR, MATMUL, MMBLK, NAMES, NEG_ZERO, NEGATIVE, assert_fixture_premise, assert_zero_intervals,
                               check_tables, linear_params, matmul_params, same_bits)
from tests.helpers import GOLDEN, load_golden


def test_the_thirteen_fixtures_are_present_and_small():
    """No file larger than the layer fixture it takes its shape from (the largest of those: 61 432 bytes)."""
    assert len(LINEAR) == 9 and len(MATMUL) == 3 and len(MMBLK) == 1 and len(NAMES) == 13, NAMES
    assert NEGATIVE in LINEAR and NEG_ZERO in LINEAR
    for n in NAMES:
        assert os.path.getsize(os.path.join(GOLDEN, n + ".npz")) <= 61432, n
        p = load_golden(n)["params"]
        assert p["eq_alpha"] >= 0.01 and p["search_round"] == 2, n
    kinds = [load_golden(n)["params"] for n in LINEAR]
    assert {p["metric"] for p in kinds} == {"hessian", "cosine", "L2_norm"} and any(p["w_bit"] == 6 for p in kinds)
    assert any(p.get("n_H", 1) == 2 and p["metric"] == "hessian" for p in kinds)
    assert any(p.get("n_a", 1) == 2 and p["metric"] == "cosine" for p in kinds)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_the_case_it_is_named_for(name):
    assert_fixture_premise(load_golden(name), name)


def _check_qf(got, ref, name):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=f"{name} quant_forward NaN pattern")
    m = ~np.isnan(ref)
    np.testing.assert_allclose(got[m], ref[m], rtol=1e-4, atol=1e-5, err_msg=f"{name} quant_forward")


@pytest.mark.parametrize("name", LINEAR)
def test_linear_oracle_reproduces_the_degenerate_run(name):
    g = load_golden(name)
    assert_fixture_premise(g, name)
    o = LinearOracle(g["weight"], g.get("bias"), **linear_params(g))
    with np.errstate(invalid="ignore", divide="ignore"):           # 0 / 0 on purpose
        res = o.calibration_step2(g["x"], g["out"], g["grad"])
        flips = check_tables([(t, None, ref) for (_, t), ref in zip(o.trace, g["scores"])], g, name)
        qf = o.quant_forward(g["x"])
    assert len(o.trace) == len(g["scores"])
    assert_zero_intervals(res["w_interval"], g["w_interval"], name + " w_interval")        # (whatever a near-tie does elsewhere)
    assert_zero_intervals(res["a_interval"], g["a_interval"], name + " a_interval")
    np.testing.assert_array_equal(np.isnan(qf), np.isnan(g["quant_forward"]), err_msg=f"{name} quant_forward NaN pattern")
    if flips == 0:
        same_bits(res["w_interval"], g["w_interval"], name + " w_interval")
        same_bits(res["a_interval"], g["a_interval"], name + " a_interval")
        _check_qf(qf, g["quant_forward"], name)


@pytest.mark.parametrize("name", MATMUL + MMBLK)
def test_matmul_oracle_reproduces_the_degenerate_run(name):
    g = load_golden(name)
    assert_fixture_premise(g, name)
    p = matmul_params(g)
    o = MatMulOracle(**p)
    with np.errstate(invalid="ignore", divide="ignore"):
        res = o.calibration_step2(g["A"], g["B"], g["out"], g["grad"])
        flips = check_tables([(t, None, ref) for (_, t), ref in zip(o.trace, g["scores"])], g, name)
        qf = o.quant_forward(g["A"], g["B"])
    assert len(o.trace) == len(g["scores"])
    assert_zero_intervals(res["A_interval"], g["A_interval"], name + " A_interval")
    assert_zero_intervals(res["B_interval"], g["B_interval"], name + " B_interval")
    np.testing.assert_array_equal(np.isnan(qf), np.isnan(g["quant_forward"]), err_msg=f"{name} quant_forward NaN pattern")
    if flips == 0:
        same_bits(res["A_interval"], g["A_interval"], name + " A_interval")
        same_bits(res["B_interval"], g["B_interval"], name + " B_interval")
        if p["sos"]:
            assert float(res["split"]) == float(g["split"])
        _check_qf(qf, g["quant_forward"], name)


# The torch port restates what the shipped configurations instantiate: n_H = n_a = 1, head-wise MatMul intervals.  The three
# sub-block fixtures (n_H = 2 / n_a = 2 Linear, 2 x 2 MatMul) are outside it, as the linblk_ / mmblk_ fixtures are.
def _port_covers(name):
    p = load_golden(name)["params"]
    return all(p.get(k, 1) == 1 for k in ("n_H", "n_a", "n_V_A", "n_H_A", "n_V_B", "n_H_B"))


@pytest.mark.parametrize("name", [n for n in LINEAR if _port_covers(n)])
def test_torch_port_linear_reproduces_the_degenerate_run(name):
    from oracle.torch_port import TorchLinear
    g = load_golden(name)
    assert_fixture_premise(g, name)
    o = TorchLinear(g["weight"], g.get("bias"), **linear_params(g))
    res = o.calibration_step2(g["x"], g["out"], g["grad"])
    assert len(o.trace) == len(g["scores"])
    assert_zero_intervals(res["w_interval"], g["w_interval"], name + " w_interval")
    assert_zero_intervals(res["a_interval"], g["a_interval"], name + " a_interval")
    if check_tables([(t, None, ref) for (_, t), ref in zip(o.trace, g["scores"])], g, name) == 0:
        same_bits(res["w_interval"], g["w_interval"], name + " w_interval")
        same_bits(res["a_interval"], g["a_interval"], name + " a_interval")


@pytest.mark.parametrize("name", [n for n in MATMUL if _port_covers(n)])
def test_torch_port_matmul_reproduces_the_degenerate_run(name):
    from oracle.torch_port import TorchMatMul
    g = load_golden(name)
    assert_fixture_premise(g, name)
    p = matmul_params(g)
    o = TorchMatMul(**p)
    res = o.calibration_step2(g["A"], g["B"], g["out"], g["grad"])
    assert len(o.trace) == len(g["scores"])
    assert_zero_intervals(res["A_interval"], g["A_interval"], name + " A_interval")
    assert_zero_intervals(res["B_interval"], g["B_interval"], name + " B_interval")
    if check_tables([(t, None, ref) for (_, t), ref in zip(o.trace, g["scores"])], g, name) == 0:
        same_bits(res["A_interval"], g["A_interval"], name + " A_interval")
        same_bits(res["B_interval"], g["B_interval"], name + " B_interval")
        if p["sos"]:
            assert float(res["split"]) == float(g["split"])
