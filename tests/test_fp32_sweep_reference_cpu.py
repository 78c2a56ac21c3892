"""No GPU: the references of tests/fp32_sweep_reference.py against the fp32 oracle, on the two conv shapes the metric grid holds the
fp32 sweep to them (the 8-row patch embedding of tests/sweep_plan_cases.py, K = 768; the 640-row one of tests/pruned_pass_cases.py,
K = 192).

  * the float64 tables (a) and the oracle agree on every argmax;
  * the oracle is within its own SCORE_RTOL of (a);
  * on the 8-row shape the three distances -- oracle to (a), the sequential fp32 emulation (b) to (a), (b) to the oracle -- are the
    ones measured when the bar was introduced (docs/DESIGN_LOG.md), within 20 %: (b) is as far from the oracle as the GPU sweep is,
    which is why the sweep is held to (a) with a bar from (b) and not to the oracle at SCORE_RTOL;
  * with 80 x the rows the emulation's error falls by an order of magnitude and the bar is SCORE_RTOL again."""
import functools

import numpy as np
import pytest

from tests.fp32_sweep_reference import bar, conv_w_tables, rel_err
from tests.helpers import SCORE_RTOL
from tests.sweep_plan_cases import SEARCH, conv_inputs

METRICS = ("L2_norm", "L1_norm", "linear_weighted_L2_norm", "square_weighted_L2_norm", "hessian")
SHAPES = {"conv_patch16_a32": (dict(seed=10), 16), "conv640_a32": (dict(seed=49, images=10, size=64, patch=8), 8)}

# metric -> (oracle vs f64, sequential fp32 vs f64, sequential vs oracle) on conv_patch16_a32
MEASURED = {"L2_norm": (4.0e-5, 1.5e-4, 1.7e-4), "L1_norm": (2.6e-5, 9.7e-5, 1.2e-4),
            "linear_weighted_L2_norm": (6.7e-5, 3.7e-4, 3.2e-4), "square_weighted_L2_norm": (8.1e-5, 4.9e-4, 5.2e-4)}


@functools.lru_cache(maxsize=None)
def tables(shape, metric):
    kw, stride = SHAPES[shape]
    w, b, x, out, grad = (t.numpy() for t in conv_inputs(**kw))
    return conv_w_tables(w, b, x, out, grad, stride=stride, metric=metric, **SEARCH)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_float64_tables_and_the_oracle_agree(shape, metric):
    t = tables(shape, metric)
    assert t["f64"].shape == t["seq32"].shape == t["oracle"].shape == (SEARCH["eq_n"], 16)
    np.testing.assert_array_equal(np.argmax(t["f64"], axis=0), np.argmax(t["oracle"], axis=0))
    assert rel_err(t["oracle"], t["f64"]) <= SCORE_RTOL, (shape, metric, rel_err(t["oracle"], t["f64"]))


@pytest.mark.parametrize("metric", sorted(MEASURED))
def test_the_distances_on_the_eight_row_patch_embedding_are_the_measured_ones(metric):
    t = tables("conv_patch16_a32", metric)
    got = (rel_err(t["oracle"], t["f64"]), rel_err(t["seq32"], t["f64"]), rel_err(t["seq32"], t["oracle"]))
    print(f"[fp32 reference] {metric}: oracle vs f64 {got[0]:.2e}, sequential vs f64 {got[1]:.2e}, sequential vs oracle {got[2]:.2e}")
    for g, want in zip(got, MEASURED[metric]):
        assert abs(g - want) <= 0.2 * want, (metric, got, MEASURED[metric])


@pytest.mark.parametrize("metric", METRICS)
def test_more_rows_average_the_rounding_out(metric):
    (b8, e8), (b640, e640) = bar(tables("conv_patch16_a32", metric)), bar(tables("conv640_a32", metric))
    assert e640 < 0.2 * e8, (metric, e8, e640)
    assert b640 == SCORE_RTOL <= b8 <= 1e-3, (metric, b8, b640)
