"""GPU: the twelve sweep-family shapes of tests/sweep_plan_cases.py under the four difference metrics that no other bit-wise check
runs (tests/metric_grid_cases.py): L2_norm, L1_norm, linear_weighted_L2_norm, square_weighted_L2_norm.  The metric selects the
epilogue instance of every sweep kernel and the metric weight of its prologue (csrc/p4v_kernels.h: EpiMode, metric_weight,
metric_add / metric_add_masked), so each (shape, metric) pair is another set of kernel instances.

Every pair runs with raw_grad = None and again with a raw_grad GIVEN: the generator's own, then -- on the pruned shape -- the
adversarial one of sweep_plan_cases.grad_of (1 / (|raw_out| + 1e-3): finite, the ranking of the elements reversed), on the
others an all-NaN one (the pruned passes answer NaN with "sweep everything", which would hide a bound taken from the wrong
tensor; a full sweep has no such way out).  None of these metrics may read raw_grad (include/ptq4vit_hip.h, d_grad): intervals,
score tables, selections and the (kernel, stage) sequence must be the same, bit for bit.

The raw_grad = None run is asserted per pair:
  * the numpy oracle at the bar of tests/helpers.py: every score table within SCORE_RTOL, every selection the oracle's argmax or a
    near-tie by the oracle's own scores (TIE_RTOL), every interval the oracle's or another entry of the same candidate table
    (the pruned 650-row layer returns no tables: its intervals alone, against the oracle's tables);
  * where the sweep records are k_sweep<float> (fp32 operands, fp32 MFMAs over K: the patch embedding with an unquantised input)
    the tables are held to the FLOAT64 tables of tests/fp32_sweep_reference.py instead, at max(SCORE_RTOL, 2 x the error of a
    sequential fp32 emulation of the same case and metric) -- computed here, on the CPU, not stored; the selections to the
    float64 argmax or a tie by the float64 table.  test_fp32_sweep_against_float64 adds hessian at that shape and the 640-row
    conv of tests/pruned_pass_cases.py under all five metrics, where the ratio to the bar must not rise;
  * the (kernel, stage) sequence of the sweep records: literals, what the library of the commit before the epilogue vocabulary
    (DESIGN.md s5 "epilogue vocabulary") produced on an MI355X (tools/plan_dump.py --gpu, profiles/r25_calls_parent_gpu.json);
    the two weighted rows of the pruned shape are what the library BEFORE the weight-source rule produced for the call with
    raw_grad = None (profiles/r26_grid_parent_gpu.json) -- with a raw_grad it took the bound of stage B1 from that tensor.
The margins go where the suite's recorder writes them (tests/helpers.py; profiles/r26_metric_weight_margins.json)."""
import functools

import numpy as np
import pytest
import torch

from tests import fp32_sweep_reference as f32ref
from tests.helpers import assert_argmax_tie_aware, assert_on_candidate_grid, assert_scores_close, candidate_grid, record_margin
from tests.metric_grid_cases import CASES, IDS, METRICS, oracle
from tests.sweep_plan_cases import SEARCH, SHAPES, conv_inputs, run_case

pytestmark = pytest.mark.gpu

_A_B1_B2 = [("k_sweep6", "A"), ("k_bound", "B1"), ("k_sweep6", "B2")]
WEIGHTED = ("linear_weighted_L2_norm", "square_weighted_L2_norm")

# shape -> [(kernel, stage)] of every sweep record; a dict where the metric changes the sequence.  Otherwise the rows are those
# of tests/test_hip_sweep_plan.py (hessian).
EXPECTED = {
    "linear_k192_n128": [("k_sweep6", "full")] * 2,
    "linear_k128_n128": [("k_sweep4/5", "full")] * 2,
    "linear_k1024_n64": [("k_sweep7", "full")] * 2,
    # post-GELU: the weight search on the twin instance, the fold of the negative plane; the activation search is a k_sweep7
    # record under the unweighted metrics only
    "postgelu_k1024_n64": {m: [("k_sweep7 (twin)", "full"), ("k_sweep2", "full")] + ([] if m in WEIGHTED else [("k_sweep7", "full")])
                           for m in METRICS},
    "linear_k1088_n64": [("k_sweep2g", "full"), ("k_sweep2", "full")],
    "linear_k192_n120_nV3": [("k_sweep<int8>", "full")] * 2,
    "matmul_qk_49": [("k_sweep9", "full")] * 2,
    "matmul_qk_120": [("k_sweep8", "full")] * 2,
    "matmul_sos_49": [("k_sos_split", "full"), ("k_sweep2", "full")],
    "conv_patch16_a32": [("k_sweep<float>", "full")],
    # the pruned passes: stage B2 sweeps the survivors under every metric.  (With a raw_grad the library before the weight-source
    # rule ended the two weighted rows after stage B1, "no survivors": its bound was a total weighted with raw_grad, 1e-11 against
    # scores of 1e-3.  The rows here are its records for raw_grad = None.)
    "bound_650x96_k192": _A_B1_B2 * 2,
    "mmblk_qk_hessian_vA2hA2_vB2hB3": [("k_sweep_seg", "full")] * 20,
}

PARAMS = [pytest.param(*c, id=i) for c, i in zip(CASES, IDS)]
FP32_SWEEP = [("k_sweep<float>", "full")]


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    return engine


def test_the_grid_is_the_twelve_shapes_times_the_four_metrics():
    assert len(CASES) == 48 and len(set(IDS)) == 48
    assert sorted(EXPECTED) == sorted(s[0] for s in SHAPES)
    assert {(n, m) for n, m, _, _ in CASES} == {(s[0], m) for s in SHAPES for m in METRICS}
    assert [(n, p) for n, _, _, p in CASES[::4]] == [(s[0], s[3]) for s in SHAPES]        # each shape keeps its pruning setting


def _tables(got_scores, got_best, refs, what):
    """engine tables [R][steps][C][blocks] / selections against the oracle's tables, pass by pass; returns the differing selections"""
    R, steps = got_scores.shape[:2]
    per_round = len(refs) // R          # (the patch embedding with an unquantised input: one pass of its two table slots)
    assert per_round * R == len(refs) and 1 <= per_round <= steps, (what, got_scores.shape, len(refs))
    flips = 0
    for i, ref in enumerate(refs):
        ref = np.asarray(ref).reshape(ref.shape[0], -1)
        got, best = got_scores[i // per_round, i % per_round], got_best[i // per_round, i % per_round]
        assert_scores_close(got[: ref.shape[0], : ref.shape[1]], ref, what=f"{what}[pass {i}]")
        flips += assert_argmax_tie_aware(best[: ref.shape[1]], ref, what=f"{what}[pass {i}]")
    return flips


CONV_SHAPES = {"conv_patch16_a32": (dict(seed=10), 16), "conv640_a32": (dict(seed=49, images=10, size=64, patch=8), 8)}


@functools.lru_cache(maxsize=None)
def _f64_tables(shape, metric):
    """the float64 / sequential-fp32 / oracle tables of a conv shape's weight search (host only)"""
    kw, stride = CONV_SHAPES[shape]
    w, b, x, out, grad = (t.numpy() for t in conv_inputs(**kw))
    return f32ref.conv_w_tables(w, b, x, out, grad, stride=stride, metric=metric, **SEARCH)


def _fp32_tables(scores, best, shape, metric, what):
    """the one table of an fp32 sweep against the float64 table at the emulation's bar; returns (differing selections, error / bar)"""
    t = _f64_tables(shape, metric)
    bar, seq_err = f32ref.bar(t)
    got = scores[0, 0][: t["f64"].shape[0], : t["f64"].shape[1]]
    err = f32ref.rel_err(got, t["f64"])
    print(f"[metric grid] {what}: fp32 sweep vs float64 {err:.3e}, vs the oracle {f32ref.rel_err(got, t['oracle']):.3e}; sequential fp32 vs float64 "
          f"{seq_err:.3e}; bar {bar:.3e}, ratio {err / bar:.2f}")
    record_margin("fp32_sweep_rel_err_vs_float64", err)
    record_margin("fp32_sweep_ratio_to_bar", err / bar)
    assert_scores_close(got, t["f64"], rtol=bar, what=f"{what} (float64 tables)")
    return assert_argmax_tie_aware(best[0, 0][: t["f64"].shape[1]], t["f64"], what=f"{what} (float64 tables)"), err / bar


def _same_bits(a, b, what):
    """two runs of a case: the same tensors bit for bit (NaN included), the same (kernel, stage, grid) records"""
    (res_a, recs_a), (res_b, recs_b) = a, b
    assert len(res_a) == len(res_b), what
    for k, (x, y) in enumerate(zip(res_a, res_b)):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: result tensor {k} differs:\n{x.ravel()[:8]}\n{y.ravel()[:8]}"
    assert recs_a == recs_b, (what, recs_a, recs_b)


@pytest.mark.parametrize("name,metric,run,pruned", PARAMS)
def test_metric_pair(eng, name, metric, run, pruned):
    res, recs, launches, _ = run_case(eng, run, prune=pruned, grad="none")
    print(f"[metric grid] {name} {metric}: {[r[:2] for r in recs]} ({launches['issued']} launches)")
    res = [t.cpu().numpy() for t in res]
    what = f"{name} {metric}"
    # raw_grad given: nothing may move
    for kind in ("seeded", "adversarial" if pruned else "nan"):
        res_g, recs_g, _, _ = run_case(eng, run, prune=pruned, grad=kind)
        _same_bits((res, recs), ([t.cpu().numpy() for t in res_g], recs_g), f"{what}: raw_grad = None against the {kind} raw_grad")
    ref = oracle(name, metric)
    n_iv = len(ref["intervals"])
    got_iv, tables = res[:n_iv], res[n_iv:]
    search = ref.get("search", SEARCH)
    mult = candidate_grid(search["eq_alpha"], search["eq_beta"], search["eq_n"])
    flips = 0
    if pruned:
        assert not tables, "a pruned call returns no tables"
    elif [r[:2] for r in recs] == FP32_SWEEP:
        scores, best = tables
        flips, _ = _fp32_tables(scores, best, name, metric, what)
    else:
        scores, best = tables
        flips = _tables(scores, best, ref["tables"], what)
    # intervals: the oracle's, or another entry of the same candidate table (further than one entry only on a tie by the oracle's
    # own table of the pass that chose it: single-block passes, where that table is known by position)
    moved = 0
    for k, (got, want) in enumerate(zip(got_iv, ref["intervals"])):
        if want is None:                       # not searched (the unquantised input of the patch embedding)
            continue
        want = np.asarray(want, dtype=np.float32).reshape(-1)
        if ref["sos"] and k != 1:
            # the split and A_interval = split / (q - 1) come from the power-of-two table, not from the candidate grid
            if flips == 0:
                np.testing.assert_array_equal(got.reshape(-1), want, err_msg=f"{what} interval {k}")
            continue
        last = ref["tables"][-1] if ref["sos"] else ref["tables"][k] if len(ref["tables"]) <= n_iv else None
        moved += assert_on_candidate_grid(got, want, mult, f"{what} interval {k}", ref_scores=last)
    if not pruned and flips == 0:
        assert moved == 0, f"{what}: same selections but {moved} different intervals"
    want_recs = EXPECTED[name][metric] if isinstance(EXPECTED[name], dict) else EXPECTED[name]
    assert [r[:2] for r in recs] == want_recs, (what, recs)


@functools.lru_cache(maxsize=None)
def _fp32_ratio(shape, metric):
    """one weight search of a conv shape with score tables (no pruning: a k_sweep<float> full sweep) against the float64 table;
    (error / bar, differing selections)"""
    from ptq4vit_amd import engine
    kw, stride = CONV_SHAPES[shape]
    w, b, x, out, grad = (t.cuda() for t in conv_inputs(**kw))
    engine.stats_reset()
    engine.stats_enable(True)
    try:
        _, _, scores, best = engine.conv_calibrate(weight=w, bias=b, x=x, out=out, grad=grad, stride=(stride, stride), padding=(0, 0), dilation=(1, 1),
                                                   w_bit=8, a_bit=32, metric=metric, prune=False, want_scores=True, **SEARCH)
        torch.cuda.synchronize()
        engine.stats_get()
        recs = [(r["kernel"], r["stage"]) for r in engine.stats_launches()]
    finally:
        engine.stats_enable(False)
    assert recs == FP32_SWEEP, (shape, metric, recs)
    flips, ratio = _fp32_tables(scores.cpu().numpy(), best.cpu().numpy(), shape, metric, f"{shape} {metric}")
    return ratio, flips


@pytest.mark.parametrize("metric", METRICS + ("hessian",))
def test_fp32_sweep_against_float64(eng, metric):
    """the fp32 sweep at 8 rows x K = 768 and at 640 rows x K = 192 against the float64 tables, hessian included.  More rows
    average the rounding of the single outputs out, so the sweep's error must fall RELATIVE to its bar -- although the 640-row
    bar is already the floor SCORE_RTOL.  A ratio that rises says that something other than rounding is at work."""
    r8, _ = _fp32_ratio("conv_patch16_a32", metric)
    r640, _ = _fp32_ratio("conv640_a32", metric)
    record_margin("fp32_sweep_ratio_to_bar_8_rows", r8)
    record_margin("fp32_sweep_ratio_to_bar_640_rows", r640)
    assert r8 <= 1.0 and r640 <= 1.0                    # (each asserted against its bar in _fp32_tables already)
    assert r640 <= r8, (metric, r8, r640)
    eng.release_workspace()
