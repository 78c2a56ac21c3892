"""GPU: stage B1 of a pruned Linear pass -- k_bound with the 64 x 64 wave tile (the default path) against the kernel it replaced
(64 x 32 per wave, kept behind tuning 12 = 4), at the smallest shapes where the new tiling can go wrong.

A wave of the new kernel owns BOTH 32-column groups of a 64-column slab and writes one partial sum per group into the table
k_finish reads, where the old kernel had one wave per group.  What can break: the B-fragment offsets of the second group, the
slot index, a slab whose second group is pure padding (N = 32, 96, 800), the 128 x 128 workgroup tile on row counts that are no
multiple of 64 / 128, the counted waits with one, three and twelve k-tiles (8 loads per tile instead of 6), and the early returns
of a launch whose chunk of the candidate plane does not hold the bound's candidate.

The engine prunes a Linear only where the 256-row slice is at most 40 % of its samples (run_pass_pruned: 640 rows), so the row
counts 65 / 130 / 394 are the tokens per image of 10 images: 650, 1300 and 3940 rows -- 10, 20 and 36 rows into the last 64-row
slab, 11, 21 and 62 slabs, the last 128-row tile half empty or not.  The metrics whose weight is not concentrated on a few
rows are pruned under variant 8388608 (prune even where the slice's bounds are loose), on both sides of every comparison.

Bars.  The B1 totals of the two kernels may differ by prune_margin() * |total| (1e-4: csrc/p4v_api.hip, the deviation the
exactness argument of the pruning allows the bound); selections and intervals must be bit-identical between pruning on, off and
the engine's own cross-check (variant 134217728), on the new kernel and on the old one.
test_every_metric_with_and_without_bias_and_column_blocks also ties the totals to the numpy oracle: see _bound_is_a_score.
"""
import functools
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import SCORE_RTOL, record_margin

pytestmark = pytest.mark.gpu

SEARCH = dict(eq_alpha=0.01, eq_beta=1.2, eq_n=100)
PRUNE_MARGIN = 1e-4                  # p4v_api.hip::prune_margin()
LOOSE, NO_PRUNE, CROSSCHECK = 8388608, 4194304, 134217728
B1_PREVIOUS = 4                      # tuning key 12: stage B1 on the previous kernel
METRICS = ("hessian", "L1_norm", "L2_norm", "linear_weighted_L2_norm", "square_weighted_L2_norm")
IMAGES = 10


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    return engine


def _host_layer(T, N, K, bias, seed, images=IMAGES):
    """host tensors of one layer"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(images, T, K, generator=g)
    x[:, 0] *= 4.0                                        # class-token rows: heavy in raw_out too (the raw_out-weighted metrics)
    w = torch.randn(N, K, generator=g) * 0.05 * torch.linspace(0.6, 1.5, N)[:, None]
    b = torch.randn(N, generator=g) * 0.1 if bias else None
    out = F.linear(x, w, b)
    grad = torch.randn(out.shape, generator=g) * 1e-10
    grad[:, 0] *= 300.0 * torch.exp(torch.randn(images, 1, generator=g))
    return dict(weight=w, bias=b, x=x, out=out, grad=grad)


def _layer(T, N, K, bias, seed, metric, images=IMAGES, grad_given=False):
    """tensors of one layer on the GPU; raw_grad for the hessian metric, as the quant layers pass it, and for any other metric
    with `grad_given`: the engine reads raw_grad if and only if the metric is hessian (include/ptq4vit_hip.h, d_grad), so under
    the other metrics the tensor changes nothing -- stage B1 weights its total with raw_out there."""
    t = _host_layer(T, N, K, bias, seed, images)
    if metric != "hessian" and not grad_given:
        t["grad"] = None
    return {k: None if v is None else v.cuda() for k, v in t.items()}


def _run(eng, args, variant=0, b1_path=0, prune=True, totals=False):
    """one calibration; returns (intervals, launch records as (kernel, stage), B1 totals or None)"""
    eng.debug_variant(variant)
    eng.debug_tuning(12, b1_path)
    eng.stats_reset()
    eng.stats_enable(True)
    if totals:
        eng.debug_bound_totals(start=True)
    try:
        res = eng.linear_calibrate(**args) if prune else eng.linear_calibrate(prune=False, **args)
        torch.cuda.synchronize()
        eng.stats_get()
        recs = [(r["kernel"], r["stage"], r["grid_x"]) for r in eng.stats_launches()]
    finally:
        kept = eng.debug_bound_totals() if totals else None
        eng.stats_enable(False)
        eng.debug_tuning(12, 0)
        eng.debug_variant(0)
    return [t.detach().clone() for t in res[:2]], recs, kept


def _check(eng, args, what, expect_b1_launches=None):
    new, recs_new, tot_new = _run(eng, args, LOOSE, 0, totals=True)
    old, recs_old, tot_old = _run(eng, args, LOOSE, B1_PREVIOUS, totals=True)
    full, recs_full, _ = _run(eng, args, 0, 0, prune=False)
    chk, _, _ = _run(eng, args, LOOSE | CROSSCHECK, 0)
    chk_old, _, _ = _run(eng, args, LOOSE | CROSSCHECK, B1_PREVIOUS)
    b1_new = [r for r in recs_new if r[:2] == ("k_bound", "B1")]
    b1_old = [r for r in recs_old if r[:2] == ("k_bound", "B1")]
    # no silent fall-back: both paths ran k_bound as stage B1, the unpruned call none of it, and the new grid is the 128 x 128 one
    assert b1_new and len(b1_new) == len(b1_old), (what, recs_new, recs_old)
    assert not [r for r in recs_full if r[0] == "k_bound"], (what, recs_full)
    assert all(2 * a[2] == b[2] for a, b in zip(b1_new, b1_old)), (what, b1_new, b1_old)
    if expect_b1_launches is not None:
        assert len(b1_new) >= expect_b1_launches, (what, len(b1_new))
    assert tot_new and len(tot_new) == len(tot_old), (what, tot_new, tot_old)
    worst = max(abs(a - b) / max(abs(b), 1e-300) for a, b in zip(tot_new, tot_old))
    print(f"[bound] {what}: {len(b1_new)} k_bound launches, {len(tot_new)} B1 totals, worst relative deviation {worst:.3g}")
    for a, b in zip(tot_new, tot_old):
        assert abs(a - b) <= PRUNE_MARGIN * abs(b), (what, a, b)
    for k in (0, 1):
        assert torch.equal(new[k], full[k]), (what, k, new[k], full[k])
        assert torch.equal(new[k], old[k]) and torch.equal(new[k], chk[k]) and torch.equal(new[k], chk_old[k]), (what, k)


_SHAPES = list(itertools.product((65, 130, 394), (32, 96, 800), (64, 192, 768)))


def _case(i):
    T, N, K = _SHAPES[i]
    n_V = 3 if (N == 96 and i % 2 == 0) else 1             # (n_V = 3 needs N % 3 == 0 and whole 32-column groups per block: N = 96)
    return T, N, K, n_V, bool((i // 2) % 2), METRICS[i % len(METRICS)]


@pytest.mark.parametrize("i", range(len(_SHAPES)), ids=lambda i: "T{}-N{}-K{}-nV{}-bias{:d}-{}".format(*_case(i)))
def test_wide_k_bound_matches_the_previous_kernel_and_the_unpruned_search(eng, i):
    T, N, K, n_V, bias, metric = _case(i)
    args = dict(_layer(T, N, K, bias, 700 + i, metric), w_bit=8, a_bit=8, n_V=n_V, n_H=1, n_a=1, search_round=1, metric=metric, **SEARCH)
    _check(eng, args, f"{IMAGES} x {T} rows, N {N}, K {K}, n_V {n_V}, bias {bias}, {metric}")


@functools.lru_cache(maxsize=None)
def _oracle_tables(metric, n_V, bias):
    """the numpy oracle's score tables of the 650-row layer, one round: [weight search [100][n_V], activation search [100]]"""
    from oracle.ptq4vit_oracle import LinearOracle
    t = {k: None if v is None else v.numpy() for k, v in _host_layer(65, 96, 192, bias, 900 + n_V).items()}
    o = LinearOracle(t["weight"], t["bias"], w_bit=8, a_bit=8, metric=metric, n_V=n_V, search_round=1, **SEARCH)
    o.calibration_step2(t["x"], t["out"], t["grad"] if metric == "hessian" else None)
    return [np.asarray(tab, dtype=np.float64) for _, tab in o.trace]


def _bound_is_a_score(total, table, what):
    """The soundness premise of the pruning: the bound of stage B1 is the score that some candidate really has, over ALL samples.
    So a B1 total of a single-block pass lies within SCORE_RTOL of an entry of the oracle's table of that pass, and does not
    exceed the table's maximum by more than SCORE_RTOL |max| (scores are negated errors: the maximum is the best).  A total
    weighted with another tensor than the metric's is off by orders of magnitude."""
    table = table.reshape(-1)
    dist = float(np.min(np.abs(table - total) / np.abs(table)))
    over = (total - table.max()) / abs(table.max())
    print(f"[bound] {what}: B1 total {total:.6e}, nearest oracle entry {dist:.3e} away, table maximum {table.max():.6e}")
    record_margin("b1_total_to_nearest_oracle_entry", dist)
    assert dist <= SCORE_RTOL, (what, total, dist)
    assert over <= SCORE_RTOL, (what, total, table.max())


@pytest.mark.parametrize("metric,n_V,bias", [(m, v, b) for m in METRICS for v, b in ((1, False), (3, True))])
def test_every_metric_with_and_without_bias_and_column_blocks(eng, metric, n_V, bias):
    """each of the five difference metrics (four epilogues) with n_V in {1, 3} and with / without bias, at one shape with padding
    in rows (650 = 10 slabs + 10 rows) and columns (96 = one slab and a half); the metrics that read no raw_grad without one and
    with one (grad_given): intervals and B1 totals must be the same, bit for bit.  Stage B1 is also tied to the numpy oracle
    (_bound_is_a_score): the totals of the single-block passes -- with n_V = 1 both searches, with n_V = 3 the activation search,
    the last total."""
    tabs = _oracle_tables(metric, n_V, bias)
    seen = []
    for grad_given in ((True,) if metric == "hessian" else (False, True)):
        what = f"650 rows, N 96, K 192, n_V {n_V}, bias {bias}, {metric}, grad_given {grad_given}"
        args = dict(_layer(65, 96, 192, bias, 900 + n_V, metric, grad_given=grad_given), w_bit=8, a_bit=8, n_V=n_V, n_H=1, n_a=1, search_round=1,
                    metric=metric, **SEARCH)
        _check(eng, args, what)
        iv, _, totals = _run(eng, args, LOOSE, 0, totals=True)
        if n_V == 1:
            assert len(totals) == 2, (what, totals)
            _bound_is_a_score(totals[0], tabs[0], what + ", weight search")
        _bound_is_a_score(totals[-1], tabs[1], what + ", activation search")
        seen.append((iv, totals))
    for iv, totals in seen[1:]:
        assert totals == seen[0][1], (metric, n_V, bias, totals, seen[0][1])
        assert all(torch.equal(a, b) for a, b in zip(iv, seen[0][0])), (metric, n_V, bias)


def test_chunked_candidate_plane_runs_the_early_returns(eng):
    """The activation search's candidate plane (100 x 16 640 rows x 768 B = 1.19 GiB) above a 1 GiB plane budget (tuning 7 = 1):
    the pass runs in two chunks, stage B1 launches k_bound once per chunk, and the launch whose chunk does not hold the bound's
    candidate returns at once (crange / c1) -- its table entries must come from the other launch alone."""
    args = dict(_layer(394, 32, 768, True, 990, "hessian", images=42), w_bit=8, a_bit=8, n_V=1, n_H=1, n_a=1, search_round=1, metric="hessian", **SEARCH)
    eng.debug_tuning(7, 1)
    try:
        _check(eng, args, "42 x 394 rows, N 32, K 768, chunked plane", expect_b1_launches=3)   # w search 1 + a search 2 chunks
    finally:
        eng.debug_tuning(7, 0)
        eng.release_workspace()
