"""GPU: the pruned drivers of csrc/p4v_api.hip (plan_prune, run_pass_pruned, run_sos_split_pruned: eligibility, slice tiers,
stage passes, survivor read-backs) -- the smallest shape per branch (tests/pruned_pass_cases.py), three search rounds each.

Asserted per case and mode ("default": memo on, the host reads the survivors; "nomemo": it does not, stage B2 always runs;
"xcheck": the engine follows every pruned pass with its full sweep and compares): the folded (kernel, stage) sequence of the
launch records, the four prune counters (staged, staged_no_survivors, kept_full_sweep, not_eligible) and the pass memo's (hits,
misses); for the two 4 137-row layers also stage A's grid_x, which tells the quarter slice from the full one.  The expected values are what the commit BEFORE the drivers were rebuilt around PrunePlan / PruneBufs / the stage
builders / read_survivors produced for the same table on an MI355X (tools/plan_dump.py --gpu,
profiles/r18_calls_parent_gpu.json); they are literals, not derived from the code under test.  A sequence that changes here
means a stage was added, dropped or moved, a counter that changes means a pass was planned differently: a behaviour change, not
a refactor.
Also asserted: the intervals of every mode are bit-equal to those of the same call with prune=False (full sweeps only), and the
"xcheck" call returns without the engine's own mismatch error.

The cases above are hessian.  test_pruned_passes_under_the_metrics_that_read_no_raw_grad runs the forced ones under the four
other difference metrics, with and without a raw_grad (tests/pruned_pass_cases.py, METRIC_CASES): those metrics read raw_out alone
(include/ptq4vit_hip.h, d_grad), so the tensor must change nothing.
"""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import record_margin
from tests.pruned_pass_cases import CASES, GRADS_GIVEN, METRIC_CASES, metric_case, metric_oracle, modes_of, run_case

pytestmark = pytest.mark.gpu

A, B1, B2, A2, FULL = "A", "B1", "B2", "A2", "full"



def _r(kernel, *stages):
    """one record per stage, the same kernel"""
    return [((kernel, s), 1) for s in stages]


S6, S2, S5, S8, S9, SF = "k_sweep6", "k_sweep2", "k_sweep4/5", "k_sweep8", "k_sweep9", "k_sweep<float>"
KB1 = _r("k_bound", B1)
SLA, SLB, SOS = _r("k_slice_a", A), _r("k_slice_b", A), "k_sos_split"

# case -> mode -> ([((kernel, stage), count)] runs of the launch records, prune counters, (memo hits, memo misses))
EXPECTED = {
    "lin650_cls": {
        "default": ((_r(S6, A) + KB1) * 3, (3, 3, 0, 0), (3, 3)),
        "nomemo": ((_r(S6, A) + KB1 + _r(S6, B2)) * 6, (6, 0, 0, 0), (0, 0)),
        "xcheck": ((_r(S6, A) + KB1 + _r(S6, FULL)) * 3, (3, 3, 0, 0), (3, 3)),
    },
    "lin650_flat": {           # (without the memo the host never measures the slice: nothing tells the module it is loose)
        "default": ([((S6, FULL), 3)], (0, 0, 3, 0), (3, 3)),
        "nomemo": ((_r(S6, A) + KB1 + _r(S6, B2)) * 6, (6, 0, 0, 0), (0, 0)),
    },
    "lin650_flat_forced": {
        "default": ((_r(S6, A) + KB1 + _r(S6, B2)) * 3, (3, 0, 0, 0), (3, 3)),
        "nomemo": ((_r(S6, A) + KB1 + _r(S6, B2)) * 6, (6, 0, 0, 0), (0, 0)),
    },
    "lin650_nV3": {
        "default": ((_r(S2, A) + KB1) * 3 + _r(S2, B2) + _r(S2, A) + KB1, (4, 3, 0, 0), (2, 4)),
        "nomemo": ((_r(S2, A) + KB1 + _r(S2, B2)) * 6, (6, 0, 0, 0), (0, 0)),
        "xcheck": ((_r(S2, A) + KB1 + _r(S2, FULL)) * 2 + _r(S2, A) + KB1 + _r(S2, B2, FULL) + _r(S2, A) + KB1 + _r(S2, FULL),
                   (4, 3, 0, 0), (2, 4)),
    },
    "postgelu650": {           # (the fold pass between the two searches is a full sweep; the twin's stage B2 runs without the memo)
        "default": ((_r(S2, A, B1, FULL) + _r(S6, A) + KB1) * 2 + _r(S2, A, B1), (5, 5, 0, 0), (1, 5)),
        "nomemo": ((_r(S2, A, B1, B2, FULL) + _r(S6, A) + KB1 + _r(S6, B2)) * 3, (6, 0, 0, 0), (0, 0)),
    },
    "lin4137_quarter": {
        "default": ((_r(S5, A) + KB1) * 6, (6, 6, 0, 0), (0, 6)),
        "nomemo": ((_r(S5, A) + KB1 + _r(S5, B2)) * 6, (6, 0, 0, 0), (0, 0)),
    },
    "lin4137_spread": {
        "default": ((_r(S5, A) + KB1 + _r(S5, B2)) * 2 + _r(S5, A) + KB1, (3, 1, 0, 0), (3, 3)),
        "nomemo": ((_r(S5, A) + KB1 + _r(S5, B2)) * 6, (6, 0, 0, 0), (0, 0)),
    },
    "lin2048_tier2": {         # (the second tier needs the survivor count: never without the memo)
        "default": ((_r(S8, A) + KB1 + _r(S8, A2, B2)) * 4, (4, 0, 0, 0), (2, 4)),
        "nomemo": ((_r(S8, A) + KB1 + _r(S8, B2)) * 6, (6, 0, 0, 0), (0, 0)),
    },
    "qk65": {
        "default": ((SLA + _r(S9, B1) + SLB + _r(S9, B1)) * 2 + _r(S9, B2), (4, 3, 0, 0), (2, 4)),
        "nomemo": ((SLA + _r(S9, B1, B2) + SLB + _r(S9, B1, B2)) * 3, (6, 0, 0, 0), (0, 0)),
        "xcheck": ((SLA + _r(S9, B1, FULL) + SLB + _r(S9, B1, FULL)) + SLA + _r(S9, B1, FULL) + SLB + _r(S9, B1, B2, FULL),
                   (4, 3, 0, 0), (2, 4)),
    },
    "qk65_d128": {
        "default": (_r(S2, A, B1) * 5, (5, 5, 0, 0), (1, 5)),
        "nomemo": (_r(S2, A, B1, B2) * 6, (6, 0, 0, 0), (0, 0)),
    },
    "sos65": {
        "default": (_r(SOS, A, B1) + SLB + _r(S2, B1), (2, 2, 0, 0), (4, 2)),
        "nomemo": ((_r(SOS, A, B1, B2) + SLB + _r(S2, B1, B2)) * 3, (6, 0, 0, 0), (0, 0)),
        "xcheck": (_r(SOS, A, B1, FULL) + SLB + _r(S2, B1, FULL), (2, 2, 0, 0), (4, 2)),
    },
    "conv640_a32": {
        "default": (_r(SF, A, B1, B2), (1, 0, 0, 0), (2, 1)),
        "nomemo": (_r(SF, A, B1, B2) * 3, (3, 0, 0, 0), (0, 0)),
    },
    "conv640_a8": {            # (its activation search runs on fp32 planes and is not handed to the pruned driver)
        "default": (_r(SF, A, B1, B2, FULL) * 2, (2, 0, 0, 0), (2, 4)),
        "nomemo": (_r(SF, A, B1, B2, FULL) * 3, (3, 0, 0, 0), (0, 0)),
    },
    "lin650_scores": {
        "default": ([((S6, FULL), 6)], (0, 0, 0, 6), (0, 0)),
        "nomemo": ([((S6, FULL), 6)], (0, 0, 0, 6), (0, 0)),
    },
}

# case -> (kernel, stage) records its literals must hold / must not hold: the branch the case is there for
MUST_REACH = {
    "lin650_cls": dict(has=[("k_bound", B1)], lacks_stage=[B2, FULL]),
    "lin650_flat": dict(lacks_stage=[A, B1, B2, A2], kept_full_sweep=True),
    "lin650_flat_forced": dict(has_stage=[A, B1, B2]),
    "lin650_nV3": dict(has=[("k_bound", B1)]),
    "postgelu650": dict(has=[("k_sweep2", A), ("k_sweep2", B1)], nomemo_has=[("k_sweep2", B2)]),    # k_sweep2: the twin's sweep
    "lin4137_quarter": dict(has_stage=[A, B1], stage_a_tiles=1),      # stage A's grid_x: 128-row tiles of the slice in use
    "lin4137_spread": dict(has_stage=[A, B1], stage_a_tiles=4),       # (the full slice: 512 rows)
    "lin2048_tier2": dict(has_stage=[A, B1, A2]),
    "qk65": dict(has=[("k_slice_a", A), ("k_slice_b", A)]),
    "qk65_d128": dict(has=[("k_sweep2", A)], lacks=[("k_slice_a", A), ("k_slice_b", A)]),
    "sos65": dict(has=[("k_sos_split", A), ("k_sos_split", B1), ("k_slice_b", A)]),
    "conv640_a32": dict(has_stage=[A, B1]),
    "conv640_a8": dict(has_stage=[A, B1]),
    "lin650_scores": dict(lacks_stage=[A, B1, B2, A2], not_eligible=True),
}


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
    assert sorted(EXPECTED) == sorted(name for name, _ in CASES) == sorted(MUST_REACH)
    assert MUST_REACH["lin4137_quarter"]["stage_a_tiles"] < MUST_REACH["lin4137_spread"]["stage_a_tiles"]
    for name, _ in CASES:
        assert sorted(EXPECTED[name]) == sorted(modes_of(name)), name
        runs, (staged, no_survivors, kept_full, not_eligible), _ = EXPECTED[name]["default"]
        recs = [k for k, _ in runs]
        stages = {s for _, s in recs}
        want = MUST_REACH[name]
        assert all(r in recs for r in want.get("has", ())), name
        assert not any(r in recs for r in want.get("lacks", ())), name
        assert all(s in stages for s in want.get("has_stage", ())), name
        assert not any(s in stages for s in want.get("lacks_stage", ())), name
        assert all(r in [k for k, _ in EXPECTED[name]["nomemo"][0]] for r in want.get("nomemo_has", ())), name
        if want.get("kept_full_sweep"):
            assert staged == 0 and kept_full > 0 and not_eligible == 0, name
        elif want.get("not_eligible"):
            assert staged == 0 and kept_full == 0 and not_eligible > 0, name
        else:
            assert staged > 0, name
        # without the memo the host does not read the survivors: stage B2 is always launched, no pass is counted as "no survivors"
        runs, counters, memo = EXPECTED[name]["nomemo"]
        assert memo == (0, 0) and counters[1] == 0, name
        assert counters[0] == 0 or B2 in {s for (_, s), _ in runs}, name


@pytest.mark.parametrize("name,run", CASES, ids=[c[0] for c in CASES])
def test_pruned_passes_launch_and_count_as_before(eng, name, run):
    for mode in modes_of(name):
        got = run_case(eng, run, mode)           # ("xcheck": an engine-side mismatch raises here)
        full = run_case(eng, functools.partial(run, prune=False), mode)
        counters = tuple(got["prune_counters"][k] for k in ("staged", "staged_no_survivors", "kept_full_sweep", "not_eligible"))
        print(f"[pruned stages] {name} {mode}: prune {counters} memo {got['memo']} {_runs(got['records'])}")
        runs, want_counters, memo = EXPECTED[name][mode]
        assert _runs(got["records"]) == runs, (name, mode)
        assert counters == want_counters, (name, mode)
        assert got["memo"] == memo, (name, mode)
        if mode == "default" and "stage_a_tiles" in MUST_REACH[name]:
            assert {r[2] for r in got["records"] if r[1] == A} == {MUST_REACH[name]["stage_a_tiles"]}, (name, got["records"])
        assert len(got["intervals"]) == len(full["intervals"]) > 0
        for a, b in zip(got["intervals"], full["intervals"]):
            assert torch.equal(a, b), (name, mode, a, b)
    eng.release_workspace()


@functools.lru_cache(maxsize=None)
def _metric_oracle(name, metric):
    return metric_oracle(name, metric)


@pytest.mark.parametrize("name,metric", METRIC_CASES, ids=[f"{n}-{m}" for n, m in METRIC_CASES])
def test_pruned_passes_under_the_metrics_that_read_no_raw_grad(eng, name, metric):
    """The forced cases under L2_norm, L1_norm and the two raw_out-weighted metrics, in every mode, with no raw_grad, with the
    case's own and with the adversarial one: each call staged its passes, its intervals are bit-identical to the full sweeps'
    (prune=False) -- so to each other -- and the full sweeps' intervals are the numpy oracle's at the bar of tests/helpers.py (the
    oracle's, or the neighbouring entry of the same candidate table)."""
    from tests.helpers import assert_on_candidate_grid, candidate_grid
    from tests.pruned_pass_cases import ROUNDS
    full = run_case(eng, functools.partial(metric_case(name, metric, False), prune=False), "default")
    assert full["prune_counters"]["staged"] == 0, (name, metric, full["prune_counters"])
    want, sos = _metric_oracle(name, metric)
    mult = candidate_grid(ROUNDS["eq_alpha"], ROUNDS["eq_beta"], ROUNDS["eq_n"])
    assert len(full["intervals"]) == len(want)
    for k, (got, ref) in enumerate(zip(full["intervals"], want)):
        if ref is None:
            continue
        got, ref = got.cpu().numpy().reshape(-1), np.asarray(ref, dtype=np.float32).reshape(-1)
        if sos and k != 1:        # the split and A_interval = split / (q - 1): powers of two, not entries of the candidate grid
            np.testing.assert_array_equal(got, ref, err_msg=f"{name} {metric} interval {k}")
        else:
            assert_on_candidate_grid(got, ref, mult, f"{name} {metric} interval {k} (full sweeps against the oracle)")
    for mode in modes_of(name):
        for given in GRADS_GIVEN:
            got = run_case(eng, metric_case(name, metric, given), mode)       # ("xcheck": an engine-side mismatch raises here)
            what = (name, metric, mode, f"grad_given={given}")
            print(f"[pruned stages] {what}: prune {got['prune_counters']} {_runs(got['records'])}")
            assert got["prune_counters"]["staged"] > 0, what
            assert len(got["intervals"]) == len(full["intervals"]) > 0
            for a, b in zip(got["intervals"], full["intervals"]):
                assert torch.equal(a, b), (what, a, b)
    eng.release_workspace()


def _row_share(mass, k):
    """share of the k heaviest rows in a float64 row mass"""
    return float(torch.topk(mass, k).values.sum() / mass.sum())


@pytest.mark.parametrize("metric,staged", [("square_weighted_L2_norm", True), ("linear_weighted_L2_norm", False)])
def test_the_slice_is_ranked_and_measured_by_the_metrics_own_weight(eng, metric, staged):
    """k_row_mass: o^2 per row under square_weighted_L2_norm ((o d)^2), |o| under linear_weighted_L2_norm (|o| d^2).  A 650-row
    Linear whose ten class-token rows are four times as large: its 256 heaviest rows hold 0.57 of sum o^2 and 0.46 of sum |o|
    (asserted here in float64, with room on both sides of the engine's threshold 0.5).  So the module is staged under the
    square-weighted metric and keeps the full sweep under the linear-weighted one -- with the two masses exchanged it is the
    other way round.  No variant bit: the engine's own decision (k_mass_fraction).  The intervals equal the unpruned search's."""
    from tests.pruned_pass_cases import ROUNDS, _call, _cuda
    from tests.sweep_plan_cases import linear_inputs
    w, b, x, _, _ = linear_inputs(192, 96, seed=41, images=10, tokens=65)
    x[:, 0] *= 4.0
    out = torch.nn.functional.linear(x, w, b)
    o = out.double().reshape(-1, out.shape[-1])
    share_sq, share_abs = _row_share((o ** 2).sum(-1), 256), _row_share(o.abs().sum(-1), 256)
    print(f"[pruned stages] the 256 heaviest of 650 rows hold {share_sq:.4f} of sum o^2 and {share_abs:.4f} of sum |o|")
    record_margin("slice_share_of_o_squared", share_sq)
    record_margin("slice_share_of_abs_o", share_abs)
    assert share_sq >= 0.55 and share_abs <= 0.47, (share_sq, share_abs)

    def run(eng, mode, prune=True):
        job = eng.linear_job(weight=_cuda(w), bias=_cuda(b), x=_cuda(x), out=_cuda(out), grad=None, w_bit=8, a_bit=8, metric=metric,
                             n_V=1, n_H=1, n_a=1, prune=prune, **ROUNDS)
        return _call(eng, job, mode)
    got = run_case(eng, run, "default")
    full = run_case(eng, functools.partial(run, prune=False), "default")
    c = got["prune_counters"]
    print(f"[pruned stages] {metric}: prune {c} {_runs(got['records'])}")
    if staged:
        assert c["staged"] > 0 and c["kept_full_sweep"] == 0 and c["not_eligible"] == 0, (metric, c)
    else:
        assert c["staged"] == 0 and c["kept_full_sweep"] > 0 and c["not_eligible"] == 0, (metric, c)
    for a, b_ in zip(got["intervals"], full["intervals"]):
        assert torch.equal(a, b_), (metric, a, b_)
    eng.release_workspace()
