"""GPU: the two premises of the exact candidate pruning on the REAL stage kernels (csrc/p4v_api.hip: prune_margin,
run_pass_pruned_impl, run_sos_split_pruned_impl), with the stage tables of every pruned pass kept (p4v_debug_prune_tables).

The cases are the smallest calibration per branch of the pruned drivers (tests/pruned_pass_cases.py), modes "default" (pass memo
on: the host reads the survivors) and "nomemo".  T, the full totals, is the same call with prune=False, want_scores=True: the
unpruned sweeps' tables, slot [round][side].  tests/test_hip_pruned_stages.py already holds the intervals of the two calls
bit-equal, so pass (round, side) of one call sees the inputs of pass (round, side) of the other.  Every kept record is matched to
its table by (round, side), and the number of records is the `staged` counter.

  Totals.  Every evaluated (!= -inf) entry of stage B1's and stage B2's tables equals T bit for bit (k_merge_scores: "the two
    agree bit for bit") -- except stage B1 of b1_bound passes (k_bound sums in another order), held to 1e-4 |T|, the bar of
    tests/test_hip_bound_kernels.py; where such a B1 entry reaches the merged table (stage B2 did not evaluate it) it is that
    same number.  Stage B2 evaluated every candidate of every block's survivor range.
  Bound.  T - SA <= m |T| for every candidate and block, the same for SA2 where the second tier evaluated it, and SA2 <= SA up to
    the same slack; m <= 1e-4 (prune_margin()).  The worst m per case is recorded.
  Replay.  tests/prune_reference.decide on the kept SA (and SA2) and T reproduces the kept r1 / r2 / r3, per-block ranges,
    winners and the exit the pass took; its selection is full_select(T).  That ties the live run to the spec the decision
    kernels are tested against (tests/test_hip_prune_decide.py).
  Same arithmetic (ZERO_REST_CASES).  With raw_grad exactly zero outside the slice's rows the slice sum and the total are the same
    sum of the same terms: |SA - T| <= 1e-4 |T|, and the ratio of the worst deviation to the 1.6e-5 the comment of prune_margin
    budgets for the order of summation (2 n u, n = PRUNE_FP32_CHAIN) is recorded per pairing of a stage-A kernel with the
    kernel of the totals.  A ratio above 1 means the argument behind the constant does not hold for that pairing.
"""
import functools

import numpy as np
import pytest
import torch

from tests import prune_reference as ref
from tests.helpers import record_margin, record_note
from tests.pruned_pass_cases import CASES, ZERO_REST_CASES, run_case

pytestmark = pytest.mark.gpu

MARGIN = 1e-4                       # prune_margin()
BUDGET = 1.6e-5                     # 2 * PRUNE_FP32_CHAIN * 2^-24: what its comment allows two orders of summation to differ by
MODES = ("default", "nomemo")
RUNS = dict(CASES + [(n, r) for n, r, _ in ZERO_REST_CASES])


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _totals(name):
    """the unpruned call with score tables: [round][side][eq_n][blocks] on the host, and its sweep kernels"""
    from ptq4vit_amd import engine
    got = run_case(engine, functools.partial(RUNS[name], prune=False, want_scores=True), "default")
    assert got["prune_counters"]["staged"] == 0, (name, got["prune_counters"])
    return got["tables"][0].cpu().numpy(), sorted({r[0] for r in got["records"]}), [t.cpu() for t in got["intervals"]]


@functools.lru_cache(maxsize=None)
def _kept(name, mode):
    """the pruned call with the stage tables kept: (records, launch records, prune counters)"""
    from ptq4vit_amd import engine
    engine.debug_prune_tables(start=True)
    try:
        got = run_case(engine, RUNS[name], mode)
    finally:
        recs = engine.debug_prune_tables()
    engine.release_workspace()
    full_iv = _totals(name)[2]
    assert len(got["intervals"]) == len(full_iv) > 0
    for a, b in zip(got["intervals"], full_iv):         # (the tables belong to the same search: same intervals, bit for bit)
        assert torch.equal(a.cpu(), b), (name, mode, a, b)
    return recs, got["records"], got["prune_counters"]


def _matched(name, mode):
    """[(record, T [eq_n][nj], label)]: every kept record with the table of its pass"""
    recs, launches, counters = _kept(name, mode)
    tables, full_kernels, _ = _totals(name)
    assert len(recs) == counters["staged"], (name, mode, len(recs), counters)
    seen, out = set(), []
    for r in recs:
        key = (r["round"], r["side"])
        assert 0 <= r["round"] < tables.shape[0] and r["side"] in (0, 1) and key not in seen, (name, mode, key)
        seen.add(key)
        T = tables[r["round"], r["side"], :r["eq_n"], :r["nj"]]
        assert T.shape == (r["eq_n"], r["nj"]) == tuple(r["SA"].shape), (name, mode, key, T.shape)
        assert r["margin"] == np.float32(MARGIN), r["margin"]
        out.append((r, np.ascontiguousarray(T), f"{name} {mode} round {r['round']} side {r['side']}"))
    stage_a = sorted({k for k, s, _, _ in launches if s == "A"})
    return out, f"A: {' + '.join(stage_a)} | totals: {' + '.join(full_kernels)}"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _rel(num, T):
    """max of num / |T| over the finite entries (0 / 0 counts as 0)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(num == 0, 0.0, num / np.abs(T.astype(np.float64)))
    q = q[np.isfinite(q)]
    return float(q.max()) if q.size else 0.0


# lin650_scores asks for score tables: no pass is eligible.  lin650_flat measures its slice as loose and keeps the full sweeps --
# where the host may read the share (pass memo on); without the memo it cannot know and stages.
STAGED = [n for n, _ in CASES if n != "lin650_scores"]
NOT_STAGED = [("lin650_scores", "default"), ("lin650_scores", "nomemo"), ("lin650_flat", "default")]


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_every_staged_pass_keeps_its_tables(eng, name):
    for mode in MODES:
        matched, pairing = _matched(name, mode)
        recs, _, counters = _kept(name, mode)
        print(f"[prune premises] {name} {mode}: {len(recs)} records, counters {counters}, {pairing}")
        assert (len(matched) == 0) == ((name, mode) in NOT_STAGED), (name, mode, counters)
        for r, T, what in matched:
            assert r["host_read"] == (mode == "default"), what
            assert (r["S2"] is None) == (mode == "default" and r["r3" if r["tier2"] else "r2"] == (0, 0)), what


@pytest.mark.parametrize("name", STAGED)
def test_totals_of_the_stages_are_the_unpruned_totals(eng, name):
    for mode in MODES:
        matched, pairing = _matched(name, mode)
        record_note("kernels", pairing)
        for r, T, what in matched:
            SB, nj, cols = r["SB"].numpy(), r["nj"], np.arange(r["nj"])
            if r["virt"]:
                best = r["best"].numpy()
                assert SB.shape == (1, nj) and ((0 <= best) & (best < r["eq_n"])).all(), what
                sb_full = np.full_like(T, -np.inf)
                sb_full[best, cols] = SB[0]
            else:
                sb_full = SB
                a, b = r["r1"]
                assert (SB[a:b] != -np.inf).all() and (np.delete(SB, np.s_[a:b], 0) == -np.inf).all(), (what, "stage B1 evaluates r1")
            ev = sb_full != -np.inf
            assert ev.any(), what
            if r["b1_bound"]:
                dev = _rel(np.abs(sb_full[ev].astype(np.float64) - T[ev]), T[ev])
                record_margin("k_bound_total_vs_sweep_total", dev)
                print(f"[prune premises] {what}: stage B1 (k_bound) within {dev:.3g} of the sweep's totals")
                assert dev <= MARGIN, (what, dev)
            else:
                assert np.array_equal(_bits(sb_full[ev]), _bits(T[ev])), (what, "stage B1 is not bit-equal to the unpruned sweep", pairing)
            if r["S2"] is None:
                continue
            S2 = r["S2"].numpy()
            rng = r["r3"] if r["tier2"] else r["r2"]
            rblk = (r["rblk3"] if r["tier2"] else r["rblk2"]).numpy() if r["has_rblk"] else np.tile(np.array(rng), (nj, 1))
            c = np.arange(r["eq_n"])[:, None]
            must = (c >= rblk[None, :, 0]) & (c < rblk[None, :, 1])             # the block's own survivors: stage B2 evaluated them
            may = (c >= rng[0]) & (c < rng[1]) & np.ones((1, nj), bool)
            assert not (must & ~may).any(), what
            assert np.array_equal(_bits(S2[must]), _bits(T[must])), (what, "stage B2 left a survivor unevaluated or differs from the sweep", pairing)
            ev2 = S2 != -np.inf
            same = _bits(S2) == _bits(T)
            merged = ev2 & ~must & (_bits(S2) == _bits(sb_full)) & ev               # stage B1's number, where stage B2 evaluated nothing
            assert (~ev2 | same | merged).all(), (what, "an entry of the merged table is neither the sweep's total nor stage B1's", pairing)
            if not r["b1_bound"]:
                assert (~ev2 | same).all(), (what, pairing)


@pytest.mark.parametrize("name", STAGED)
def test_stage_a_scores_are_upper_bounds_of_the_totals(eng, name):
    for mode in MODES:
        matched, pairing = _matched(name, mode)
        record_note("kernels", pairing)
        for r, T, what in matched:
            SA = r["SA"].numpy()
            assert np.isfinite(SA).all() and np.isfinite(T).all(), what
            m = _rel(T.astype(np.float64) - SA, T)
            record_margin("m_stage_A", m)
            record_margin(f"m_stage_A_side{r['side']}", m)
            print(f"[prune premises] {what}: worst T - SA = {m:.3g} |T| ({pairing})")
            assert m <= MARGIN, (what, m, pairing)
            if r["SA2"] is not None:
                SA2 = r["SA2"].numpy()
                ev = SA2 != -np.inf
                assert ev.any(), what
                m2 = _rel(T[ev].astype(np.float64) - SA2[ev], T[ev])
                over = _rel(SA2[ev].astype(np.float64) - SA[ev], T[ev])
                record_margin("m_stage_A2", m2)
                record_margin("m_A2_above_A", over)
                print(f"[prune premises] {what}: worst T - SA2 = {m2:.3g} |T|, worst SA2 - SA = {over:.3g} |T|")
                assert m2 <= MARGIN and over <= MARGIN, (what, m2, over)


@pytest.mark.parametrize("name", STAGED)
def test_replaying_the_kept_tables_through_the_reference_gives_the_kept_ranges(eng, name):
    tier2_seen = False
    for mode in MODES:
        matched, _ = _matched(name, mode)
        for r, T, what in matched:
            SA2 = r["SA2"].numpy() if r["SA2"] is not None else None
            want = ref.decide(r["SA"].numpy(), T, r["virt"], False, r["host_read"], SA2=SA2)     # (SA2 is kept as swept: already ranged)
            assert np.array_equal(want["sel"], ref.full_select(T)), what
            assert r["r1"] == want["r1"] and r["r2"] == want["r2"], (what, r["r1"], r["r2"], want["r1"], want["r2"])
            if r["has_rblk"]:
                assert np.array_equal(r["rblk2"].numpy(), want["rblk2"]), (what, r["rblk2"].tolist(), want["rblk2"].tolist())
            if r["virt"]:
                assert np.array_equal(r["best"].numpy(), want["winners"]), what
            if r["tier2"]:
                tier2_seen = True
                assert r["r3"] == want["r3"], (what, r["r3"], want["r3"])
                assert np.array_equal(r["rblk3"].numpy(), want["rblk3"]), what
                if r["r3"] != (0, 0):
                    assert r["r2"][0] <= r["r3"][0] and r["r3"][1] <= r["r2"][1], what
            else:
                assert r["r3"] == (-1, -1) and SA2 is None, what
            assert (r["S2"] is None) == (want["exit"] != 0), (what, want["exit"])
            assert r["hull_selects"] == (r["split_search"] or r["virt"] or r["nj"] <= 32), what
    assert tier2_seen == (name == "lin2048_tier2"), name


@pytest.mark.parametrize("name,pairing", [(n, p) for n, _, p in ZERO_REST_CASES], ids=[n for n, _, _ in ZERO_REST_CASES])
def test_slice_sum_and_total_are_the_same_arithmetic(eng, name, pairing):
    """raw_grad zero outside the slice (asserted on the host by the case): the stage-A score IS the total, up to the arithmetic"""
    worst = 0.0
    for mode in MODES:
        matched, kernels = _matched(name, mode)
        assert matched, (name, mode)
        record_note("kernels", kernels)
        for r, T, what in matched:
            exact = "SA2" if name == "lin2048_tier2_zero_rest" else "SA"           # (the second slice holds all of the weight there)
            if r[exact] is None:
                continue
            S = r[exact].numpy()
            ev = S != -np.inf
            dev = _rel(np.abs(S[ev].astype(np.float64) - T[ev]), T[ev])
            worst = max(worst, dev)
            record_margin(f"m_stage_{exact[1:]}", _rel(T[ev].astype(np.float64) - S[ev], T[ev]))      # signed: how far BELOW the total
            record_margin(f"zero_rest_ratio_to_budget_side{r['side']}", dev / BUDGET)
            print(f"[prune premises] {what}: |{exact} - T| <= {dev:.3g} |T| = {dev / BUDGET:.3f} of the summation budget ({pairing}; {kernels})")
            assert dev <= MARGIN, (what, dev, pairing)
    record_margin("zero_rest_deviation", worst)
    record_margin("zero_rest_ratio_to_budget", worst / BUDGET)
    if name == "lin2048_tier2_zero_rest":
        assert any(r["tier2"] for mode in MODES for r, _, _ in _matched(name, mode)[0]), "the second tier did not run"
