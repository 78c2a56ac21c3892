"""tests/prune_reference.py alone satisfies the property the exact candidate pruning claims: on every table whose stage-A scores
are valid bounds, `decide` selects what `full_select` selects from the full totals -- in every branch (synthetic candidate or
not, per-block ranges honoured or not, the host reading the survivors or not, with and without the second tier).  The GPU test
(tests/test_hip_prune_decide.py) then holds the kernels to `decide` literally."""
import numpy as np
import pytest

from tests import prune_reference as ref
from tests.prune_table_cases import BUDGET, CS, NJS, modes_of, tables

CPU_NJS = tuple(nj for nj in NJS if nj <= 257)      # (the larger block counts change nothing for numpy; the GPU test runs them)


def test_first_max_is_torch_argmax():
    S = np.array([[1.0, np.nan, -np.inf, 0.0, -0.0],
                  [3.0, 2.0, -np.inf, -0.0, 0.0],
                  [3.0, np.nan, -np.inf, -1.0, -1.0]], np.float32)
    assert ref.first_max(S).tolist() == [1, 0, 0, 0, 0]
    import torch
    assert torch.argmax(torch.from_numpy(S), 0).tolist() == ref.first_max(S).tolist()


def test_tables_obey_what_the_sweeps_can_produce():
    for C in CS:
        for nj in (1, 3, 65):
            for name, SA, T, SA2 in tables(C, nj, seed=1):
                assert SA.dtype == T.dtype == np.float32 and SA.shape == T.shape == (C, nj), name
                fin = np.isfinite(T)
                assert (SA[fin] >= T[fin] * np.float32(1 + 1.01 * BUDGET)).all(), name      # T <= 0: at most the budget below
                lone_nan = np.isnan(T) & ~np.isnan(SA) & ~np.isnan(T).all(0)[None, :]
                assert not lone_nan.any(), name
                if SA2 is not None:
                    assert ((SA2 >= T) & (SA2 <= SA)).all(), name


@pytest.mark.parametrize("nj", CPU_NJS)
def test_decide_selects_what_the_full_table_selects(nj):
    checked = 0
    for C in CS:
        for name, SA, T, SA2 in tables(C, nj, seed=1):
            want = ref.full_select(T)
            for virt, honour, reads in modes_of(nj):
                for tier2 in ((None, SA2) if SA2 is not None else (None,)):
                    got = ref.decide(SA, T, virt, honour, reads, SA2=tier2)
                    what = (name, C, nj, virt, honour, reads, tier2 is not None)
                    assert np.array_equal(got["sel"], want), what
                    a, b = got["r1"]
                    assert 0 <= a < b <= C, what
                    for r in (got["r2"], got["r3"]):
                        assert r is None or r == ref.EMPTY or 0 <= r[0] < r[1] <= C, what
                    if got["r3"] not in (None, ref.EMPTY):       # the second tier only drops candidates
                        assert got["r2"][0] <= got["r3"][0] and got["r3"][1] <= got["r2"][1], what
                    checked += 1
    assert checked >= len(CS) * 20 * len(modes_of(nj))


def test_the_margin_is_what_keeps_the_rounded_optimum():
    """family h with no margin: the optimum, whose slice sum lies 1.6e-5 below its total, is dropped -- the property above has
    teeth, and the margin is what it rests on"""
    name, SA, T, _ = next(t for t in tables(100, 3, seed=1) if t[0] == "h_rounding")
    keep = ref.MARGIN
    try:
        ref.MARGIN = np.float32(0.0)
        got = ref.decide(SA, T, True, True, False)
    finally:
        ref.MARGIN = keep
    assert not np.array_equal(got["sel"], ref.full_select(T))
    assert np.array_equal(ref.decide(SA, T, True, True, False)["sel"], ref.full_select(T))


def test_an_ambiguous_threshold_is_refused():
    """a stage-A score on the one value where `L - margin * |L|` rounded in two steps and fused disagree: no literal reference"""
    Ls = -np.random.default_rng(3).uniform(0.5, 1.0, 20000).astype(np.float32)
    two, fused = ref._threshold(Ls)
    i = int(np.flatnonzero(two != fused)[0])
    T = np.full((32, 2), -2.0, np.float32)
    T[5] = Ls[i]
    SA = T.copy()
    SA[7, 0] = min(two[i], fused[i])
    with pytest.raises(ref.AmbiguousTable):
        ref.decide(SA, T, False, False, False)
    SA[7, 0] = np.nextafter(min(two[i], fused[i]), np.float32(-4))
    assert np.array_equal(ref.decide(SA, T, False, False, False)["sel"], [5, 5])
