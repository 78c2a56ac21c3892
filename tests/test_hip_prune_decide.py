"""GPU: the decision kernels of the exact candidate pruning -- k_prune_pick, k_prune_hull, k_merge_scores / k_merge_virtual and
k_select, launched by the pruned pass's own launchers in its own order (p4v_debug_prune_decide) -- on adversarial score tables,
against the numpy reference of the decision (tests/prune_reference.py).

The second premise of the pruning: given stage-A scores that are valid upper bounds, the chain selects what k_select selects
from the full table (first maximum, NaN counting as the maximum).  No sweep runs here: stages B1 / A2 / B2 are the tables
k_finish would leave of the full totals T, so every table below is tiny and decides by itself.  For each table:
  * the selection (interval and best_out) equals prune_reference.full_select(T);
  * r1, r2, r3, the per-block ranges of both hulls and the stage-A winners equal prune_reference.decide's literally, as does the
    exit the chain took (no stage B2 after the first / second hull, or merge and k_select).
for virt x honour_blk x host_reads, and with a second-tier SA2 where the family has one.

Sizes (tests/prune_table_cases.py): C in {32, 100, 257, 600} -- 32 is the smallest eligible eq_n, 257 / 600 cross the 256-thread
stride of the candidate loops; nj in {1, 2, 3, 12, 31, 32, 33, 63, 64, 65, 257, 768, 4096} -- around MIR_BLK = 32 (the mirrored
per-block ranges, the hull's own selection), around PRUNE_WIDE_NJ = 64 (one workgroup per block vs one thread per block), past
the thread stride of the wide path, and the cap of plan_prune.  Families a .. m: the module's docstring there.

The calls run on a stream of their own: the null stream has no mapped mirror block, and the host's read of the survivors goes
through the mirror wherever a calibration runs."""
import numpy as np
import pytest
import torch

from tests import prune_reference as ref
from tests.prune_table_cases import NJS, candidate_table, modes_of, sizes_of, tables

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    return engine


@pytest.fixture(scope="module")
def stream():
    return torch.cuda.Stream()


def _pair(r):
    return (-1, -1) if r is None else tuple(int(v) for v in r)


def _blk(r, nj):
    return np.full((nj, 2), -1) if r is None else np.asarray(r)


def _check(eng, stream, name, SA, T, SA2, cands, d_cands, virt, honour, reads):
    C, nj = T.shape
    what = (name, C, nj, "virt" if virt else "non-virt", "honour_blk" if honour else "global range", "host reads" if reads else "device only",
            "tier 2" if SA2 is not None else "one tier")
    want = ref.decide(SA, T, virt, honour, reads, SA2=SA2)
    full = ref.full_select(T)
    assert np.array_equal(want["sel"], full), ("the reference itself", what)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    d_SA, d_T, d_SA2 = dev(SA), dev(T), dev(SA2)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        got = eng.debug_prune_decide(d_SA, d_T, d_cands, virt=virt, honour_blk=honour, host_reads=reads, SA2=d_SA2)
    # the selection: what k_select picks from the full table
    assert np.array_equal(got["best_out"].numpy(), full), (what, got["best_out"].tolist(), full.tolist(), want["r2"], got["r2"])
    assert np.array_equal(got["interval"].numpy(), cands[full, np.arange(nj)]), what
    # the ranges, literally
    assert got["hull_selects"] == (virt or nj <= 32), what
    assert got["r1"] == _pair(want["r1"]), (what, got["r1"], want["r1"])
    assert got["r2"] == _pair(want["r2"]), (what, got["r2"], want["r2"])
    assert got["exit"] == want["exit"], (what, got["exit"], want["exit"])
    assert np.array_equal(got["rblk2"].numpy(), _blk(want["rblk2"], nj)), (what, got["rblk2"].tolist(), want["rblk2"].tolist())
    assert got["r3"] == _pair(want["r3"]), (what, got["r3"], want["r3"])
    assert got["tier2"] == (want["r3"] is not None), what
    assert np.array_equal(got["rblk3"].numpy(), _blk(want["rblk3"], nj)), (what, got["rblk3"].tolist())
    if virt:
        assert np.array_equal(got["best"].numpy(), want["winners"]), (what, got["best"].tolist(), want["winners"].tolist())
    else:
        assert (got["best"].numpy() == -1).all(), what
    if want["r3"] not in (None, ref.EMPTY):
        assert got["r2"][0] <= got["r3"][0] and got["r3"][1] <= got["r2"][1], (what, got["r2"], got["r3"])
    return want["exit"]


@pytest.mark.parametrize("nj", NJS)
def test_decision_kernels_select_what_the_full_table_selects(eng, stream, nj):
    exits, n = set(), 0
    for C in sizes_of(nj):
        cands = candidate_table(C, nj)
        d_cands = torch.from_numpy(cands).cuda()
        for name, SA, T, SA2 in tables(C, nj, seed=1):
            for virt, honour, reads in modes_of(nj):
                for tier2 in ((None, SA2) if SA2 is not None else (None,)):
                    exits.add((_check(eng, stream, name, SA, T, tier2, cands, d_cands, virt, honour, reads), tier2 is not None))
                    n += 1
    print(f"[prune decide] nj {nj}: {n} tables x modes, exits taken {sorted(exits)}")
    # every exit of the chain was taken at this block count: the merge, and the early ends after the first and the second hull
    assert {(0, False), (1, False), (0, True), (2, True)} <= exits, exits
