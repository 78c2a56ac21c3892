"""A plain numpy reference of the DECISION of the exact candidate pruning, written from the comments of csrc/p4v_api.hip
(prune_margin, run_pass_pruned_impl) and csrc/p4v_kernels.h (prune_pick, prune_hull, k_merge_*), not from the kernel bodies.

A pass has C candidates and nj score blocks, scored independently.  `T` [C][nj] are the full totals (what the unpruned sweep
computes), `SA` [C][nj] the stage-A scores on the sample slice: upper bounds of T, up to rounding.  The unpruned pass selects
`full_select(T)`; `decide` follows the stages and must select the same whenever SA is a valid bound (tests/
test_prune_reference_cpu.py asserts that on the CPU; the GPU tests hold the kernels to `decide`, ranges included).

The rules:
  winner of block j   = first maximum of SA[:, j] (NaN counts as the maximum, the first NaN wins: torch.argmax)
  r1                  = hull of the winners, [min, max + 1)
  stage B1            = T on r1 for every block (virt: only T[winner_j][j], the synthetic candidate)
  L_j                 = best B1 total of block j (virt: its winner's own total)
  survivor (c, j)     = not (S[c][j] < L_j - margin * |L_j|), in fp32; S = SA, in the second tier SA2 where it was evaluated
  bad                 = a NaN anywhere in S, a NaN among the B1 totals of a block, or an L_j that is not > -inf: everything survives,
                        every range is [0, C)
  non-virt            range = empty if all survivors lie in r1, else hull(survivors) united with r1; every block gets that range
  virt                block j is open iff it has a survivor other than its winner; an open block's range is the hull of ITS
                      survivors, a closed block's is empty; range = hull of the open blocks' ranges, empty if none is open
  stage A2 (optional) SA2 where c lies in the first hull's range (with honour_blk: in the block's own range), -inf elsewhere; the
                      same L, a second hull r3
  stage B2            T where c lies in the last hull's range (with honour_blk: in the block's own range), -inf elsewhere
  merge               non-virt: entries B2 left at -inf take stage B1's; virt: block j's winner takes its B1 total if B2 left it at -inf
  selection           first maximum of the merged table per block
  host_reads          the host reads a hull's range; when it is empty the pass ends there and the B1 totals decide (non-virt: the first
                      maximum of B1's table; virt: every block's winner).  Same selection either way -- the flag picks the branch.
An empty range is written (0, 0)."""
import numpy as np

MARGIN = np.float32(1e-4)          # prune_margin(): max(1e-4, 4 * 2 * PRUNE_FP32_CHAIN * 2^-24)
EMPTY = (0, 0)


class AmbiguousTable(ValueError):
    """a stage-A score within one rounding of its threshold: fp32 `L - margin * |L|` with or without a fused multiply-add would
    decide differently, so the table cannot be held against the kernels literally (the generators avoid these)"""


def first_max(S):
    """per column of S [C][nj]: index of the first maximum, NaN counting as the maximum (the first NaN wins)"""
    S = np.asarray(S)
    nan = np.isnan(S)
    filled = np.where(nan, -np.inf, S)
    return np.where(nan.any(0), nan.argmax(0), filled.argmax(0)).astype(np.int64)


def full_select(T):
    """what the unpruned pass selects: k_select on the full table (include/ptq4vit_hip.h, p4v_score_argmax_gather)"""
    return first_max(np.asarray(T, np.float32))


def _threshold(L):
    """L - margin * |L| in fp32, both ways a compiler may round it"""
    L = np.asarray(L, np.float32)
    with np.errstate(invalid="ignore"):
        two = (L - (MARGIN * np.abs(L)).astype(np.float32)).astype(np.float32)
        fused = (L.astype(np.float64) - np.float64(MARGIN) * np.abs(L).astype(np.float64)).astype(np.float32)
    return two, fused


def _survivors(S, L):
    two, fused = _threshold(L)
    with np.errstate(invalid="ignore"):
        s_two, s_fused = ~(S < two[None, :]), ~(S < fused[None, :])
    if (s_two != s_fused).any():
        raise AmbiguousTable("a stage-A score within one rounding of the threshold")
    return s_two


def _hull_of(mask_1d):
    idx = np.flatnonzero(mask_1d)
    return (int(idx[0]), int(idx[-1]) + 1) if idx.size else EMPTY


def _hull(S, L, b1_nan, winners, r1, virt):
    """one k_prune_hull: (range, per-block ranges [nj][2]) of the scores S against the bounds L"""
    C, nj = S.shape
    surv = _survivors(S, L)
    with np.errstate(invalid="ignore"):
        bad = bool(np.isnan(S).any() or b1_nan.any() or (~(L > -np.inf)).any())
    if bad:
        return (0, C), np.tile(np.array([0, C]), (nj, 1))
    if not virt:
        lo, hi = _hull_of(surv.any(1))
        r = EMPTY if (hi <= lo or (lo >= r1[0] and hi <= r1[1])) else (min(lo, r1[0]), max(hi, r1[1]))
        return r, np.tile(np.array(r), (nj, 1))
    others = surv.copy()
    others[winners, np.arange(nj)] = False
    is_open = others.any(0)
    rblk = np.array([_hull_of(surv[:, j]) if is_open[j] else EMPTY for j in range(nj)]).reshape(nj, 2)
    if not is_open.any():
        return EMPTY, rblk
    return (int(rblk[is_open, 0].min()), int(rblk[is_open, 1].max())), rblk


def _swept(src, rng, rblk, honour_blk):
    """the table a sweep over the candidate range leaves: src inside, -inf outside"""
    C, nj = src.shape
    c = np.arange(C)[:, None]
    inside = (c >= rng[0]) & (c < rng[1]) & np.ones((1, nj), bool)
    if honour_blk:
        inside &= (c >= rblk[None, :, 0]) & (c < rblk[None, :, 1])
    return np.where(inside, src, np.float32(-np.inf)).astype(np.float32)


def decide(SA, T, virt, honour_blk, host_reads, SA2=None):
    """-> dict(sel [nj], winners [nj], r1, r2, r3 (None: no second tier), rblk2, rblk3 [nj][2], exit 0 merge / 1 / 2 ended after
    the first / second hull, tables SB and S2 (None after an early exit))"""
    SA, T = np.asarray(SA, np.float32), np.asarray(T, np.float32)
    C, nj = SA.shape
    assert T.shape == SA.shape and not (virt and nj == 1)
    cols = np.arange(nj)
    winners = first_max(SA)
    r1 = (int(winners.min()), int(winners.max()) + 1)
    if virt:
        L = T[winners, cols]
        b1_nan = np.isnan(L)
        SB = None
    else:
        SB = _swept(T, r1, None, False)
        b1 = SB[r1[0]:r1[1]]
        b1_nan = np.isnan(b1).any(0)
        L = np.where(np.isnan(b1), -np.inf, b1).max(0).astype(np.float32)

    def from_b1():
        return winners.copy() if virt else first_max(SB)
    out = dict(winners=winners, r1=r1, r3=None, rblk3=None, SB=SB, S2=None)
    r2, rblk2 = _hull(SA, L, b1_nan, winners, r1, virt)
    out.update(r2=r2, rblk2=rblk2)
    if host_reads and r2 == EMPTY:
        return dict(out, sel=from_b1(), exit=1)
    rng, rblk = r2, rblk2
    if SA2 is not None:
        SA2m = _swept(np.asarray(SA2, np.float32), r2, rblk2, honour_blk)
        r3, rblk3 = _hull(SA2m, L, b1_nan, winners, r1, virt)
        out.update(r3=r3, rblk3=rblk3)
        if host_reads and r3 == EMPTY:
            return dict(out, sel=from_b1(), exit=2)
        rng, rblk = r3, rblk3
    S2 = _swept(T, rng, rblk, honour_blk)
    if virt:
        at = S2[winners, cols]
        S2[winners, cols] = np.where(at == -np.inf, L, at)
    else:
        S2 = np.where(S2 == -np.inf, SB, S2)
    return dict(out, S2=S2, sel=first_max(S2), exit=0)
