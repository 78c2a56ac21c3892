"""Adversarial score tables for the decision of the exact candidate pruning, shared by tests/test_prune_reference_cpu.py (the
reference alone selects what the full table selects) and tests/test_hip_prune_decide.py (the kernels do what the reference does).

A table is (name, SA, T, SA2 or None): fp32 [C][nj], scores are MINUS sums of non-negative terms, so T <= 0, and the tables obey
what the sweeps can produce: SA >= T up to rounding (a partial sum of the same terms), and a NaN in T[c][j] comes with a NaN in
SA[c][j] or with a block of T that is NaN throughout.  Families (the letters of the docstring of test_hip_prune_decide.py):
  a tight bound  b loose bound  c exact ties at the maximum, the earlier index not the stage-A winner  d a stage-A winner that is
  not the optimum  e optimum at c = 0 / c = C - 1  f blocks with disjoint survivor ranges  g every block closed / some open / all
  open (virt)  h SA below T by 1.6e-5 relative on the optimum  i one block of T all NaN, with and without NaN in SA  j one NaN
  candidate  k one block of totals all -inf  l L = 0 with SA in {0, -0}  m a second-tier SA2 between SA and T"""
import numpy as np

CS = (32, 100, 257, 600)            # 32: the smallest eligible eq_n; 257, 600: past the 256-thread stride
NJS = (1, 2, 3, 12, 31, 32, 33, 63, 64, 65, 257, 768, 4096)      # MIR_BLK = 32, PRUNE_WIDE_NJ = 64, the thread stride, the cap
BUDGET = 1.6e-5                     # 2 n u, n = PRUNE_FP32_CHAIN: what the margin's comment allows the two sums to disagree by


def sizes_of(nj):
    """the candidate counts a block count is run with: all four up to 65 blocks, two each (rotating) for the large tables"""
    if nj <= 65:
        return CS
    return {257: (32, 600), 768: (100, 257), 4096: (32, 100)}[nj]


def _base(rng, C, nj):
    """totals in [-2, -1] with the optimum of every block lifted to -0.5 at a random candidate: gaps far above the margin"""
    T = -rng.uniform(1.0, 2.0, (C, nj)).astype(np.float32)
    opt = rng.integers(0, C, nj)
    T[opt, np.arange(nj)] = -0.5
    return T, opt


def _loose(rng, T, lo=0.3):
    return (T * rng.uniform(lo, 1.0, T.shape).astype(np.float32)).astype(np.float32)      # T <= 0: u T >= T


def tables(C, nj, seed):
    rng = np.random.default_rng([seed, C, nj])
    cols = np.arange(nj)
    jm = nj // 2                                           # the block the single-block families act on
    out = []
    T, opt = _base(rng, C, nj)
    out.append(("a_tight", T.copy(), T, None))
    out.append(("b_loose", _loose(rng, T), T, None))
    # c: T ties at the maximum in c1 < c2; c2 wins stage A (its bound is loose, c1's is tight)
    T, _ = _base(rng, C, nj)
    c1, c2 = rng.integers(0, C // 2, nj), rng.integers(C // 2, C, nj)
    T[T == -0.5] = -1.0
    T[c1, cols] = -0.5
    T[c2, cols] = -0.5
    SA = T.copy()
    SA[c2, cols] = -0.25
    out.append(("c_ties", SA, T, None))
    # d: the stage-A winner w is a poor candidate with a very loose bound
    T, opt = _base(rng, C, nj)
    w = (opt + 1 + rng.integers(0, C - 1, nj)) % C
    T[w, cols] = -2.0
    SA = T.copy()
    SA[w, cols] = -0.3
    out.append(("d_wrong_winner", SA, T, None))
    # e: the optimum at the first / the last candidate, alternating over the blocks (and the other way round)
    for k, first in enumerate(("e_ends_0", "e_ends_1")):
        T, _ = _base(rng, C, nj)
        T[T == -0.5] = -1.0
        at = np.where((cols + k) % 2 == 0, 0, C - 1)
        T[at, cols] = -0.5
        out.append((first, _loose(rng, T, 0.6), T, None))
    # f: block j's near-optimal candidates form a band of three at a place of its own; everything else is far below
    T = -rng.uniform(10.0, 20.0, (C, nj)).astype(np.float32)
    start = (cols * 7) % (C - 3)
    for d in range(3):
        T[start + d, cols] = -1.0 - 1e-5 * ((d + cols) % 3)
    out.append(("f_disjoint", T.copy(), T, None))
    # g: tight bounds and gaps above the margin close every block; loose bounds on every other block / on all open them
    T, _ = _base(rng, C, nj)
    out.append(("g_closed", T.copy(), T, None))
    SA = np.where((cols % 2 == 0)[None, :], T, _loose(rng, T))
    out.append(("g_some_open", SA.astype(np.float32), T, None))
    out.append(("g_all_open", _loose(rng, T, 0.3), T, None))
    # h: the optimum's slice sum lies BELOW the bound by the rounding the margin is there for: w wins stage A with a total
    # 1e-5 worse than the optimum's, the optimum's stage-A score is 1.6e-5 below its own total
    T, opt = _base(rng, C, nj)
    w = (opt + 1 + rng.integers(0, C - 1, nj)) % C
    T[w, cols] = np.float32(-0.5 * (1 + 1e-5))
    SA = T.copy()
    SA[opt, cols] = np.float32(-0.5 * (1 + BUDGET))
    out.append(("h_rounding", SA, T, None))
    # i: one block of T all NaN -- SA NaN throughout, NaN in one entry, finite
    T, _ = _base(rng, C, nj)
    Tn = T.copy()
    Tn[:, jm] = np.nan
    SA = _loose(rng, T)
    for name, rows in (("i_nan_block_sa_all", slice(None)), ("i_nan_block_sa_one", C // 3), ("i_nan_block_sa_none", None)):
        S = SA.copy()
        if rows is not None:
            S[rows, jm] = np.nan
        out.append((name, S, Tn, None))
    # j: one NaN candidate in SA and T (two of them in the block: the first wins)
    Tn, S = T.copy(), SA.copy()
    for c in (C // 2, C - 2):
        Tn[c, jm] = np.nan
        S[c, jm] = np.nan
    out.append(("j_nan_candidate", S, Tn, None))
    # k: one block whose totals are all -inf, its stage-A scores -inf as well / finite
    Tk = T.copy()
    Tk[:, jm] = -np.inf
    S = SA.copy()
    S[:, jm] = -np.inf
    out.append(("k_inf_block_sa_inf", S, Tk, None))
    out.append(("k_inf_block_sa_finite", SA.copy(), Tk, None))
    # l: a block whose best total is 0 (as -0 in the first candidate, +0 later) under stage-A scores of 0 and -0
    Tl, S = T.copy(), SA.copy()
    Tl[0, jm], Tl[C // 2, jm] = -0.0, 0.0
    S[:, jm] = np.where(np.arange(C) % 2 == 0, 0.0, -0.0)
    out.append(("l_zero", S.astype(np.float32), Tl, None))
    # m: the second tier's scores halfway between the slice's and the totals
    T, _ = _base(rng, C, nj)
    SA = _loose(rng, T, 0.3)
    SA2 = (T * np.float32(0.5) + SA * np.float32(0.5)).astype(np.float32)
    SA2 = np.minimum(np.maximum(SA2, T), SA)
    out.append(("m_tier2_loose", SA, T, SA2))
    out.append(("m_tier2_tight", SA.copy(), T, T.copy()))
    # ... and a second tier that closes the pass: one candidate is the optimum of every block and wins stage A, the loose slice
    # keeps many others, the exact SA2 none
    T = -rng.uniform(1.0, 2.0, (C, nj)).astype(np.float32)
    T[C // 3] = -0.5
    SA = _loose(rng, T, 0.2)
    SA[C // 3] = -0.1
    out.append(("m_tier2_closes", SA, T, T.copy()))
    return out


def modes_of(nj):
    """(virt, honour_blk, host_reads): the synthetic candidate needs several score blocks"""
    return [(v, h, r) for v in ((False, True) if nj > 1 else (False,)) for h in (False, True) for r in (False, True)]


def candidate_table(C, nj):
    """[C + 1][nj], every entry another value (exact in fp32)"""
    return (np.arange((C + 1) * nj, dtype=np.float32) + np.float32(0.5)).reshape(C + 1, nj)
