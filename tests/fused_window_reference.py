"""CPU reference for stage 1 of the fused int8 WINDOW attention forward (tests/test_hip_fused_window_attention.py,
tests/test_fused_window_reference_cpu.py), built on tests/fused_reference.py: numpy float64 and int64 only, the oracle's
quantisers, nothing of the library under test.  Stages 2 and 3 (the planes, `out`) are fused_reference's, unchanged.

  t64 = Q(q) . Q(k^T), exact in int64, times f64(A_iv) * f64(B_iv)        (q arrives scaled: there is no `* scale`)
  u64 = t64 + bias[head] + mask[window]                                   window = b_ % n_windows; -inf entries allowed
  p64 = softmax(u64) in float64                                           a row of nothing but -inf: NaN, as in torch

The call's probs must satisfy, per row,
    |probs - p64| <= p64 * U_row * 2^-23   wherever p64 >= 2^-100,          0 <= probs <= 2^-99   elsewhere,
    U_row = 10 + N / 64 + 6 * W_row,   W_row = max over the row's keys with p64 >= 2^-100 of max(|t64|, |t64 + bias|, |u64|).
10 + N / 64 is fused_reference's (exp, the division, the final rounding, the pairwise row sum).  The 6: the exponent u - max
goes through FIVE fp32 roundings here -- S1 = A_iv * B_iv, acc * S1, `+ bias`, `+ mask`, u - max -- one more than the plain
chain's four.  Each is at most 2^-24 of the value it rounds: |t| twice, |t + bias|, |u|, |u - max|, none above W_row for a key
that contributes, except |u - max| <= 2 W_row.  That is 6 * 2^-24 W_row in the exponent of the numerator and as much in the
denominator's dominant terms, of which the part common to both cancels: at most 6 * 2^-24 W_row * 2 = 6 W_row ulps of 2^-23 (the
same accounting that gives fused_reference its 5 for four roundings).  Only keys that contribute count: a masked key at -100 has
|u| near 100 and a probability near e^-100 < 2^-100 -- it falls under the second clause and must not loosen the bar of its
row's unmasked keys.  So that the second clause cannot absorb a failure either, `check_window_probs` also asserts that every
entry below 2^-100 is a MASKED entry (mask != 0) of a row that still has an unmasked key."""
import numpy as np

from tests import fused_reference as fr

F32, F64 = np.float32, np.float64


def window_float_stage(q, kT, A_iv, B_iv, A_bit, B_bit, bias, mask=None):
    """dict(t64, tb64, u64, p64 [B_][H][M][N], masked [B_][1][M][N] bool) of the scaled q [B_][H][M][D], kT [B_][H][D][N],
    matmul1's head-wise intervals [H], bias [H][M][N], mask None or [nW][M][N] (B_ % nW == 0, window = b_ % nW)."""
    t64, _ = fr.attn_float_stage(q, kT, A_iv, B_iv, A_bit, B_bit, 1.0)           # (* f64(float32(1.0)): exact)
    B_, H, M, N = t64.shape
    b64 = fr.as_np(bias).astype(F64)
    assert b64.shape == (H, M, N), f"bias {b64.shape} is not {(H, M, N)}"
    tb64 = t64 + b64[None]
    if mask is None:
        u64, masked = tb64, np.zeros((B_, 1, M, N), bool)
    else:
        m64 = fr.as_np(mask).astype(F64)
        nW = m64.shape[0]
        assert m64.shape == (nW, M, N) and B_ % nW == 0, f"mask {m64.shape} for {B_} windows of {(M, N)}"
        per_b = m64[np.arange(B_) % nW][:, None]
        u64, masked = tb64 + per_b, per_b != 0
    with np.errstate(invalid="ignore"):
        e = np.exp(u64 - u64.max(-1, keepdims=True))
        p64 = e / e.sum(-1, keepdims=True)
    return dict(t64=t64, tb64=tb64, u64=u64, p64=p64, masked=masked)


def row_bound_ulps(st):
    """U_row [B_][H][M][1] of a window_float_stage record"""
    p64 = st["p64"]
    N = p64.shape[-1]
    with np.errstate(invalid="ignore"):
        big = ~np.isnan(p64) & (p64 >= fr.P_FLOOR)
        w = np.maximum(np.maximum(np.abs(st["t64"]), np.abs(st["tb64"])), np.abs(st["u64"]))
    W = np.where(big, w, 0.0).max(-1, keepdims=True)
    return 10.0 + N / 64.0 + 6.0 * W


def check_window_probs(probs, st, what):
    """Stage 1 of the window chain; returns (the worst ratio of |probs - p64| to its bound, the share of entries below 2^-100)."""
    probs, p64 = fr.as_np(probs), st["p64"]
    assert probs.shape == p64.shape, f"{what}: probs {probs.shape}, reference {p64.shape}"
    live = ~np.isnan(p64)
    assert np.isnan(probs[~live]).all(), f"{what}: finite probabilities where the reference is NaN"
    assert not np.isnan(probs[live]).any(), f"{what}: NaN probabilities where the reference is finite"
    with np.errstate(invalid="ignore"):
        big = live & (p64 >= fr.P_FLOOR)
        bound = p64 * row_bound_ulps(st) * 2.0 ** -23
    small = live & ~big
    assert (probs[small] >= 0).all() and (probs[small] <= 2.0 ** -99).all(), \
        f"{what}: a probability below 2^-100 came out as {probs[small].max()!r} / {probs[small].min()!r}"
    masked = np.broadcast_to(st["masked"], p64.shape)
    has_unmasked = np.broadcast_to((~masked).any(-1, keepdims=True), p64.shape)
    stray = small & ~(masked & has_unmasked)
    assert not stray.any(), f"{what}: {int(stray.sum())} entries below 2^-100 are no masked entries of a row with an unmasked key"
    if not big.any():
        return 0.0, float(small.mean())
    ratio = np.abs(probs.astype(F64) - p64)[big] / bound[big]
    worst = float(ratio.max())
    assert worst <= 1.0, f"{what}: |probs - p64| is {worst:.3f} of the bound p64 * U_row * 2^-23 ({int((ratio > 1).sum())} entries above)"
    return worst, float(small.mean())


def shift_mask(nW, N, rng, value=-100.0):
    """A Swin-style mask [nW][N][N] of 0 / `value`: the tokens of window w > 0 fall into 2 + w % 2 groups (window 0: one group, no
    masked key) that do not see each other -- symmetric, the diagonal unmasked, different per window."""
    mask = np.zeros((nW, N, N), F32)
    for w in range(nW):
        group = rng.integers(0, 2 + w % 2 if w else 1, size=N)
        mask[w][group[:, None] != group[None, :]] = value
    return mask
