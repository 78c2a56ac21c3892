"""No GPU: the float64 stage-1 reference of the fused window attention forward (tests/fused_window_reference.py) and its bar, held
against an fp32 emulation of the kernel's chain on the CPU -- S1 = A_iv * B_iv, float(acc) * S1, `+ bias`, `+ mask`, the true row
maximum, exp(u - max) in fp32, a pairwise fp32 row sum, the fp32 division -- over bias std 0.02 ... 4, q x 1 ... 6, Swin-style
0 / -100 masks, one fully masked row, -inf masks, N = 49 and 144, D = 12 and 32.  The emulation's exp is numpy's, not the GPU's: the
bar's 8 ulp for exp and the division cover either.  And the bar itself: it refuses a probability that is off by more than U_row
ulps, a masked key at -100 does not loosen the bar of its row, an entry below 2^-100 that is not a masked one is refused.

With P4V_FUSED_WATTN_OUT set the emulation's worst ratio is written there, under "emulation" (profiles/r26_fused_wattn_margins.json).
"""
import os

import numpy as np
import pytest

from tests import fused_reference as fr
from tests import fused_window_reference as fw
from tests.fused_common import merge_margins

F32 = np.float32
_MARGINS = {}
#        id                  B_  nW  H   N    D   bias std  q factor  mask
CASES = [("w7_quiet",        8,  4,  3,  49,  32, 0.02,     1.0,      "shift"),
         ("w7_nomask",       8,  4,  3,  49,  32, 0.5,      2.0,      None),
         ("w7_peaked",       8,  4,  3,  49,  32, 4.0,      6.0,      "shift"),
         ("w7_d12",          8,  4,  2,  49,  12, 1.0,      3.0,      "shift"),
         ("w7_row_masked",   8,  4,  3,  49,  32, 0.5,      1.0,      "row"),
         ("w7_neg_inf",      8,  4,  3,  49,  32, 0.5,      1.0,      "inf"),
         ("w12_shift",       4,  4,  2,  144, 32, 1.0,      2.0,      "shift"),
         ("w12_peaked_inf",  4,  4,  2,  144, 32, 4.0,      6.0,      "inf")]
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module", autouse=True)
def _write_margins():
    yield
    merge_margins(os.environ.get("P4V_FUSED_WATTN_OUT"), "emulation", _MARGINS, IDS)


def _inputs(case):
    name, B_, nW, H, N, D, bstd, qf, kind = case
    rng = np.random.default_rng(2600 + IDS.index(name))
    q = (rng.standard_normal((B_, H, N, D)) * qf * D ** -0.5).astype(F32)        # scaled, as the module hands it to matmul1
    kT = rng.standard_normal((B_, H, D, N)).astype(F32)
    bias = (rng.standard_normal((H, N, N)) * bstd).astype(F32)
    mask = None
    if kind is not None:
        mask = fw.shift_mask(nW, N, rng, -np.inf if kind == "inf" else -100.0)
        if kind == "row":
            mask[1, 5, :] = -100.0                                               # every key of one row: ordinary probabilities
    f = np.array([1.0, 0.8, 1.25][:H], F32).reshape(1, H, 1, 1)
    A_iv = (np.abs(q).max(axis=(0, 2, 3), keepdims=True) / F32(127.5) * f).astype(F32)
    B_iv = (np.abs(kT).max(axis=(0, 2, 3), keepdims=True) / F32(127.5) * f[:, ::-1]).astype(F32)
    return q, kT, bias, mask, A_iv, B_iv


def _pairwise(e):
    """fp32 sum over the last axis, adjacent pairs level by level"""
    while e.shape[-1] > 1:
        if e.shape[-1] % 2:
            e = np.concatenate([e, np.zeros(e.shape[:-1] + (1,), F32)], -1)
        e = (e[..., 0::2] + e[..., 1::2]).astype(F32)
    return e


def emulate(q, kT, bias, mask, A_iv, B_iv, bits=8):
    """The kernel's chain in fp32 on the CPU"""
    Q = 2 ** (bits - 1)
    qi, _ = fr.int_plane(q, A_iv, -Q, Q - 1)
    ki, _ = fr.int_plane(kT, B_iv, -Q, Q - 1)
    acc = fr._imatmul(qi, ki)
    assert np.abs(acc).max() < 2 ** 24                                           # float(acc) is exact
    S1 = (A_iv * B_iv).astype(F32)
    u = (acc.astype(F32) * S1).astype(F32)
    u = (u + bias[None]).astype(F32)
    if mask is not None:
        u = (u + mask[np.arange(q.shape[0]) % mask.shape[0]][:, None]).astype(F32)
    with np.errstate(invalid="ignore"):
        e = np.exp((u - u.max(-1, keepdims=True)).astype(F32)).astype(F32)
        return (e / _pairwise(e)).astype(F32)


_STAGES = {}


def _stage(case):
    if case[0] not in _STAGES:
        q, kT, bias, mask, A_iv, B_iv = _inputs(case)
        _STAGES[case[0]] = (fw.window_float_stage(q, kT, A_iv, B_iv, 8, 8, bias, mask), emulate(q, kT, bias, mask, A_iv, B_iv), mask)
    return _STAGES[case[0]]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_emulation_meets_the_bar(case):
    st, probs, mask = _stage(case)
    worst, below = fw.check_window_probs(probs, st, case[0])
    masked_share = float(np.broadcast_to(st["masked"] & (~st["masked"]).any(-1, keepdims=True), probs.shape).mean())
    print(f"[window reference] {case[0]}: emulation / bound {worst:.3f}; below 2^-100: {below:.4f} (masked: {masked_share:.4f})")
    _MARGINS.setdefault("emulation_over_bound", {})[case[0]] = worst
    _MARGINS.setdefault("share_below_floor", {})[case[0]] = below
    assert 0.0 < worst <= 0.6, "the emulation sits well inside the bar, and the bar is not vacuous"
    assert below == masked_share, "exactly the masked entries fall below 2^-100"
    if case[8] == "row":
        row = probs[1::4, :, 5]                                                  # window 1 of every image
        assert (row > 2.0 ** -20).all() and np.allclose(row.sum(-1), 1.0, atol=1e-5), "a fully masked row has ordinary probabilities"


def test_masks_are_what_the_cases_say():
    for case in CASES:
        st, probs, mask = _stage(case)
        if mask is None:
            assert not st["masked"].any()
            continue
        assert not mask[0].any() and all(m.any() for m in mask[1:]), "window 0 unmasked, every other window masked somewhere"
        assert len({m.tobytes() for m in mask}) == len(mask), "a different mask per window"
        assert (np.isinf(mask).any()) == (case[8] == "inf")


def test_bar_refuses_what_it_must():
    case = CASES[IDS.index("w7_quiet")]
    st, probs, mask = _stage(case)
    U = fw.row_bound_ulps(st)
    # a masked key at -100 does not loosen its row: the bar of every row comes from |u| of its contributing keys (a few units here)
    assert np.abs(st["u64"]).max() > 90.0 and U.max() < 10.0 + 49 / 64.0 + 6.0 * 8.0, float(U.max())
    big = st["p64"] >= fr.P_FLOOR
    z, h, m, n = (int(i) for i in np.argwhere(big & (st["p64"] > 1e-3))[0])
    bad = probs.copy()
    bad[z, h, m, n] = F32(st["p64"][z, h, m, n] * (1.0 + 1.5 * U[z, h, m, 0] * 2.0 ** -23))
    with pytest.raises(AssertionError, match="of the bound"):
        fw.check_window_probs(bad, st, "off by 1.5 U_row ulps")
    # an unmasked entry below 2^-100 is refused even where it is tiny, and so is a masked entry that is not tiny
    bad = probs.copy()
    z, h, m, n = (int(i) for i in np.argwhere(~big)[0])
    bad[z, h, m, n] = F32(2.0 ** -90)
    with pytest.raises(AssertionError, match="below 2\\^-100 came out"):
        fw.check_window_probs(bad, st, "a masked key at 2^-90")
    st2 = dict(st, masked=np.zeros_like(st["masked"]))
    with pytest.raises(AssertionError, match="no masked entries"):
        fw.check_window_probs(probs, st2, "tiny entries without a mask")
    # wrong window index: the mask of window w + 1 on window w
    q, kT, bias, mask, A_iv, B_iv = _inputs(case)
    wrong = emulate(q, kT, bias, np.roll(mask, 1, axis=0), A_iv, B_iv)
    with pytest.raises(AssertionError):
        fw.check_window_probs(wrong, st, "mask of the wrong window")


def test_all_neg_inf_row_is_nan_in_both():
    case = CASES[IDS.index("w7_neg_inf")]
    q, kT, bias, mask, A_iv, B_iv = _inputs(case)
    mask = mask.copy()
    mask[2, 7, :] = -np.inf
    st = fw.window_float_stage(q, kT, A_iv, B_iv, 8, 8, bias, mask)
    probs = emulate(q, kT, bias, mask, A_iv, B_iv)
    assert np.isnan(st["p64"][2::4, :, 7]).all() and np.isnan(probs[2::4, :, 7]).all()
    assert np.isnan(st["p64"]).sum() == 2 * 3 * 49
    worst, _ = fw.check_window_probs(probs, st, "one row of -inf")
    assert worst <= 1.0
