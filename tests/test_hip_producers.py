"""GPU, bit-exact: the producer kernels of the search that only move and quantise bytes.

* k_pack_twin (the merged post-GELU twin plane, p4v_pack_plane_i8 mode "twin") and k_pack_dual (both fixed planes of a
  twin row operand from one read, p4v_debug_pack_dual) against numpy's IEEE division, on and around every breakpoint of
  the 8-bit and 6-bit grids, plus zeros, saturation, NaN / +-inf and a scale whose reciprocal overflows;
* k_prep_epi6 (k_sweep6's epilogue operands in fragment order, p4v_debug_prep_epi6) against a numpy restatement of the
  chunk order documented in csrc/p4v_kernels.h, in both orientations, for every wt_mode, ragged sizes included.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    return engine


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _grid(v, lo, hi):
    """fminf(fmaxf(rintf(v), lo), hi) with C's NaN rules (fmaxf / fminf return the other operand)."""
    return np.fmin(np.fmax(np.rint(v), np.float32(lo)), np.float32(hi))


def _around(points):
    """Every point and its two float32 neighbours."""
    p = np.asarray(points, np.float32)
    return np.concatenate([p, np.nextafter(p, np.float32(np.inf)), np.nextafter(p, np.float32(-np.inf))])


SPECIALS = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 3.0e38, -3.0e38, 1e-30, -1e-30], np.float32)


def _rows(values, cols, rng):
    """values laid out row-major over `cols` columns (the tail filled with random ones), shuffled so that every special
    value also lands in the last, partial 16-element run of a row."""
    n = -(-len(values) // cols) * cols
    x = np.concatenate([values, rng.standard_normal(n - len(values)).astype(np.float32)])
    rng.shuffle(x)
    return x.reshape(-1, cols)


def _twin_ref(x, s, sn, lo, hi):
    with np.errstate(all="ignore"):
        pos = _grid(x / np.float32(s), 0, hi)
        neg = _grid(x / np.float32(sn), lo, 0)
    return pos, neg


def _i8(v):
    return (v.astype(np.int64) & 0xFF).astype(np.uint8).view(np.int8)


CASES = [(8, 0.0123), (6, 0.0567), (8, 2.0e-39)]     # (bits, positive-range scale); 2e-39: 1/s overflows


@pytest.mark.parametrize("bit,s", CASES)
@pytest.mark.parametrize("cols", [256, 199])          # aligned rows (dwordx4 loads) and ragged ones (per element)
def test_twin_plane_matches_ieee_division(eng, bit, s, cols):
    q = 2 ** (bit - 1)
    lo, hi = -q, q - 1
    sn = np.float32(0.2785 / q)
    k = np.arange(-q - 2, q + 2, dtype=np.float32)
    x = np.concatenate([_around((k + 0.5) * np.float32(s)), _around((k + 0.5) * sn), _around(k * np.float32(s)), SPECIALS])
    x = _rows(x, cols, np.random.default_rng(bit * 7 + cols))
    pos, neg = _twin_ref(x, s, sn, lo, hi)
    got, padded = eng.pack_plane_i8(_t(x), mode="twin", scales=torch.tensor([s], dtype=torch.float32), const_scale=float(sn),
                                    lo=lo, hi=hi, qmax=q)
    np.testing.assert_array_equal(got.cpu().numpy(), _i8(pos + neg))
    assert not padded[:, cols:].any()


@pytest.mark.parametrize("bit,s", CASES)
@pytest.mark.parametrize("cols", [256, 199])
def test_dual_postgelu_planes_match_ieee_division(eng, bit, s, cols):
    q = 2 ** (bit - 1)
    lo, hi = -q, q - 1
    sn = np.float32(0.2785 / q)
    k = np.arange(-q - 2, q + 2, dtype=np.float32)
    x = np.concatenate([_around((k + 0.5) * np.float32(s)), _around((k + 0.5) * sn), SPECIALS])
    x = _rows(x, cols, np.random.default_rng(bit * 11 + cols))
    pos, neg = _twin_ref(x, s, sn, lo, hi)
    p1, p2, q1, q2 = eng.debug_pack_dual(_t(x), sos=False, scale=s, lo=lo, hi=hi, qmax=q, const_scale=float(sn))
    np.testing.assert_array_equal(p1.cpu().numpy(), _i8(pos))
    np.testing.assert_array_equal(p2.cpu().numpy(), _i8(neg))
    assert not q1[:, cols:].any() and not q2[:, cols:].any()


@pytest.mark.parametrize("bit,split", [(8, 0.0371), (6, 0.125), (8, 1.0e-38)])
@pytest.mark.parametrize("cols", [256, 199])
def test_dual_split_of_softmax_planes_match_ieee_division(eng, bit, split, cols):
    """PACK_SOS_HI = clamp(rint(clamp(x, split, 1) * (q-1)), 0, q-1), PACK_SOS_LO = clamp(rint(clamp(x, 0, split) / a), 0, q-1)
    with a = split / (q-1) (matmul.py:595-598)."""
    q = 2 ** (bit - 1)
    qm1 = np.float32(q - 1)
    split = np.float32(split)
    a = np.float32(split / qm1)
    k = np.arange(-1, q + 1, dtype=np.float32)
    x = np.concatenate([_around((k + 0.5) * a), _around((k + 0.5) / qm1), _around([split, 1.0]), SPECIALS])
    x = _rows(x, cols, np.random.default_rng(bit * 13 + cols))
    x[::2] = np.abs(x[::2]) * np.float32(0.05)           # softmax-like rows: mostly small and positive
    with np.errstate(all="ignore"):
        ref_hi = _grid(np.fmin(np.fmax(x, split), np.float32(1.0)) * qm1, 0, qm1)
        ref_lo = _grid(np.fmin(np.fmax(x, np.float32(0.0)), split) / a, 0, qm1)
    p1, p2, q1, q2 = eng.debug_pack_dual(_t(x), sos=True, scale=float(split), lo=0, hi=q - 1, qmax=q)
    np.testing.assert_array_equal(p1.cpu().numpy(), _i8(ref_hi))
    np.testing.assert_array_equal(p2.cpu().numpy(), _i8(ref_lo))
    assert not q1[:, cols:].any() and not q2[:, cols:].any()


# ---- k_prep_epi6 ----------------------------------------------------------------------------------------------------------
def _epi6_ref(O, Wt, bias, o_ss, o_ts, SR, TR, bias_on_t, wt_mode, transposed):
    """Chunk ((((t * 8 + b) * 2 + cb) * 4 + q) * 2 + k) * 64 + lane of 16 bytes, t = tt * stiles + st, lane = 32 g + l31:
    plain, stationary rows st*256 + b*32 + 8q + 4g + e at streaming row tt*64 + cb*32 + l31; transposed, streaming rows
    tt*64 + cb*32 + 8q + 4g + e at stationary row st*256 + b*32 + l31.  k = 0: raw_out - bias (raw_out itself for wt_mode 4),
    k = 1: the metric weight (1, raw_grad, raw_out, |raw_out|, the bias for wt_mode 0..4); zero where either row is padding."""
    stiles, ttiles = -(-SR // 256), -(-TR // 64)
    tt, st, b, cb, q, g, l31, e = np.meshgrid(np.arange(ttiles), np.arange(stiles), np.arange(8), np.arange(2), np.arange(4),
                                              np.arange(2), np.arange(32), np.arange(4), indexing="ij")
    within = 8 * q + 4 * g + e
    if transposed:
        sr, tr = st * 256 + b * 32 + l31, tt * 64 + cb * 32 + within
    else:
        sr, tr = st * 256 + b * 32 + within, tt * 64 + cb * 32 + l31
    valid = (sr < SR) & (tr < TR)
    idx = np.where(valid, sr * o_ss + tr * o_ts, 0)
    o = O[idx]
    bs = bias[np.where(valid, tr if bias_on_t else sr, 0)]
    one = np.ones_like(o)
    v0 = o if wt_mode == 4 else o - bs
    v1 = {0: one, 1: Wt[idx] if Wt is not None else one, 2: o, 3: np.abs(o), 4: bs}[wt_mode]
    out = np.stack([np.where(valid, v0, 0), np.where(valid, v1, 0)], axis=5).astype(np.float32)
    # axes: tt, st, b, cb, q, k, g, l31, e -> chunk order with t = tt * stiles + st
    return out.reshape(-1)


# (SR, TR, ld, orientation) -- "a": the activation search (features contiguous, bias by stationary row), "cos_t": the
# transposed cosine weight search (features contiguous, bias by streaming row; wt_mode 4 only), "w": the plain weight search
# (strided stationary rows: the element-by-element path).  An aligned row stride with a column count that is not a multiple of
# 4 (302 / 304, 98 / 100) takes the dwordx4 path with a last, partial chunk per row loaded element by element.
EPI6 = [(sr, tr, ld, o, m) for (sr, tr, ld, o) in [(512, 128, 512, "a"), (300, 70, 300, "a"), (302, 70, 304, "a"), (299, 65, 301, "a"),
                                                   (300, 70, 70, "w")]
        for m in range(5)] + [(256, 192, 192, "cos_t", 4), (260, 98, 100, "cos_t", 4), (260, 97, 97, "cos_t", 4)]


@pytest.mark.parametrize("SR,TR,ld,orient,wt_mode", EPI6)
def test_prep_epi6_chunk_order(eng, SR, TR, ld, orient, wt_mode):
    rng = np.random.default_rng(SR * 1000 + TR * 10 + wt_mode)
    transposed = orient == "cos_t"
    if orient == "a":       # raw_out [TR][ld]: s -> column
        o_ss, o_ts, n, bias_on_t = 1, ld, TR * ld, 0
    else:                   # raw_out [SR][ld]: t -> column
        o_ss, o_ts, n, bias_on_t = ld, 1, SR * ld, 1
    O = rng.standard_normal(n).astype(np.float32)
    Wt = rng.standard_normal(n).astype(np.float32) if wt_mode == 1 else None
    bias = rng.standard_normal(max(SR, TR)).astype(np.float32)
    ref = _epi6_ref(O, Wt, bias, o_ss, o_ts, SR, TR, bias_on_t, wt_mode, transposed)
    got = eng.debug_prep_epi6(_t(O), _t(Wt) if Wt is not None else None, _t(bias), o_ss=o_ss, o_ts=o_ts, sr=SR, tr=TR,
                              bias_on_t=bias_on_t, wt_mode=wt_mode, transposed=transposed).cpu().numpy()
    assert got.shape == ref.shape
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))
