"""CPU references for each stage of the two fused int8 forwards (tests/test_hip_fused_attention.py, tests/test_hip_fused_mlp.py,
tests/test_fused_reference_cpu.py).  numpy / torch float64 and int64 only; the quantisers are the oracle's (quant_int,
twin_planes, sos_planes of oracle/ptq4vit_oracle.py).  Nothing of the library under test is imported here.

Stage 1, the float stage, from the RAW fp32 inputs and the intervals:

  attention   dot = Q(q) . Q(k^T), exact in int64;  u64 = dot * f64(A_iv) * f64(B_iv) * f64(float32(scale));
              p64 = softmax(u64) in float64.  The call's probs must satisfy
                  |probs - p64| <= p64 * U_row * 2^-23   wherever p64 >= 2^-100,      0 <= probs <= 2^-99   elsewhere,
              U_row = 10 + N / 64 + 5 * max_n |u64|:  the project's 8 ulp cover exp, the division and the final rounding; the
              N / 32-long addition chain of the pairwise row sum adds N / 64 + 2 (half an ulp per addition, plus the four levels
              of the pairwise tree and the exchange between the lane halves); S1 = A_iv * B_iv, acc * S1, `* scale` and u - max
              are four fp32 roundings of the EXPONENT, 2^-24 |u| each at most -- 4 * 2^-24 |u|max in the numerator, as much
              in the denominator's dominant terms, of which the part common to both cancels: at most 5 * 2^-24 |u|max * 2 =
              5 |u|max ulps of 2^-23.
  MLP         o64 = dot * f64(a_iv) * f64(w_iv[block]);  v64 = o64 + bias;  g64 = v64 * 0.5 * (1 + erf(v64 / sqrt 2)).
              The call's hidden must satisfy |hidden - g64| <= E_g = 2^-24 (3 |o64| + 12 |v64|) + 2^-126:  the scale product
              and acc * S1 give 2^-24 |o| each, the bias addition 2^-24 |v|, all three times GELU's slope (at most 1.13):
              (2 |o| + |v|) * 1.13; erff is held to OpenCL's 16 ulp of a value of at most 1, times |v| / 2: 8 * 2^-23 |v| / 2
              = 8 * 2^-24 |v|; `1 +`, `* 0.5` (exact) and the last multiply: 2 * 2^-24 |v|.  Rounded up: 3 |o| + 12 |v|.

Stage 2, the quantiser: the call's planes are, byte for byte, sos_planes / twin_planes / quant_int of the call's OWN fp32
  probs / hidden; NaN entries are excluded (their byte only has to lie on the grid); padding rows and columns are zero.  Exact.

Stage 3, the consumer: `out` against the int64 GEMM of the call's own planes with quant_int(v) / quant_int(W2), scaled in
  float64 (each of the twin's planes on its own scale; fc2's bias added); the bar is the project's int8-forward bar, 2e-6 sqrt(K)
  of the largest output.

A zero interval (a block of zeros under the min-max rule) is the reference's 0 / 0: every entry of the block's integer plane is
undefined, every product with it NaN -- `float_plane` keeps that NaN, and the float stage hands it on."""
import numpy as np
import torch

from oracle.ptq4vit_oracle import qmax_of, quant_int, sos_planes, twin_planes

F32, F64 = np.float32, np.float64
P_FLOOR = 2.0 ** -100
FORWARD_BAR = 2e-6


def as_np(t, dtype=F32):
    if torch.is_tensor(t):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t, dtype=dtype))


def int_plane(x, s, lo, hi):
    """(quant_int(x, s, lo, hi) as int64 with 0 where the quotient is NaN, the NaN mask)"""
    x, s = as_np(x), np.asarray(s, dtype=F32)
    with np.errstate(all="ignore"):
        nan = np.isnan(x / s)                       # 0 / 0: the entry has no grid index
        k = quant_int(x, s, lo, hi)
    return np.where(nan, 0, k).astype(np.int64), nan


def _imatmul(a, b):
    return (torch.from_numpy(np.ascontiguousarray(a)) @ torch.from_numpy(np.ascontiguousarray(b))).numpy()


# ---- attention -------------------------------------------------------------------------------------------------------------------
def attn_float_stage(q, kT, A_iv, B_iv, A_bit, B_bit, scale):
    """(u64, p64) [B][H][M][N] of q [B][H][M][D], kT [B][H][D][N] and matmul1's head-wise intervals [H]."""
    q, kT = as_np(q), as_np(kT)
    H = q.shape[1]
    a, b = as_np(A_iv).reshape(1, H, 1, 1), as_np(B_iv).reshape(1, H, 1, 1)
    Aq, Bq = qmax_of(A_bit), qmax_of(B_bit)
    qi, qn = int_plane(q, a, -Aq, Aq - 1)
    ki, kn = int_plane(kT, b, -Bq, Bq - 1)
    dot = _imatmul(qi, ki)
    u64 = dot.astype(F64) * a.astype(F64) * b.astype(F64) * F64(F32(scale))
    u64[qn.any(-1)[..., :, None] | kn.any(-2)[..., None, :]] = np.nan
    with np.errstate(invalid="ignore"):
        e = np.exp(u64 - u64.max(-1, keepdims=True))
        p64 = e / e.sum(-1, keepdims=True)
    return u64, p64


def check_probs(probs, u64, p64, what):
    """Stage 1 of the attention chain; returns the worst ratio of |probs - p64| to its bound."""
    probs = as_np(probs)
    assert probs.shape == p64.shape, f"{what}: probs {probs.shape}, reference {p64.shape}"
    live = ~np.isnan(p64)
    assert np.isnan(probs[~live]).all(), f"{what}: finite probabilities where the reference is NaN"
    assert not np.isnan(probs[live]).any(), f"{what}: NaN probabilities where the reference is finite"
    N = p64.shape[-1]
    with np.errstate(invalid="ignore"):
        U = 10.0 + N / 64.0 + 5.0 * np.abs(u64).max(-1, keepdims=True)
        bound = p64 * U * 2.0 ** -23
        big = live & (p64 >= P_FLOOR)
    small = live & ~big
    assert (probs[small] >= 0).all() and (probs[small] <= 2.0 ** -99).all(), \
        f"{what}: a probability below 2^-100 came out as {probs[small].max()!r} / {probs[small].min()!r}"
    if not big.any():
        return 0.0
    ratio = np.abs(probs.astype(F64) - p64)[big] / bound[big]
    worst = float(ratio.max())
    assert worst <= 1.0, f"{what}: |probs - p64| is {worst:.3f} of the bound p64 * U_row * 2^-23 ({int((ratio > 1).sum())} entries above)"
    return worst


def attn_planes_of(probs, H, *, sos, A_bit, split=None, A_iv=None):
    """matmul2's integer row plane(s) [Z][M][N] of the fp32 probabilities [B][H][M][N] and the mask of their NaN entries."""
    p = as_np(probs)
    B, _, M, N = p.shape
    nan = np.isnan(p)
    q = qmax_of(A_bit)
    safe = np.where(nan, F32(0), p)
    if sos:
        planes = sos_planes(safe, F32(as_np(split).reshape(-1)[0]), q)
        grid = [(0, q - 1), (0, q - 1)]
    else:
        with np.errstate(all="ignore"):
            planes = (quant_int(safe, as_np(A_iv).reshape(1, H, 1, 1), -q, q - 1),)
        grid = [(-q, q - 1)]
    return [k.reshape(B * H, M, N) for k in planes], nan.reshape(B * H, M, N), grid


def check_planes(got, want, nan, grid, what):
    """Stage 2: `got` the call's padded int8 planes [Z][Mp][Kp] (or [Mp][Kp]), `want` the integer planes [Z][M][N] (or [M][N]) of
    the call's own fp32 tensor.  Exact outside the NaN entries, on the grid there, zero in the padding.  Returns the bytes compared."""
    assert len(got) == len(want) == len(grid), f"{what}: {len(got)} planes, {len(want)} expected"
    n = 0
    for i, (g, w, (lo, hi)) in enumerate(zip(got, want, grid)):
        g = as_np(g, np.int8).astype(np.int64)
        if g.ndim == 2:
            g, w, m = g[None], w[None], nan[None]
        else:
            m = nan
        Z, M, N = w.shape
        assert g.shape[0] == Z and g.shape[1] >= M and g.shape[2] >= N, f"{what}: plane {g.shape} for {w.shape}"
        body = g[:, :M, :N]
        bad = (body != w) & ~m
        assert not bad.any(), f"{what} plane {i + 1}: {int(bad.sum())} bytes differ from the CPU quantiser's (first at {tuple(np.argwhere(bad)[0])})"
        assert ((body >= lo) & (body <= hi)).all(), f"{what} plane {i + 1}: a byte outside [{lo}, {hi}]"
        assert not g[:, M:].any(), f"{what} plane {i + 1}: padding rows must be zero"
        assert not g[:, :, N:].any(), f"{what} plane {i + 1}: padding columns must be zero"
        n += int((~m).sum())
    return n


def attn_consumer_stage(planes, v, H, *, sos, A_bit, B_bit, B_iv, A_iv, M, N):
    """out64 [B][H][M][Dv] of the call's own padded planes [Z][Mp][Kp] and v [B][H][N][Dv]; A_iv: the split-of-softmax scalar
    A_interval (= split / (q - 1)) or the head-wise [H]."""
    v = as_np(v)
    B, _, _, Dv = v.shape
    Bq = qmax_of(B_bit)
    b = as_np(B_iv).reshape(1, H, 1, 1)
    vi, vn = int_plane(v, b, -Bq, Bq - 1)
    pl = [as_np(p, np.int8).astype(np.int64)[:, :M, :N].reshape(B, H, M, N) for p in planes]
    b64 = b.astype(F64)
    if sos:
        out = _imatmul(pl[0], vi).astype(F64) * (1.0 / (qmax_of(A_bit) - 1)) * b64 + \
            _imatmul(pl[1], vi).astype(F64) * F64(as_np(A_iv).reshape(-1)[0]) * b64
    else:
        out = _imatmul(pl[0], vi).astype(F64) * as_np(A_iv).reshape(1, H, 1, 1).astype(F64) * b64
    out[np.broadcast_to(vn.any(-2)[..., None, :], out.shape)] = np.nan
    return out


def check_out(out, ref64, K, what, skip=None):
    """Stage 3: the NaN pattern of the reference; elsewhere max |out - ref| <= 2e-6 sqrt(K) max |ref|.  `skip`: a mask of
    entries that are not compared (the planes held an undefined byte there).  Returns the ratio to the bar."""
    out = as_np(out).astype(F64)
    assert out.shape == ref64.shape, f"{what}: out {out.shape}, reference {ref64.shape}"
    keep = np.ones(out.shape, bool) if skip is None else ~np.broadcast_to(skip, out.shape)
    nan = np.isnan(ref64)
    assert (np.isnan(out) == nan)[keep].all(), f"{what}: NaN pattern of out differs from the reference's"
    m = keep & ~nan
    if not m.any():
        return 0.0
    ratio = float(np.abs(out[m] - ref64[m]).max() / (FORWARD_BAR * K ** 0.5 * np.abs(ref64[m]).max()))
    assert ratio <= 1.0, f"{what}: max |out - ref| is {ratio:.3f} of 2e-6 sqrt({K}) max |ref|"
    return ratio


# ---- MLP -------------------------------------------------------------------------------------------------------------------------
def _weight_plane(W, w_iv, w_bit):
    """Q(W) [N][K] with one interval per block of N / n_V rows (n_H = 1)"""
    W = as_np(W)
    w_iv = as_np(w_iv).reshape(-1)
    nV = w_iv.size
    assert W.shape[0] % nV == 0
    s = np.repeat(w_iv, W.shape[0] // nV).reshape(-1, 1)
    q = qmax_of(w_bit)
    wi, wn = int_plane(W, s, -q, q - 1)
    return wi, wn, s


def mlp_float_stage(x, W1, b1, w_iv, a_iv, w_bit, a_bit):
    """(o64, v64, g64) [M][hidden] of x [..][K], fc1's weight [hidden][K], bias or None, w_interval [n_V], a_interval (scalar)."""
    x = as_np(x)
    x = x.reshape(-1, x.shape[-1])
    a = F32(as_np(a_iv).reshape(-1)[0])
    q = qmax_of(a_bit)
    xi, xn = int_plane(x, a, -q, q - 1)
    wi, wn, s = _weight_plane(W1, w_iv, w_bit)
    o64 = _imatmul(xi, wi.T).astype(F64) * F64(a) * s.reshape(1, -1).astype(F64)
    o64[xn.any(-1)[:, None] | wn.any(-1)[None, :]] = np.nan
    v64 = o64 + (0.0 if b1 is None else as_np(b1).astype(F64).reshape(1, -1))
    g64 = v64 * 0.5 * (1.0 + torch.erf(torch.from_numpy(v64 / np.sqrt(2.0))).numpy())
    return o64, v64, g64


def check_hidden(hidden, o64, v64, g64, what):
    """Stage 1 of the MLP chain; returns the worst ratio of |hidden - g64| to E_g."""
    h = as_np(hidden)
    h = h.reshape(-1, h.shape[-1])
    assert h.shape == g64.shape, f"{what}: hidden {h.shape}, reference {g64.shape}"
    live = ~np.isnan(g64)
    assert np.isnan(h[~live]).all(), f"{what}: finite hidden entries where the reference is NaN"
    assert not np.isnan(h[live]).any(), f"{what}: NaN hidden entries where the reference is finite"
    if not live.any():
        return 0.0
    E = 2.0 ** -24 * (3.0 * np.abs(o64[live]) + 12.0 * np.abs(v64[live])) + 2.0 ** -126
    ratio = np.abs(h[live].astype(F64) - g64[live]) / E
    worst = float(ratio.max())
    assert worst <= 1.0, f"{what}: |hidden - g64| is {worst:.3f} of E_g ({int((ratio > 1).sum())} entries above)"
    return worst


def mlp_planes_of(hidden, *, twin, a_bit, a_iv, a_neg=None):
    """fc2's integer row plane(s) [M][hidden] of the fp32 hidden tensor and the mask of its NaN entries."""
    h = as_np(hidden)
    h = h.reshape(-1, h.shape[-1])
    nan = np.isnan(h)
    safe = np.where(nan, F32(0), h)
    q = qmax_of(a_bit)
    a = F32(as_np(a_iv).reshape(-1)[0])
    if twin:
        return list(twin_planes(safe, a, F32(a_neg), q)), nan, [(0, q - 1), (-q, 0)]
    return [quant_int(safe, a, -q, q - 1)], nan, [(-q, q - 1)]


def mlp_consumer_stage(planes, W2, b2, w_iv, w_bit, *, twin, a_iv, a_neg, M, hidden):
    """out64 [M][out_features] of the call's own padded planes [Mp][Kp] and fc2's weight [out][hidden]."""
    wi, wn, s = _weight_plane(W2, w_iv, w_bit)
    pl = [as_np(p, np.int8).astype(np.int64)[:M, :hidden] for p in planes]
    s64 = s.reshape(1, -1).astype(F64)
    out = _imatmul(pl[0], wi.T).astype(F64) * F64(F32(as_np(a_iv).reshape(-1)[0])) * s64
    if twin:
        out = out + _imatmul(pl[1], wi.T).astype(F64) * F64(F32(a_neg)) * s64
    out[np.broadcast_to(wn.any(-1)[None, :], out.shape)] = np.nan
    return out + (0.0 if b2 is None else as_np(b2).astype(F64).reshape(1, -1))
