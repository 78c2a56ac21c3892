"""GPU: the fused block output (k_lin_res; engine.linear_quant_forward / mlp_quant_forward with residual=).

Per case, with `out` inside a NaN-filled buffer:
1. out against the unfused chain on the same GPU -- residual + window_reverse / roll(+shift) of linear_quant_forward(x), or
   residual + mlp_quant_forward(...) -- bit for bit.
2. out against float64: the int64 GEMM of the oracle's quantisers times the fp32 scale table, + bias + residual, within
   4 * 2^-24 * (|acc s1| + |acc2 s2| + |bias| + |residual|) per element (four fp32 roundings, each at most half an ulp of a term no
   larger than that sum).  With P4V_FUSED_RES_OUT set the worst ratios go there (profiles/r36_fused_residual_margins.json).
3. the buffer around out is still NaN and every element of out is finite: the scatter writes each destination and nothing else.
4. the launch records: one k_lin_res, no forward sweep.
Then the refusals: an error before any launch, out untouched.
"""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle.ptq4vit_oracle import qmax_of
from ptq4vit_amd.utils.models import window_reverse
from tests.fused_common import merge_margins
from tests.fused_reference import F32, F64, _imatmul, _weight_plane, as_np, int_plane, mlp_planes_of
from tests.workspace_guard import Guard

pytestmark = pytest.mark.gpu

_MARGINS = {}
Lin = namedtuple("Lin", "name rows K N n_V bias w_bit window", defaults=(1, True, 8, None))     # window: (B, H, W, ws, shift)
LIN = [Lin("id_m130", 130, 72, 100),                                # a row tile with 2 valid rows, K pad, one unfilled column tile
       Lin("id_m257_nv2", 257, 192, 260, 2, False),                 # a third column tile of 4 columns; the scale block changes at 130
       Lin("win_ws3", 162, 96, 96, window=(3, 6, 9, 3, 1)),         # H != W; a tile spans many windows and two images; wrap-around
       Lin("win_ws7", 392, 128, 128, window=(2, 14, 14, 7, 3)),     # ws^2 does not divide 128: Swin's own geometry
       Lin("win_ws4", 160, 64, 64, window=(5, 8, 4, 4, 0)),         # the map without a roll
       Lin("id_w4a8", 200, 64, 64, w_bit=4)]                        # grid bounds other than +-128
Mlp = namedtuple("Mlp", "name C hidden shape twin ln")
MLP = [Mlp("mlp_twin", 96, 384, (2, 197), True, False), Mlp("mlp_twin_ln", 96, 384, (2, 197), True, True),
       Mlp("mlp_plain", 64, 200, (1, 130), False, False)]
IDS = [c.name for c in LIN + MLP]


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    yield engine
    engine.release_workspace()
    merge_margins(os.environ.get("P4V_FUSED_RES_OUT"), "engine", _MARGINS, IDS)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _layer(g, N, K, n_V=1, bias=True, w_bit=8, a_max=3.0, postgelu=False):
    W = torch.randn(N, K, generator=g) * K ** -0.5
    w_iv = W.view(n_V, -1).abs().amax(1) / (qmax_of(w_bit) - 0.5)
    return dict(weight=W.cuda(), bias=(0.1 * torch.randn(N, generator=g)).cuda() if bias else None, w_interval=w_iv.cuda(),
                a_interval=torch.tensor([a_max / 127.5]).cuda(), w_bit=w_bit, a_bit=8, n_V=n_V, n_H=1, n_a=1, postgelu=postgelu)


def _framed(shape):
    """(the NaN-filled buffer, `out`: a 16-byte aligned view of `shape` in its middle)"""
    n, pad = int(np.prod(shape)), 4 * shape[-1]
    buf = torch.full((n + 2 * pad,), float("nan"), device="cuda")
    return buf, buf[pad:pad + n].view(shape)


def _run(eng, call, lead=()):
    """the guarded call on its exact, poisoned workspace, with its launch records"""
    eng.stats_enable(True)
    try:
        eng.stats_reset()
        res = call()
        torch.cuda.synchronize()
        kernels = [r["kernel"] for r in eng.stats_launches()]
    finally:
        eng.stats_enable(False)
    assert kernels.count("k_lin_res") == 1 and not any(k.startswith("k_sweep") for k in kernels), kernels
    assert [k for k in kernels if k != "k_lin_res"] == list(lead), kernels
    return res


def _check64(name, out, layer, planes, scales, residual):
    """check 2, in the planes' row order; `planes`: the integer row plane(s) [M][K], `scales`: their activation scales"""
    wi, _, s = _weight_plane(layer["weight"], layer["w_interval"], layer["w_bit"])
    terms = [_imatmul(np.asarray(p, np.int64), wi.T).astype(F64) * (F32(a) * s.reshape(1, -1)).astype(F64) for p, a in zip(planes, scales)]    # acc * fp32 table
    bias = 0.0 if layer["bias"] is None else as_np(layer["bias"]).astype(F64).reshape(1, -1)
    r64 = as_np(residual).astype(F64).reshape(terms[0].shape)
    ref = sum(terms) + bias + r64
    bar = 4 * 2.0 ** -24 * (sum(np.abs(t) for t in terms) + np.abs(bias) + np.abs(r64))
    ratio = float((np.abs(as_np(out).astype(F64).reshape(ref.shape) - ref) / bar).max())
    print(f"[fused residual] {name}: worst |out - ref64| / bar {ratio:.3f}")
    _MARGINS.setdefault("out_over_bar", {})[name] = ratio
    assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("case", LIN, ids=[c.name for c in LIN])
def test_linear_residual(eng, monkeypatch, case):
    g = torch.Generator().manual_seed(3600 + LIN.index(case))
    layer = _layer(g, case.N, case.K, case.n_V, case.bias, case.w_bit)
    if case.window is None:
        x, rshape, window = torch.randn(1, case.rows, case.K, generator=g).cuda(), (1, case.rows, case.N), None
    else:
        B, H, W, ws, shift = case.window
        x, rshape, window = torch.randn(case.rows // (ws * ws), ws * ws, case.K, generator=g).cuda(), (B, H * W, case.N), (H, W, ws, shift)
    residual = torch.randn(rshape, generator=g).cuda()
    buf, out = _framed(rshape)
    with torch.no_grad(), Guard(eng, monkeypatch, 0xCD) as guard:
        got = _run(eng, lambda: eng.linear_quant_forward(x=x, **layer, residual=residual, window=window, out=out))
        reps = guard.finish()
        y = eng.linear_quant_forward(x=x, **layer)
    assert got is out and all(r["guard_changed"] == 0 and 0 < r["touched"] <= r["need"] for r in reps), reps
    if window is not None:
        y = window_reverse(y.view(-1, ws, ws, case.N), ws, H, W)
        y = torch.roll(y, shifts=(shift, shift), dims=(1, 2)) if shift else y
    assert torch.equal(_bits(out), _bits(residual + y.reshape(rshape))), f"{case.name}: not the unfused chain's bits"
    # the reference in x's row order, the residual gathered by the inverse map
    xi, _ = int_plane(x.reshape(-1, case.K), as_np(layer["a_interval"]), -128, 127)
    idx = torch.arange(case.rows, dtype=torch.float32).view(-1, 1)
    if window is not None:
        idx = torch.roll(window_reverse(idx.view(-1, ws, ws, 1), ws, H, W), shifts=(shift, shift), dims=(1, 2))
    dst = torch.empty(case.rows, dtype=torch.long)
    dst[idx.reshape(-1).long()] = torch.arange(case.rows)              # dst[m]: the token row m goes to
    flat = lambda t: t.reshape(case.rows, case.N).cpu()[dst]
    _check64(case.name, flat(out), layer, [xi], [as_np(layer["a_interval"])[0]], flat(residual))
    assert int(torch.isnan(buf).sum()) == buf.numel() - out.numel() and torch.isfinite(out).all()


@pytest.mark.parametrize("case", MLP, ids=[c.name for c in MLP])
def test_mlp_residual(eng, monkeypatch, case):
    g = torch.Generator().manual_seed(3650 + MLP.index(case))
    fc1 = _layer(g, case.hidden, case.C)
    fc2 = _layer(g, case.C, case.hidden, a_max=2.0, postgelu=case.twin)
    x = torch.randn(*case.shape, case.C, generator=g).cuda()
    ln = dict(weight=(1.0 + 0.3 * torch.randn(case.C, generator=g)).cuda(), bias=(0.2 * torch.randn(case.C, generator=g)).cuda(), eps=1e-6) if case.ln else None
    residual = x if case.ln else torch.randn(x.shape, generator=g).cuda()
    buf, out = _framed(tuple(x.shape))
    lead = (["k_ln_pack"] if case.ln else []) + ["k_mlp_fc1"]
    with torch.no_grad(), Guard(eng, monkeypatch, 0xCD) as guard:
        got, hidden = _run(eng, lambda: eng.mlp_quant_forward(x=x, ln=ln, fc1=fc1, fc2=fc2, residual=residual, out=out, want_hidden=True), lead)
        reps = guard.finish()
        ref, hid_r = eng.mlp_quant_forward(x=x, ln=ln, fc1=fc1, fc2=fc2, want_hidden=True)
    assert got is out and all(r["guard_changed"] == 0 and 0 < r["touched"] <= r["need"] for r in reps), reps
    assert torch.equal(_bits(hidden), _bits(hid_r)) and torch.equal(_bits(out), _bits(residual + ref)), f"{case.name}: not the unfused chain's bits"
    a_neg = F32(0.16997124254703522 / 128)
    planes, _, _ = mlp_planes_of(hidden, twin=case.twin, a_bit=8, a_iv=fc2["a_interval"], a_neg=a_neg)
    _check64(case.name, out, fc2, planes, [as_np(fc2["a_interval"])[0], a_neg], residual)
    assert int(torch.isnan(buf).sum()) == buf.numel() - out.numel() and torch.isfinite(out).all()


#            id             message                  N   rows layer        window         residual / out offsets in the buffer (floats)
REFUSED = [("n_mod4",      "multiple of 4",         98, 128, {},          None,          0, None),
           ("n_a2",        "n_H = n_a = 1",         64, 128, {"n_a": 2},  None,          0, None),
           ("h_mod_ws",    "window map",            64, 128, {},          (8, 16, 3, 0), 0, None),
           ("shift_ge_ws", "window map",            64, 128, {},          (8, 8, 4, 4),  0, None),
           ("rows_mod_hw", "window map",            64, 96,  {},          (8, 8, 4, 0),  0, None),
           ("misaligned",  "aligned to 16 bytes",   64, 128, {},          None,          1, None),
           ("overlap",     "overlaps the residual", 64, 128, {},          None,          0, 4),
           ("ws_short",    "workspace too small",   64, 128, {},          None,          0, None)]


@pytest.mark.parametrize("name,msg,N,rows,over,window,r_off,o_off", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_before_any_launch(eng, monkeypatch, name, msg, N, rows, over, window, r_off, o_off):
    g = torch.Generator().manual_seed(3690)
    layer, x = dict(_layer(g, N, 64), **over), torch.randn(2, rows // 2, 64, generator=g).cuda()
    n, buf = rows * N, torch.randn(rows * N + 8, generator=g).cuda()
    residual = buf[r_off:r_off + n].view(2, rows // 2, N)
    out = torch.full_like(residual, float("nan")) if o_off is None else buf[o_off:o_off + n].view(2, rows // 2, N)
    before_bits = _bits(out).clone()
    with torch.no_grad(), Guard(eng, monkeypatch, 0xCD, declare=(lambda b: b - 1) if name == "ws_short" else None) as guard:
        torch.cuda.synchronize()
        before = eng.launch_counters()
        with pytest.raises((NotImplementedError, RuntimeError), match=msg):
            eng.linear_quant_forward(x=x, **layer, residual=residual, window=window, out=out)
        assert eng.launch_counters() == before and all(r["touched"] == 0 and r["guard_changed"] == 0 for r in guard.finish())
    assert torch.equal(_bits(out), before_bits)


def test_keyword_rules(eng):
    g = torch.Generator().manual_seed(3699)
    layer, x = _layer(g, 64, 64), torch.randn(1, 4, 64, generator=g).cuda()
    ln = dict(weight=torch.ones(64).cuda(), bias=torch.zeros(64).cuda(), eps=1e-6)
    with pytest.raises(ValueError, match="do not go together"):
        eng.linear_quant_forward(x=x, **layer, ln=ln, residual=x)
    with pytest.raises(ValueError, match="window belongs"):
        eng.linear_quant_forward(x=x, **layer, window=(2, 2, 2, 0))
