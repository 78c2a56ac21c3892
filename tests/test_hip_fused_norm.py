"""GPU: the fused LayerNorm producer (k_ln_pack; engine.linear_quant_forward / mlp_quant_forward with ln=).

Per case, with want_norm and want_planes, on a poisoned workspace of exactly the size asked for:
1. y against the float64 LayerNorm of the same inputs.  The bar is per case: twice the largest error of torch's own fp32
   F.layer_norm against that float64 result (two fp32 evaluations differ by the order of the two row sums only), plus
   4 * 2^-24 * max(|gamma * yhat64| + |beta|).  With P4V_FUSED_NORM_OUT set the ratios go there (profiles/r35_fused_norm_margins.json).
2. the plane against the oracle's quant_int of the call's own y: every byte, the zero padding of rows and columns included.
3. out against engine.linear_quant_forward / mlp_quant_forward on the call's own y: bit for bit.
4. the window map: y and the plane rows are the identity-map call's, permuted as window_partition(torch.roll(.)) permutes row indices.
Then the workspace contract, the refusals, the launch records and the stream contract of the two fused calls.
"""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.ptq4vit_oracle import quant_int
from ptq4vit_amd.utils.models import window_partition
from tests.fused_common import merge_margins
from tests.workspace_guard import Guard

pytestmark = pytest.mark.gpu

_MARGINS = {}
Case = namedtuple("Case", "name C rows a_bit eps edge", defaults=(8, 1e-6, None))
#               id           C     rows
CASES = [Case("c96_r5",      96,   5),                      # two rows per wave, odd row count, partial lanes
         Case("c128_r130",   128,  130),                    # crosses a 128-row tile
         Case("c192_r33",    192,  33),
         Case("c384_r7",     384,  7),                      # NV = 2, half used
         Case("c768_r3",     768,  3),
         Case("c1024_r2",    1024, 2),
         Case("c2048_r2",    2048, 2),
         Case("c96_a6",      96,   5, 6, 1e-5),             # a narrower grid: quant16_any / pack_value off the sat8 path
         Case("c768_a6",     768,  3, 6, 1e-5),
         Case("c96_const",   96,   5, 8, 1e-6, "const"),    # a row of 0.5: variance 0, exact sums -> y == beta
         Case("c192_mean",   192,  33, 8, 1e-5, "mean"),    # mean 1e4, unit spread: the two-pass variance
         Case("c1024_clamp", 1024, 2, 8, 1e-6, "clamp")]    # x12: both clamp ends reached
IDS = [c.name for c in CASES]
WINDOWS = [(2, 8, 8, 4, 0), (2, 8, 8, 4, 2), (2, 6, 12, 3, 1), (2, 4, 4, 4, 0)]        # B, H, W, ws, shift


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    yield engine
    engine.release_workspace()
    merge_margins(os.environ.get("P4V_FUSED_NORM_OUT"), "engine", _MARGINS, IDS + ["mlp_c48", "mlp_c192"])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _inputs(C, shape, seed, a_bit=8, eps=1e-6, edge=None, N=64):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, C, generator=g)
    if edge == "const":
        x[..., 1, :] = 0.5
    elif edge == "mean":
        x += 1e4
    gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    if edge == "clamp":
        gamma = gamma * 12.0
    W = torch.randn(N, C, generator=g) * C ** -0.5
    q = 2 ** (a_bit - 1)
    layer = dict(weight=W.cuda(), bias=(0.1 * torch.randn(N, generator=g)).cuda(), w_interval=(W.abs().amax() / 127.5).reshape(1).cuda(),
                 a_interval=torch.tensor([3.0 / (q - 0.5)]).cuda(), w_bit=8, a_bit=a_bit, n_V=1, n_H=1, n_a=1)
    return x.cuda(), dict(weight=gamma.cuda(), bias=beta.cuda(), eps=eps), layer


def _guarded(eng, monkeypatch, call):
    with torch.no_grad(), Guard(eng, monkeypatch, 0xCD) as g:
        res = call()
        reps = g.finish()
    assert len(reps) == 1 and reps[0]["guard_changed"] == 0 and 0 < reps[0]["touched"] <= reps[0]["need"], reps
    return res


def _check_y(y, x, ln, name):
    """check 1; returns |y - y64| over the bar"""
    x64, g64, b64 = x.double(), ln["weight"].double(), ln["bias"].double()
    yhat = (x64 - x64.mean(-1, keepdim=True)) / torch.sqrt(x64.var(-1, unbiased=False, keepdim=True) + ln["eps"])
    y64 = yhat * g64 + b64
    torch_err = (F.layer_norm(x, (x.shape[-1],), ln["weight"], ln["bias"], ln["eps"]).double() - y64).abs().max().item()
    bar = 2.0 * torch_err + 4 * 2.0 ** -24 * ((yhat * g64).abs() + b64.abs()).max().item()
    err = (y.double() - y64).abs().max().item()
    print(f"[fused norm] {name}: |y - y64| {err:.3e}, torch's {torch_err:.3e}, bar {bar:.3e}, ratio {err / bar:.3f}")
    _MARGINS.setdefault("y_over_bar", {})[name] = err / bar
    assert err <= bar, (name, err, bar)


def _check_plane(plane, y, layer, name):
    """check 2: every byte, the padding included"""
    M, C = y.numel() // y.shape[-1], y.shape[-1]
    q = 2 ** (layer["a_bit"] - 1)
    assert plane.shape[0] % 128 == 0 and plane.shape[0] >= M and plane.shape[1] == (C + 63) // 64 * 64
    ref = np.zeros(tuple(plane.shape), np.int32)
    ref[:M, :C] = quant_int(y.reshape(M, C).cpu().numpy(), layer["a_interval"].cpu().numpy(), -q, q - 1)
    bad = int((plane.cpu().numpy().astype(np.int32) != ref).sum())
    assert bad == 0, f"{name}: {bad} of {ref.size} plane bytes differ from quant_int(y)"
    return ref


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ln_linear(eng, monkeypatch, case):
    x, ln, layer = _inputs(case.C, (1, case.rows), 3500 + IDS.index(case.name), case.a_bit, case.eps, case.edge)
    out, y, plane = _guarded(eng, monkeypatch, lambda: eng.linear_quant_forward(x=x, ln=ln, **layer, want_norm=True, want_planes=True))
    _check_y(y, x, ln, case.name)
    ref = _check_plane(plane, y, layer, case.name)
    with torch.no_grad():
        assert torch.equal(_bits(out), _bits(eng.linear_quant_forward(x=y, **layer)))
    if case.edge == "const":
        assert torch.equal(y[0, 1], ln["bias"]), "variance 0 and exact sums: y is beta"
    if case.edge == "clamp":
        assert ref.min() == -128 and ref.max() == 127


@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: "b%d_%dx%d_ws%d_s%d" % w)
def test_window_map_is_roll_and_partition_of_the_rows(eng, monkeypatch, win):
    B, H, W, ws, shift = win
    x, ln, layer = _inputs(96, (B, H * W), 3580)
    with torch.no_grad():
        out0, y0, plane0 = eng.linear_quant_forward(x=x, ln=ln, **layer, want_norm=True, want_planes=True)
    out, y, plane = _guarded(eng, monkeypatch, lambda: eng.linear_quant_forward(x=x, ln=ln, **layer, window=(H, W, ws, shift),
                                                                                  want_norm=True, want_planes=True))
    idx = torch.arange(B * H * W).view(B, H, W, 1)
    perm = window_partition(torch.roll(idx, shifts=(-shift, -shift), dims=(1, 2)), ws).reshape(-1).cuda()
    M = B * H * W
    assert torch.equal(_bits(y).view(M, -1), _bits(y0).view(M, -1)[perm]) and torch.equal(plane[:M], plane0[:M][perm])
    assert not plane[M:].any() and torch.equal(_bits(out).view(M, -1), _bits(out0).view(M, -1)[perm])
    _check_plane(plane, y, layer, "window")


@pytest.mark.parametrize("name,C,hidden,shape,twin", [("mlp_c48", 48, 72, (1, 5), True), ("mlp_c192", 192, 768, (2, 197), False)])
def test_ln_mlp(eng, monkeypatch, name, C, hidden, shape, twin):
    x, ln, fc1 = _inputs(C, shape, 3590 + C, N=hidden)
    g = torch.Generator().manual_seed(3600 + C)
    W2 = (torch.randn(C, hidden, generator=g) * hidden ** -0.5).cuda()
    fc2 = dict(weight=W2, bias=None, w_interval=(W2.abs().amax() / 127.5).reshape(1), a_interval=torch.tensor([2.0 / 127.5]).cuda(),
               w_bit=8, a_bit=8, n_V=1, n_H=1, n_a=1, postgelu=twin)
    out, y, hid, plane = _guarded(eng, monkeypatch, lambda: eng.mlp_quant_forward(x=x, ln=ln, fc1=fc1, fc2=fc2, want_norm=True,
                                                                                    want_hidden=True, want_planes=True))
    _check_y(y, x, ln, name)
    _check_plane(plane, y, fc1, name)
    with torch.no_grad():
        out_r, hid_r = eng.mlp_quant_forward(x=y, fc1=fc1, fc2=fc2, want_hidden=True)
    assert torch.equal(_bits(hid), _bits(hid_r)) and torch.equal(_bits(out), _bits(out_r))


def test_workspace_refusals_and_records(eng, monkeypatch):
    x, ln, layer = _inputs(96, (2, 64), 3599)
    kw = dict(x=x, ln=ln, **layer)
    with torch.no_grad():
        torch.cuda.synchronize()
        before = eng.launch_counters()
        # one byte less: refused, nothing launched
        with Guard(eng, monkeypatch, 0xCD, declare=lambda n: n - 1) as g:
            with pytest.raises(RuntimeError, match="workspace too small"):
                eng.linear_quant_forward(**kw)
            reps = g.finish()
        assert all(r["touched"] == 0 and r["guard_changed"] == 0 for r in reps), reps
        # outside the envelope: refused before any launch
        for C in (2052, 98):
            xb, lnb, layerb = _inputs(C, (1, 2), 3598)
            with pytest.raises(NotImplementedError, match="multiple of 4 up to 2048"):
                eng.linear_quant_forward(x=xb, ln=lnb, **layerb)
        for window in ((8, 8, 4, 4), (8, 16, 3, 0)):                # shift = ws; H % ws != 0
            with pytest.raises((NotImplementedError, RuntimeError), match="window map"):
                eng.linear_quant_forward(**kw, window=window)
        assert eng.launch_counters() == before
        # the launch records: one launch of the new kind, as many launches as the unfused Linear (k_pack1 of the rows is gone)
        eng.stats_enable(True)
        try:
            eng.stats_reset()
            c0 = eng.launch_counters()["asked"]
            _, y, plane = eng.linear_quant_forward(**kw, want_norm=True, want_planes=True)
            c1 = eng.launch_counters()["asked"]
            torch.cuda.synchronize()
            recs = eng.stats_launches()
            eng.linear_quant_forward(x=y, **layer)
            c2 = eng.launch_counters()["asked"]
        finally:
            eng.stats_enable(False)
    kernels = [r["kernel"] for r in recs]
    assert kernels.count("k_ln_pack") == 1 and len(kernels) == 2 and c1 - c0 == c2 - c1, (kernels, c0, c1, c2)
    rec = recs[kernels.index("k_ln_pack")]
    assert rec["alg_bytes"] == 2 * 4 * 128 * 96 + 8 * 96 + plane.numel() and rec["alg_ops"] == 0      # x, y_out, gamma + beta, the plane


def test_the_fused_calls_run_on_the_callers_stream_and_never_synchronise(eng):
    """the stream contract (tests/test_hip_streams.py) for the ln= paths: behind a busy named stream the calls return at once, read
    what that stream wrote before them, and give the default stream's bits"""
    x, ln, fc1 = _inputs(96, (2, 64), 3597, N=192)
    fc2 = dict(fc1, weight=fc1["weight"].t().contiguous(), bias=None)
    calls = (lambda t: eng.linear_quant_forward(x=t, ln=ln, window=(8, 8, 4, 2), **fc1), lambda t: eng.mlp_quant_forward(x=t, ln=ln, fc1=fc1, fc2=fc2))
    with torch.no_grad():
        refs = [c(x) for c in calls]                            # (first calls of the process: the conversion probe runs here)
        from tests.stream_cases import Delay
        delay, side, done = Delay(x.device), torch.cuda.Stream(), torch.cuda.Event()
        late = torch.full_like(x, float("nan"))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            [c(late) for c in calls]                            # (the side stream's workspace and output blocks exist before the timing)
        torch.cuda.synchronize()
        delay(side, 50.0)
        with torch.cuda.stream(side):
            late.copy_(x)                                       # the input arrives on the side stream, behind the delay
            got = [c(late) for c in calls]
            done.record()
            returned_while_busy = not done.query()
        side.synchronize()
    assert returned_while_busy, "a fused call waited for its stream"
    assert all(torch.equal(_bits(g), _bits(r)) for g, r in zip(got, refs))
