"""GPU: the one-kernel attention cores write proj's int8 row plane (k_attn_qkpv_plane / k_wattn_qkpv_plane; proj= on
engine.attn_quant_forward / window_attn_quant_forward).  Per case, with `out` inside a NaN-filled buffer, on a
poisoned workspace of exactly the size asked for: (1) `core` is today's bits and meets the float64 consumer stage at check_out's bar;
(2) the plane is the oracle's quant_int of the head-merged core with proj's interval and width, byte for byte, padding zero; (3) `out`
equals today's chain bit for bit -- the same call without proj=, then linear_quant_forward(..., residual=, window=) -- and the float64
value (int64 GEMM of that plane with proj's integer weights, times the fp32 scale table, + bias, + the residual through the row map)
within s5.15's four fp32 roundings; (4) the launch records hold one plane-instance launch (the fallback cases: the kernels of today),
with a residual one k_lin_res and no forward sweep -- pack kernels carry no record: that proj's rows were not packed is what (2) on
that path shows --, the guards are intact and the buffer around out is still NaN.  P4V_FUSED_PROJ_OUT: the worst ratios go there.
Dv = 20 is a multiple of 4, so with the one-kernel bit it runs the ViT plane instance on dword stores (v65_d20) and falls back only
with the bit clear (v65_d20_fallback); Dv = 18 is the fallback behind the one-kernel fp32 core.  `lead`: the first launch of a
fallback case; core=False: the call without want_core (the fallback then keeps the fp32 core in its workspace)."""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from ptq4vit_amd.utils.models import window_reverse
from tests import fused_reference as fr
from tests import test_hip_fused_attention as fa
from tests import test_hip_fused_window_attention as wa
from tests.fused_common import merge_margins
from tests.test_hip_fused_residual import _bits, _framed, _layer      # (int32 view; out inside a NaN buffer; a Linear's engine keywords)
from tests.workspace_guard import Guard

pytestmark = pytest.mark.gpu
_MARGINS = {}
# res: None | "id" | a shift (the window map over images of (ih, iw) windows of ws x ws tokens); one: the one-kernel bit
Case = namedtuple("Case", "name shape twin mask a_bit bias res one img lead core", defaults=(8, True, None, True, None, None, True))
#        id                   (images, nW, H, N, D) / (B, H, M, N, D, Dv)
CASES = [Case("w7_h3_sos_shift",   (2, 4, 3, 49, 32), True, "shift", res=3, img=(2, 2)),       # Kp = 128 > C = 96; 392 rows; 17-row tile
         Case("w7_h1_plain_a4",    (1, 4, 1, 49, 32), False, None, 4, False, 0, img=(2, 2)),   # one head; map without a roll; 4-bit grid
         Case("n64_id",            (1, 2, 2, 64, 32), True, "shift", res="id"),                # 128 rows: no row padding
         Case("w12_nores",         (1, 4, 2, 144, 32), True, "shift"),                         # NT = 5, five row tiles
         Case("w7_d24",            (1, 2, 2, 49, 24), True, "shift", res="id"),                # dword stores; C = 48
         Case("w7_d16_plain",      (1, 2, 3, 49, 16), False, None),                            # half a tile per head
         Case("n196_fallback",     (1, 1, 2, 196, 32), True, "shift", res="id", lead="k_attn_qk", core=False),    # no instance: the kernels of today
         Case("v5_sos",            (2, 3, 5, 5, 64, 64), True, None, res="id"),                # NDT = 2, one live wave per z
         Case("v65_d80_plain",     (1, 3, 65, 65, 80, 80), False, None, 4),                    # NDT = 4 with 2.5 live tiles; Kp = 256 > 240
         Case("v197_d128",         (1, 3, 197, 197, 128, 128), True, None, res="id"),          # NDT = 4; two row tiles per z
         Case("v65_d20",           (1, 3, 65, 65, 20, 20), True, None, res="id"),              # the ViT instance on dword stores; C = 60
         Case("v65_d18_fallback",  (1, 3, 65, 65, 18, 18), True, None, lead="k_attn_qkpv", core=False),           # Dv % 4 != 0: fp32 core, head merge
         Case("v65_d20_fallback",  (1, 3, 65, 65, 20, 20), True, None, res="id", one=False, lead="k_attn_qk")]
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    yield engine
    engine.release_workspace()
    merge_margins(os.environ.get("P4V_FUSED_PROJ_OUT"), "engine", _MARGINS, IDS)


def _setup(case):
    """(the engine function's name, its keywords, matmul2, (B, H, M, Dv))"""
    from ptq4vit_amd.utils.fuse import _matmul_side
    seed = 3700 + IDS.index(case.name)
    if len(case.shape) == 5:
        images, nW, H, N, D = case.shape
        wc = wa.Case(case.name, case.shape, case.twin, 8, case.mask)
        q, kT, v, bias, mask = wa._inputs(wc, seed=seed)
        m1, m2 = fa._modules(wa._fa_case(wc), q, kT, v)
        kw, fn, dims = dict(bias=bias, mask=mask), "window_attn_quant_forward", (images * nW, H, N, D)
    else:
        B, H, M, N, D, Dv = case.shape
        g = torch.Generator().manual_seed(seed)
        q, k, v = (torch.randn(B, H, n, d, generator=g).cuda() for n, d in ((M, D), (N, D), (N, Dv)))
        kT = k.transpose(-2, -1)
        m1, m2 = fa._modules(fa.Case(case.name, case.shape, case.twin, (8, 8), (8, 8), 1.0, False), q, kT, v)
        kw, fn, dims = dict(scale=D ** -0.5), "attn_quant_forward", (B, H, M, Dv)
    if not case.twin:                                  # probabilities: absmax <= 1, a different factor per head
        m2.A_interval = (torch.tensor(fa.HEAD_FACTORS["pA"][:H], device="cuda") / (m2.A_qmax - 0.5)).view(1, H, 1, 1, 1, 1, 1)
    kw.update(q=q, kT=kT, v=v, qk=_matmul_side(m1, H), pv=_matmul_side(m2, H), one_kernel=case.one)
    return fn, kw, m2, dims


def _records(eng, call):
    eng.stats_enable(True)
    try:
        eng.stats_reset()
        res = call()
        torch.cuda.synchronize()
        return res, [r["kernel"] for r in eng.stats_launches()]
    finally:
        eng.stats_enable(False)


def _out_over_bar(out, layer, plane, residual):
    """|out - ref64| over s5.15's bar of four fp32 roundings, worst element; plane [M][K]: the integer row plane, in out's row order"""
    wi, _, s = fr._weight_plane(layer["weight"], layer["w_interval"], layer["w_bit"])
    acc = fr._imatmul(plane, wi.T).astype(fr.F64) * (fr.as_np(layer["a_interval"])[0] * s.reshape(1, -1)).astype(fr.F64)      # acc * the fp32 table
    bias = 0.0 if layer["bias"] is None else fr.as_np(layer["bias"]).astype(fr.F64).reshape(1, -1)
    r64 = 0.0 if residual is None else fr.as_np(residual).astype(fr.F64)
    bar = 4 * 2.0 ** -24 * (np.abs(acc) + np.abs(bias) + np.abs(r64))
    err = np.abs(fr.as_np(out).astype(fr.F64) - (acc + bias + r64))
    return float(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0)).max())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_core_writes_projs_plane(eng, monkeypatch, case):
    fn, kw, m2, (B, H, M, Dv) = _setup(case)
    call = getattr(eng, fn)
    C_, rows = H * Dv, B * M
    g = torch.Generator().manual_seed(3750 + IDS.index(case.name))
    aq = 1 << (case.a_bit - 1)
    proj = dict(_layer(g, C_, C_, bias=case.bias), a_bit=case.a_bit, a_interval=torch.tensor([1.5 / (aq - 0.5)]).cuda())
    window, rshape = None, (B, M, C_)
    if isinstance(case.res, int):
        ws, (ih, iw) = int(M ** 0.5), case.img
        window, rshape = (ih * ws, iw * ws, ws, case.res), (B // (ih * iw), ih * iw * M, C_)
    residual = torch.randn(rshape, generator=g).cuda() if case.res is not None else None
    buf, out = _framed(rshape)
    with torch.no_grad(), Guard(eng, monkeypatch, 0xCD) as guard:
        res, kernels = _records(eng, lambda: call(**kw, proj=proj, residual=residual, window=window, out=out, want_core=case.core, want_probs=True,
                                                  want_planes=True))
        reps = guard.finish()
        core0 = call(**kw)
        got, core, probs, plane = res if case.core else (res[0], core0, res[1], res[2])
        merged = core0.transpose(1, 2).reshape(B, M, C_)
        chain = eng.linear_quant_forward(x=merged, **proj, **(dict(residual=residual, window=window) if residual is not None else {}))
    assert got is out and all(r["guard_changed"] == 0 and 0 < r["touched"] <= r["need"] for r in reps), reps
    # 1: the core -- today's bits, and the float64 consumer stage of the call's own probabilities
    assert torch.equal(_bits(core), _bits(core0))
    planes, _, _ = fr.attn_planes_of(probs, H, **fa._pv_kw(m2))
    ref = fr.attn_consumer_stage(planes, kw["v"], H, sos=m2._sos, A_bit=m2.A_bit, B_bit=m2.B_bit, B_iv=m2.B_interval, A_iv=m2.A_interval,
                                 M=M, N=probs.shape[-1])
    s1 = fr.check_out(core, ref, probs.shape[-1], case.name)
    # 2: the plane, byte for byte, its padding zero
    want, _ = fr.int_plane(merged.reshape(rows, C_), fr.as_np(proj["a_interval"]), -aq, aq - 1)
    pl = plane.cpu().numpy().astype(np.int64)
    assert pl.shape[0] >= rows and pl.shape[0] % 128 == 0 and pl.shape[1] == (C_ + 63) // 64 * 64, pl.shape
    assert np.array_equal(pl[:rows, :C_], want), f"{int((pl[:rows, :C_] != want).sum())} of {want.size} plane bytes differ"
    assert not pl[rows:].any() and not pl[:, C_:].any(), "the plane's padding is not zero"
    # 3: out -- today's chain bit for bit, and float64 in the plane's row order (the residual gathered by the inverse map)
    assert torch.equal(_bits(out), _bits(chain.reshape(rshape))), f"{case.name}: not the unfused chain's bits"
    idx = torch.arange(rows, dtype=torch.float32).view(-1, 1)
    if window is not None:
        wh, ww, ws, shift = window
        idx = torch.roll(window_reverse(idx.view(-1, ws, ws, 1), ws, wh, ww), shifts=(shift, shift), dims=(1, 2))
    dst = torch.argsort(idx.reshape(-1))                               # dst[m]: the token row m goes to
    flat = lambda t: t.reshape(rows, C_).cpu()[dst]
    s3 = _out_over_bar(flat(out), proj, want, None if residual is None else flat(residual))
    print(f"[fused proj plane] {case.name}: |core - ref64| / bar {s1:.3f}; |out - ref64| / bar {s3:.3f}; {kernels}")
    _MARGINS.setdefault("out_over_bar", {})[case.name] = s3
    _MARGINS.setdefault("core_over_bar", {})[case.name] = s1
    assert s3 <= 1.0, (case.name, s3)
    # 4: the launches; nothing written around out
    inst = "k_attn_qkpv_plane" if fn == "attn_quant_forward" else "k_wattn_qkpv_plane"
    if case.lead is not None:
        assert inst not in kernels and kernels[0] == case.lead and (case.lead == "k_attn_qk" or "k_attn_qk" not in kernels), kernels
    else:
        assert kernels[0] == inst and kernels.count(inst) == 1 and not {"k_attn_qk", "k_attn_qkpv", "k_wattn_qkpv"} & set(kernels), kernels
        assert len(kernels) == 2 and (residual is None or kernels[1] == "k_lin_res"), kernels
    assert kernels.count("k_lin_res") == (residual is not None), kernels
    assert int(torch.isnan(buf).sum()) == buf.numel() - out.numel() and torch.isfinite(out).all()


#            id              message                   proj overrides      in_features  overlap
REFUSED = [("n_a2",         "n_H = n_a = 1",          {"n_a": 2},         96,          False),
           ("postgelu",     "twin_postgelu",          {"postgelu": True}, 96,          False),
           ("in_features",  "head-merged",            {},                 64,          False),
           ("overlap",      "overlaps the residual",  {},                 96,          True)]


@pytest.mark.parametrize("name,msg,over,K,overlap", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_before_any_launch(eng, monkeypatch, name, msg, over, K, overlap):
    fn, kw, _, (B, H, M, Dv) = _setup(CASES[0])
    g, n = torch.Generator().manual_seed(3790), B * M * 96
    proj, buf = dict(_layer(g, 96, K), **over), torch.randn(n + 8, generator=g).cuda()
    residual = buf[:n].view(B, M, 96)
    out = buf[4:4 + n].view(B, M, 96) if overlap else torch.full_like(residual, float("nan"))
    before_bits = _bits(out).clone()
    with torch.no_grad(), Guard(eng, monkeypatch, 0xCD) as guard:
        torch.cuda.synchronize()
        before = eng.launch_counters()
        with pytest.raises((NotImplementedError, RuntimeError), match=msg):
            getattr(eng, fn)(**kw, proj=proj, residual=residual, out=out)
        assert eng.launch_counters() == before and all(r["touched"] == 0 and r["guard_changed"] == 0 for r in guard.finish())
    assert torch.equal(_bits(out), before_bits)
