"""GPU: the one-kernel attention core (P4V_ATTN_ONE_KERNEL; k_attn_qkpv; engine.*attn_quant_forward(one_kernel=True)).

k_attn_qkpv is k_attn_qk whose third walk feeds the quantised probabilities, in registers, to matmul2's int8 MFMAs.  Per case, on
a poisoned workspace of exactly the size asked for:
1. `out` and `probs` equal the two-kernel call's bit for bit (NaNs as equal bit patterns): integer accumulation is exact and
   order-free, the epilogue is the forward sweep's expression -- no tolerance to choose;
2. `out` against the int64 GEMM of the oracle's quantiser of the call's own probs with quant_int(v), in float64, at the consumer
   stage's bar 2e-6 sqrt(K); `probs` against the float64 softmax within U_row (tests/fused_reference.py);
3. with P4V_FUSED_PV_OUT set the worst ratios are written there (profiles/r33_fused_pv_margins.json).
Then the qkv entry point, the workspace contract, the launch records, the Dv > 128 fallback and the mini ViT.
"""
import json
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import fused_reference as fr
from tests.fused_common import _Loader, _count_fused_calls, merge_margins
from tests.workspace_guard import Guard

pytestmark = pytest.mark.gpu

SPLIT = 2.0 ** -5
FACTORS = {"qA": (1.0, 0.8, 1.25), "qB": (0.9, 1.15, 1.0), "pA": (1.1, 0.9, 1.0), "pB": (1.2, 1.0, 0.85)}
_MARGINS = {}

Case = namedtuple("Case", "name shape sos bits strided zero_v", defaults=((8, 8), False, False))
#               id              (batch, H, M, N, D, Dv)        sos
CASES = [Case("n5",             (2, 3, 5, 5, 64, 64),          True),      # one partial tile, padding keys and queries
         Case("n197_sos",       (2, 3, 197, 197, 64, 64),      True),      # production: 7 key tiles, the last one partial
         Case("n197_plain",     (2, 3, 197, 197, 64, 64),      False),     # PACK_SYM head-wise, no second accumulator
         Case("d40",            (2, 3, 50, 50, 40, 40),        True),      # Dv no multiple of 32 (24 dead columns), K1p padding
         Case("d128",           (1, 2, 130, 130, 128, 128),    True),      # NDT = 4, the ktiles = 2 score tile
         Case("m64_n130_dv96",  (1, 2, 64, 130, 64, 96),       False),     # M != N, Dv != D, Dv in the NDT = 4 instance
         Case("m1",             (2, 3, 1, 197, 64, 64),        True),      # a single live row
         Case("n321",           (1, 2, 321, 321, 64, 64),      True),      # past Kp = 256, off the b64 column plane
         Case("a2b8",           (1, 2, 197, 197, 64, 64),      True, (2, 8)),   # narrow clamp ranges
         Case("strided",        (2, 3, 197, 197, 64, 64),      True, (8, 8), True),
         Case("zero_v_head",    (2, 3, 197, 197, 64, 64),      True, (8, 8), False, True)]
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    yield engine
    engine.release_workspace()
    merge_margins(os.environ.get("P4V_FUSED_PV_OUT"), "attention_pv", _MARGINS, IDS)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _iv(x, qmax, factors):
    """the min-max rule per head, absmax / (q - 0.5), times a different factor per head (a wrong head index shows); 0 stays 0"""
    return x.abs().amax(dim=(0, 2, 3)) / (qmax - 0.5) * torch.tensor(factors[:x.shape[1]], device=x.device)


def _operands(case):
    B, H, M, N, D, Dv = case.shape
    g = torch.Generator().manual_seed(3300 + IDS.index(case.name))
    if case.strided:                                   # views of a packed qkv buffer [B][N][3][H][D], as Attention.forward has them
        q, k, v = torch.randn(B, N, 3, H, D, generator=g).cuda().permute(2, 0, 3, 1, 4).unbind(0)
        assert not q.is_contiguous() and not v.is_contiguous()
    else:
        q, k, v = (torch.randn(B, H, r, c, generator=g).cuda() for r, c in ((M, D), (N, D), (N, Dv)))
    if case.zero_v:
        v = v.clone()
        v[:, 1] = 0.0
    return q, k.transpose(-2, -1), v


def _sides(case, q, kT, v):
    H = q.shape[1]
    a, b = (2 ** (bit - 1) for bit in case.bits)
    qk = dict(A_interval=_iv(q, 128, FACTORS["qA"]), B_interval=_iv(kT, 128, FACTORS["qB"]), split=None, A_bit=8, B_bit=8, sos=False)
    pv = dict(B_interval=_iv(v, b, FACTORS["pB"]), A_bit=case.bits[0], B_bit=case.bits[1], sos=case.sos)
    if case.sos:
        pv["split"] = torch.tensor(SPLIT, device="cuda")
        pv["A_interval"] = torch.tensor(float(np.float32(SPLIT) / np.float32(a - 1)), device="cuda")        # split / (q - 1)
    else:
        pv["split"] = None
        pv["A_interval"] = torch.tensor(FACTORS["pA"][:H], device="cuda") / (a - 0.5)                      # probabilities: absmax <= 1
    return qk, pv


def _guarded(eng, monkeypatch, call):
    """`call()` on a poisoned workspace of exactly the size asked for; returns (its result, the bytes asked for)"""
    with torch.no_grad(), Guard(eng, monkeypatch, 0xCD) as g:
        res = call()
        reps = g.finish()
    assert len(reps) == 1 and reps[0]["guard_changed"] == 0 and 0 < reps[0]["touched"] <= reps[0]["need"], reps
    return res, reps[0]["need"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_kernel_is_the_two_kernel_chain_bit_for_bit(eng, monkeypatch, case):
    B, H, M, N, D, Dv = case.shape
    q, kT, v = _operands(case)
    qk, pv = _sides(case, q, kT, v)
    kw = dict(q=q, kT=kT, v=v, scale=D ** -0.5, qk=qk, pv=pv, want_probs=True)
    (out2, probs2), need2 = _guarded(eng, monkeypatch, lambda: eng.attn_quant_forward(**kw))
    (out1, probs1), need1 = _guarded(eng, monkeypatch, lambda: eng.attn_quant_forward(**kw, one_kernel=True))
    assert need1 < need2
    # 1: the same bits
    assert out1.shape == (B, H, M, Dv) and torch.equal(_bits(probs1), _bits(probs2))
    assert torch.equal(_bits(out1), _bits(out2)), f"{int((_bits(out1) != _bits(out2)).sum())} of {out1.numel()} outputs differ"
    if case.zero_v:
        assert torch.isnan(out1[:, 1]).all() and torch.isfinite(out1[:, [0, 2]]).all()
    # 2: the float64 stage references
    u64, p64 = fr.attn_float_stage(q, kT, qk["A_interval"], qk["B_interval"], 8, 8, D ** -0.5)
    s1 = fr.check_probs(probs1, u64, p64, case.name)
    planes, nan, _ = fr.attn_planes_of(probs1, H, sos=case.sos, A_bit=case.bits[0], split=pv["split"], A_iv=pv["A_interval"])
    assert not nan.any()
    ref = fr.attn_consumer_stage(planes, v, H, sos=case.sos, A_bit=case.bits[0], B_bit=case.bits[1], B_iv=pv["B_interval"],
                                 A_iv=pv["A_interval"], M=M, N=N)
    s3 = fr.check_out(out1, ref, N, case.name)
    print(f"[fused pv] {case.name}: |probs - p64| / bound {s1:.3f}; |out - ref| / bar {s3:.3f}; workspace {need1} < {need2}")
    _MARGINS.setdefault("stage_ratios", {})[case.name] = dict(probs_over_bound=s1, out_over_bar=s3, ws_one=need1, ws_two=need2)


def _qkv_args(eng):
    B, N, H, D, K = 2, 197, 3, 64, 192
    g = torch.Generator().manual_seed(3390)
    x = torch.randn(B, N, K, generator=g).cuda()
    W = (torch.randn(3 * H * D, K, generator=g) * K ** -0.5).cuda()
    bias = (torch.randn(3 * H * D, generator=g) * 0.2).cuda()
    lin = dict(weight=W, bias=bias, w_interval=W.reshape(3, -1).abs().amax(1) / 127.5, a_interval=x.abs().amax().reshape(1) / 127.5,
               w_bit=8, a_bit=8, n_V=3, n_H=1, n_a=1)
    with torch.no_grad():
        q, k, v = eng.linear_quant_forward(x=x, **lin).reshape(B, N, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
    qk, pv = _sides(Case("qkv", (B, H, N, N, D, D), True), q, k.transpose(-2, -1), v)
    return dict(x=x, qkv=lin, scale=D ** -0.5, qk=qk, pv=pv, want_probs=True, want_planes=True)


def test_qkv_entry_point_bit_for_bit(eng, monkeypatch):
    kw = _qkv_args(eng)
    (out2, probs2, planes2), need2 = _guarded(eng, monkeypatch, lambda: eng.qkv_attn_quant_forward(**kw))
    (out1, probs1, planes1), need1 = _guarded(eng, monkeypatch, lambda: eng.qkv_attn_quant_forward(**kw, one_kernel=True))
    assert need1 < need2 and len(planes2) == 5 and len(planes1) == 3          # (Q, Kt, V): no P1 / P2
    assert torch.equal(_bits(out1), _bits(out2)) and torch.equal(_bits(probs1), _bits(probs2))
    assert all(torch.equal(a, b) for a, b in zip(planes1, planes2))


def test_workspace_records_and_fallback(eng, monkeypatch):
    case = CASES[IDS.index("n197_sos")]
    q, kT, v = _operands(case)
    qk, pv = _sides(case, q, kT, v)
    kw = dict(q=q, kT=kT, v=v, scale=0.125, qk=qk, pv=pv)
    with torch.no_grad():
        with pytest.raises(ValueError, match="want_planes"):
            eng.attn_quant_forward(**kw, one_kernel=True, want_planes=True)
        # one byte less: refused, nothing launched
        torch.cuda.synchronize()
        before = eng.launch_counters()
        with Guard(eng, monkeypatch, 0xCD, declare=lambda n: n - 1) as g:
            with pytest.raises(RuntimeError, match="workspace too small"):
                eng.attn_quant_forward(**kw, one_kernel=True)
            reps = g.finish()
        assert eng.launch_counters() == before and all(r["touched"] == 0 and r["guard_changed"] == 0 for r in reps), reps
        # the launch records: the new kind alone; a default call's list is what it was
        eng.stats_enable(True)
        try:
            lists = {}
            for one in (False, True):
                eng.stats_reset()
                eng.attn_quant_forward(**kw, one_kernel=one)
                torch.cuda.synchronize()
                lists[one] = [r["kernel"] for r in eng.stats_launches()]
        finally:
            eng.stats_enable(False)
        assert lists[True] == ["k_attn_qkpv"] and lists[False] == ["k_attn_qk", "k_sweep2"], lists
        # Dv = 160: no instance -- the two-kernel chain, its workspace, its result
        v160 = torch.randn(2, 3, 197, 160, generator=torch.Generator().manual_seed(3391)).cuda()
        kw160 = dict(kw, v=v160, pv=dict(pv, B_interval=_iv(v160, 128, FACTORS["pB"])))
    out2, need2 = _guarded(eng, monkeypatch, lambda: eng.attn_quant_forward(**kw160))
    out1, need1 = _guarded(eng, monkeypatch, lambda: eng.attn_quant_forward(**kw160, one_kernel=True))
    assert need1 == need2 and torch.equal(_bits(out1), _bits(out2))


def test_mini_vit_logits_bit_for_bit(eng, monkeypatch):
    from ptq4vit_amd.configs import PTQ4ViT
    from ptq4vit_amd.utils import fuse, models, net_wrap
    from ptq4vit_amd.utils.quant_calib import HessianQuantCalibrator
    g = np.load("tests/golden/minivit_ptq4vit.npz", allow_pickle=False)
    net = models.get_net("vit_tiny_patch16_224", seed=0, device="cuda", **json.loads(str(g["model_kwargs"])))
    wrapped = net_wrap.wrap_modules_in_net(net, PTQ4ViT)
    images = torch.from_numpy(g["images"][:4]).cuda()
    HessianQuantCalibrator(net, wrapped, _Loader(images), sequential=False, batch_size=4).batching_quant_calib()
    attns = [n for n, m in net.named_modules() if isinstance(m, models.Attention)]
    seen = []
    orig = eng.qkv_attn_quant_forward
    monkeypatch.setattr(eng, "qkv_attn_quant_forward", lambda **kw: (seen.append(kw.get("one_kernel")), orig(**kw))[1])
    with torch.no_grad():
        y_u = net(images)
        for with_mlp in (False, True):
            if with_mlp:
                fuse.fuse_mlp(net)
            assert fuse.fuse_qkv_attention(net) == attns
            y2 = net(images)
            assert fuse.fuse_qkv_attention(net, one_kernel=True) == attns
            del seen[:]
            y1 = net(images)
            assert seen == [True] * len(attns) and torch.equal(_bits(y1), _bits(y2))
        # a hooked matmul2: that block falls back to the original forward
        mods = dict(net.named_modules())
        h = mods[attns[0]].matmul2.register_forward_hook(lambda mod, inp, out: None)
        del seen[:]
        net(images)
        h.remove()
        assert seen == [True] * (len(attns) - 1)
        fuse.unfuse_mlp(net)
        assert fuse.unfuse_attention(net) == attns
        calls = _count_fused_calls(eng, monkeypatch, "qkv_attn_quant_forward")
        assert torch.equal(net(images), y_u) and not calls
        assert all("forward" not in mods[n].__dict__ and fuse._ONE_KERNEL not in mods[n].__dict__ for n in attns)
