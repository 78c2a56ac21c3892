"""GPU: the one-kernel window attention core (P4V_WATTN_ONE_KERNEL; k_wattn_qkpv; engine.window_attn_quant_forward(one_kernel=True)).

k_wattn_qkpv keeps a window's whole score row in registers: scores, bias and mask are produced once, the quantised probabilities
feed matmul2's int8 MFMAs from registers.  Per case, on a poisoned workspace of exactly the size asked for:
1. `out` and `probs` equal the two-kernel window call's bit for bit (NaNs as equal bit patterns): the probabilities come from the
   same operations in the same order, integer accumulation is exact, the epilogue is the forward sweep's expression;
2. `probs` against the float64 softmax within U_row (tests/fused_window_reference.py); `out` against the int64 GEMM of the oracle's
   quantiser of the call's own probs with quant_int(v), in float64, at the consumer stage's bar 2e-6 sqrt(K);
3. the launch record holds the new kind alone and the workspace is smaller -- or, where the kernel has no instance (more than
   160 keys, Dv > 32), the two-kernel chain's launches and size;
4. with P4V_FUSED_WPV_OUT set the worst ratios are written there (profiles/r34_fused_wpv_margins.json).
Then the contract (want_planes, one byte less, the debug record) and the tiny Swin's logits.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import fused_reference as fr
from tests import fused_window_reference as fw
from tests import test_hip_fused_attention as fa
from tests import test_hip_fused_window_attention as wa
from tests.fused_common import merge_margins
from tests.test_hip_fused_window_attention import tiny  # noqa: F401  (the calibrated tiny Swin, built as that file builds it)
from tests.workspace_guard import Guard

pytestmark = pytest.mark.gpu

_MARGINS = {}
W7 = (2, 4, 3, 49, 32)
#                  id                 (images, nW, H, N, D)  twin   bits  mask     strided
CASES = [wa.Case("w7_sos_mask",       W7,                    True,  8,    "shift"),        # NT = 2, ragged key tile, 17-row tile, dwords
         wa.Case("w7_plain_nomask",   W7,                    False, 8,    None),           # PACK_SYM, no mask
         wa.Case("w7_one_window",     (1, 1, 3, 49, 32),     True,  8,    "shift"),        # six waves: two of a workgroup return
         wa.Case("n64",               (1, 2, 2, 64, 32),     True,  8,    "shift"),        # NT = 2, both tiles full
         wa.Case("n65",               (1, 2, 2, 65, 32),     True,  8,    "shift"),        # NT = 5 with three live tiles
         wa.Case("w12_sos_mask",      (1, 4, 2, 144, 32),    True,  8,    "shift"),        # five row tiles, 16-byte loads
         wa.Case("n160",              (1, 2, 2, 160, 32),    False, 8,    "shift"),        # the instance's cap
         wa.Case("n161_two_kernels",  (1, 2, 2, 161, 32),    True,  8,    "shift"),        # no instance: the two-kernel chain
         wa.Case("d12_w6",            (2, 4, 2, 49, 12),     True,  6,    "shift"),        # the tiny Swin's head_dim, 6 bit
         wa.Case("d30",               (1, 2, 2, 49, 30),     True,  8,    "shift"),        # Dv % 4 != 0: scalar stores of out
         wa.Case("d40_two_kernels",   (1, 2, 2, 49, 40),     True,  8,    "shift"),        # Dv > 32: the two-kernel chain
         wa.Case("strided",           W7,                    True,  8,    "shift", True),
         wa.Case("mask_neg_inf",      W7,                    True,  8,    "inf"),
         wa.Case("row_all_masked",    W7,                    True,  8,    "row"),
         wa.Case("zero_q_head",       W7,                    False, 8,    "shift")]
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    yield engine
    engine.release_workspace()
    merge_margins(os.environ.get("P4V_FUSED_WPV_OUT"), "window_attention_pv", _MARGINS, IDS)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _call_args(case):
    from ptq4vit_amd.utils.fuse import _matmul_side
    H = case.shape[2]
    zero = 1 if case.name == "zero_q_head" else None
    q, kT, v, bias, mask = wa._inputs(case, seed=3400 + IDS.index(case.name), zero_q_head=zero)
    m1, m2 = fa._modules(wa._fa_case(case), q, kT, v)
    if not case.twin:                                  # probabilities: absmax <= 1, a different factor per head
        m2.A_interval = (torch.tensor(fa.HEAD_FACTORS["pA"][:H], device="cuda") / (m2.A_qmax - 0.5)).view(1, H, 1, 1, 1, 1, 1)
    kw = dict(q=q, kT=kT, v=v, bias=bias, mask=mask, qk=_matmul_side(m1, H), pv=_matmul_side(m2, H))
    return kw, m1, m2


def _guarded(eng, monkeypatch, call):
    """`call()` on a poisoned workspace of exactly the size asked for; returns (its result, the bytes asked for)"""
    with torch.no_grad(), Guard(eng, monkeypatch, 0xCD) as g:
        res = call()
        reps = g.finish()
    assert len(reps) == 1 and reps[0]["guard_changed"] == 0 and 0 < reps[0]["touched"] <= reps[0]["need"], reps
    return res, reps[0]["need"]


def _launches(eng, kw, one):
    eng.stats_enable(True)
    try:
        eng.stats_reset()
        with torch.no_grad():
            eng.window_attn_quant_forward(**kw, one_kernel=one)
        torch.cuda.synchronize()
        return [r["kernel"] for r in eng.stats_launches()]
    finally:
        eng.stats_enable(False)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_kernel_is_the_two_kernel_window_chain_bit_for_bit(eng, monkeypatch, case):
    images, nW, H, N, D = case.shape
    kw, m1, m2 = _call_args(case)
    (out2, probs2), need2 = _guarded(eng, monkeypatch, lambda: eng.window_attn_quant_forward(**kw, want_probs=True))
    (out1, probs1), need1 = _guarded(eng, monkeypatch, lambda: eng.window_attn_quant_forward(**kw, want_probs=True, one_kernel=True))
    # 1: the same bits
    assert out1.shape == (images * nW, H, N, D) and torch.equal(_bits(probs1), _bits(probs2))
    assert torch.equal(_bits(out1), _bits(out2)), f"{int((_bits(out1) != _bits(out2)).sum())} of {out1.numel()} outputs differ"
    # 2: the float64 stage references
    st = fw.window_float_stage(kw["q"], kw["kT"], m1.A_interval, m1.B_interval, m1.A_bit, m1.B_bit, kw["bias"], kw["mask"])
    s1, _ = fw.check_window_probs(probs1, st, case.name)
    planes, nan, _ = fr.attn_planes_of(probs1, H, **fa._pv_kw(m2))
    skip = np.zeros((1, H, 1, 1), bool)
    if case.name == "zero_q_head":
        assert torch.isnan(probs1[:, 1]).all() and torch.isfinite(out1[:, [0, 2]]).all()
        skip[0, 1] = True                              # (the NaN head's plane bytes are undefined)
    else:
        assert not nan.any()
    ref = fr.attn_consumer_stage(planes, kw["v"], H, sos=m2._sos, A_bit=m2.A_bit, B_bit=m2.B_bit, B_iv=m2.B_interval,
                                 A_iv=m2.A_interval, M=N, N=N)
    s3 = fr.check_out(out1, ref, N, case.name, skip=skip)
    # 3: the launches and the workspace
    two = _launches(eng, kw, False)
    one = _launches(eng, kw, True)
    assert two[0] == "k_attn_qk" and len(two) == 2 and "k_wattn_qkpv" not in two, two
    if case.name.endswith("two_kernels"):
        assert one == two and need1 == need2
    else:
        assert one == ["k_wattn_qkpv"] and 0 < need1 < need2, (one, need1, need2)
    print(f"[fused wpv] {case.name}: |probs - p64| / bound {s1:.3f}; |out - ref| / bar {s3:.3f}; workspace {need1} vs {need2}; {one}")
    _MARGINS.setdefault("stage_ratios", {})[case.name] = dict(probs_over_bound=s1, out_over_bar=s3, ws_one=need1, ws_two=need2)


def test_contract(eng, monkeypatch):
    from ptq4vit_amd import _lib
    kw, _, _ = _call_args(CASES[0])
    with torch.no_grad():
        with pytest.raises(ValueError, match="want_planes"):
            eng.window_attn_quant_forward(**kw, one_kernel=True, want_planes=True)
        # one byte less: refused, nothing launched
        torch.cuda.synchronize()
        before = eng.launch_counters()
        with Guard(eng, monkeypatch, 0xCD, declare=lambda n: n - 1) as g:
            with pytest.raises(RuntimeError, match="workspace too small"):
                eng.window_attn_quant_forward(**kw, one_kernel=True)
            reps = g.finish()
        assert eng.launch_counters() == before and all(r["touched"] == 0 and r["guard_changed"] == 0 for r in reps), reps
        # no plane of matmul2 exists after a one-kernel call
        eng.window_attn_quant_forward(**kw, one_kernel=True)
        info = (C.c_uint64 * 5)()
        _lib.check(_lib.load().p4v_debug_attn_planes(info), "p4v_debug_attn_planes")
        assert list(info) == [0, 0, 0, 0, 1]


def test_tiny_swin_logits_bit_for_bit(eng, tiny, monkeypatch):  # noqa: F811
    from ptq4vit_amd.utils import fuse
    net, wrapped, images = tiny
    watts = wa._window_names(net)
    seen = []
    orig = eng.window_attn_quant_forward
    monkeypatch.setattr(eng, "window_attn_quant_forward", lambda **kw: (seen.append(kw.get("one_kernel")), orig(**kw))[1])
    try:
        with torch.no_grad():
            y_u = net(images)
            for with_mlp in (False, True):
                if with_mlp:
                    fuse.fuse_mlp(net)
                assert fuse.fuse_window_attention(net) == watts
                y2 = net(images)
                assert fuse.fuse_window_attention(net, one_kernel=True) == watts
                del seen[:]
                y1 = net(images)
                assert seen == [True] * len(watts) and torch.equal(_bits(y1), _bits(y2))
            fuse.unfuse_mlp(net)
            assert fuse.unfuse_window_attention(net) == watts
            del seen[:]
            assert torch.equal(net(images), y_u) and not seen
            assert all(fuse._WONE_KERNEL not in m.__dict__ for m in net.modules())
    finally:
        fuse.unfuse_mlp(net)
        fuse.unfuse_window_attention(net)
