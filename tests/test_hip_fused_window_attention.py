"""GPU: the fused int8 window attention forward (p4v_wattn_quant_forward, engine.window_attn_quant_forward,
utils/fuse.py::fuse_window_attention) -- Swin's WindowAttention: q scaled before matmul1, the relative-position bias and the
shift mask added before the softmax.

The window instances of k_attn_qk compute matmul1's int8 GEMM, `+ bias[head]`, `+ mask[window]` (two separate fp32 additions),
the softmax over the keys and matmul2's A quantiser and write matmul2's int8 row plane(s); the chain around them is the plain
fused attention forward's.  The structure and the helpers are those of tests/test_hip_fused_attention.py (imported, not copied);
per case, on a poisoned workspace of exactly the size asked for, with a bias that differs per head and a mask that differs per
window (a wrong index shows):

1. the planes are, byte for byte and padding included, what the packers make of the call's own probs;
2. `out` is matmul2.quant_forward(probs, v), bit for bit;
3. probs and torch's softmax(matmul1.quant_forward(q, kT) + bias (+ mask)), both in fp32 ulps against the float64 softmax of the
   same fp32 scores: U_k <= max(2 U_t, 8), taken where the float64 stage reference is >= 2^-100 (a masked key at -100 is a
   subnormal fp32 number on either side);
4. against the unfused chain the tie rule of the plain test holds for differing plane bytes;
5. the float64 stage references: tests/fused_window_reference.py for probs (its bar, and: every entry below 2^-100 is a masked
   entry of a row that still has an unmasked key), fused_reference's check_planes / check_out unchanged;
6. the contract: exact workspace, one byte less, the new refusals, null probs, null mask;
7. a zero q head poisons that head alone.

Cases, as (images, nW, H, N, D): window 7 (49 tokens: the second wave of the row tile ragged with 17 rows, the second key tile
ragged, Kp = 64, the window index wrapping over two images) with split-of-softmax and plain matmul2, with and without mask;
window 12 (144 tokens: two row tiles, the second with 16 live rows, Kp = 192, the last 64-key chunk half empty); head_dim 12 at
6 bit (the tiny Swin's); q / k / v as views of the permuted qkv tensor; 64 tokens (no ragged key tile); one window per image;
one row whose keys are all at -100 (ordinary probabilities); partial rows at -inf; bias std 4 with q x 6.

Module level, on a tiny Swin calibrated on the GPU: 4 fused calls per forward, fused against unfused logits held to the plane
bytes that differ on the unfused net's own window tensors, the three fusions in two orders, the raw / hooked / CPU / autograd
states falling back bit-identically, a second calibration of the fused net giving the unfused net's intervals, unfuse restoring.

With P4V_FUSED_WATTN_OUT set the measured margins are written there, under "window_attention"
(profiles/r26_fused_wattn_margins.json).
"""
import copy
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import fused_reference as fr
from tests import fused_window_reference as fw
from tests import test_hip_fused_attention as fa
from tests.fused_common import _Loader, _count_fused_calls, _intervals, _wrapped_of, merge_margins, ulp_distance
from tests.workspace_guard import Guard

pytestmark = pytest.mark.gpu

_MARGINS = {}
Case = namedtuple("Case", "name shape twin bits mask strided bstd qf", defaults=(False, 0.5, 1.0))
W7 = (2, 4, 3, 49, 32)
#               id                 (images, nW, H, N, D)  twin   bits  mask     strided  bias std  q factor
CASES = [Case("w7_sos_mask",       W7,                    True,  8,    "shift"),
         Case("w7_sos_nomask",     W7,                    True,  8,    None),
         Case("w7_plain_mask",     W7,                    False, 8,    "shift"),
         Case("w12_sos_mask",      (1, 4, 2, 144, 32),    True,  8,    "shift"),
         Case("w7_d12_w6",         (2, 4, 2, 49, 12),     True,  6,    "shift"),
         Case("w7_strided",        W7,                    True,  8,    "shift", True),
         Case("n64",               (1, 2, 2, 64, 32),     True,  8,    "shift"),
         Case("one_window_mask",   (2, 1, 2, 49, 32),     True,  8,    "shift"),
         Case("row_all_masked",    W7,                    True,  8,    "row"),
         Case("mask_neg_inf",      W7,                    True,  8,    "inf"),
         Case("peaked_bias",       W7,                    True,  8,    "shift", False,   4.0,      6.0)]
IDS = [c.name for c in CASES]
ROW_ALL_MASKED = (1, 5)                       # (window, query) of row_all_masked


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    yield engine
    engine.release_workspace()
    merge_margins(os.environ.get("P4V_FUSED_WATTN_OUT"), "window_attention", _MARGINS, IDS)


def _inputs(case, seed=None, zero_q_head=None, device="cuda"):
    """q (scaled), kT, v as WindowAttention.forward hands them over -- q the product of a view of the qkv Linear's output
    [B_][N][3][H][D] with the scale, k and v views of it --, the bias [H][N][N] and the mask [nW][N][N] or None."""
    images, nW, H, N, D = case.shape
    B_ = images * nW
    seed = 2600 + IDS.index(case.name) if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B_, N, 3, H, D, generator=g)
    qkv[:, :, 0] *= case.qf
    if zero_q_head is not None:
        qkv[:, :, 0, zero_q_head] = 0.0
    qkv = qkv.to(device).permute(2, 0, 3, 1, 4)
    if not case.strided:
        qkv = qkv.contiguous()
    q, k, v = qkv.unbind(0)
    q = q * D ** -0.5
    if case.strided:
        assert not q.is_contiguous() and not k.is_contiguous() and not v.is_contiguous()
    bias = (torch.randn(H, N, N, generator=g) * case.bstd).to(device)
    mask = None
    if case.mask is not None:
        rng = np.random.default_rng(seed)
        m = fw.shift_mask(nW + 1, N, rng, -np.inf if case.mask == "inf" else -100.0)[1:]      # (every window masked somewhere)
        if case.mask == "row":
            m[ROW_ALL_MASKED] = -100.0
        assert len({w.tobytes() for w in m}) == nW
        mask = torch.from_numpy(m).to(device)
    return q, k.transpose(-2, -1), v, bias, mask


def _unfused_scores(m1, q, kT, bias, mask):
    """WindowAttention.forward between matmul1 and the softmax"""
    attn = m1.quant_forward(q, kT)
    B_, H, N, _ = attn.shape
    attn = attn + bias.unsqueeze(0)
    if mask is not None:
        nW = mask.shape[0]
        attn = (attn.view(B_ // nW, nW, H, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, H, N, N)
    return attn


def _fa_case(case):
    images, nW, H, N, D = case.shape
    return fa.Case(case.name, (images * nW, H, N, N, D, D), case.twin, (case.bits,) * 2, (case.bits,) * 2, case.qf, case.strided)


_RUNS = {}


def _run(eng, monkeypatch, case, key, **inp):
    """One fused call (exact, guarded, poisoned workspace) and the unfused chain next to it"""
    if key in _RUNS:
        return _RUNS[key]
    from ptq4vit_amd.utils.fuse import _matmul_side
    images, nW, H, N, D = case.shape
    q, kT, v, bias, mask = _inputs(case, **inp)
    m1, m2 = fa._modules(_fa_case(case), q, kT, v)
    with torch.no_grad():
        u_ref = _unfused_scores(m1, q, kT, bias, mask)
        p_ref = u_ref.softmax(dim=-1)
        if not case.twin:
            m2.A_interval = fa._headwise(torch.nan_to_num(p_ref), (0, 2, 3), m2.A_qmax, fa.HEAD_FACTORS["pA"])
        out_ref = m2.quant_forward(p_ref, v)
        p64 = torch.softmax(u_ref.double().cpu(), dim=-1).float().cuda()
        sides = _matmul_side(m1, H), _matmul_side(m2, H)
        with Guard(eng, monkeypatch, 0xCD) as g:
            out, probs, planes = eng.window_attn_quant_forward(q=q, kT=kT, v=v, bias=bias, mask=mask, qk=sides[0], pv=sides[1],
                                                               want_probs=True, want_planes=True)
            reps = g.finish()
        assert len(reps) == 1 and reps[0]["guard_changed"] == 0 and 0 < reps[0]["touched"] <= reps[0]["need"], reps
    st = fw.window_float_stage(q, kT, m1.A_interval, m1.B_interval, m1.A_bit, m1.B_bit, bias, mask)
    with np.errstate(invalid="ignore"):
        live = torch.from_numpy(~np.isnan(st["p64"]) & (st["p64"] >= fr.P_FLOOR)).cuda()
    r = dict(m1=m1, m2=m2, q=q, kT=kT, v=v, bias=bias, mask=mask, sides=sides, out=out, probs=probs, planes=planes, u_ref=u_ref,
             p_ref=p_ref, p64=p64, out_ref=out_ref, need=reps[0]["need"], live=live, stage=st)
    _RUNS[key] = r
    return r


def run_case(eng, monkeypatch, case):
    return _run(eng, monkeypatch, case, case.name)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_planes_are_the_packers_bytes_of_the_calls_own_probs(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    images, nW, H, N, D = case.shape
    Z = images * nW * H
    want = fa._packed(eng, r["m2"], r["probs"])
    assert len(want) == len(r["planes"]) == (2 if case.twin else 1)
    for got, ref in zip(r["planes"], want):
        assert got.shape[0] == Z and got.shape[1] == (N + 127) // 128 * 128 and got.shape[2] == ref.shape[2] == (N + 63) // 64 * 64
        for z in range(Z):
            assert torch.equal(got[z, :N], ref[z]), f"{case.name} z {z}: {(got[z, :N] != ref[z]).sum().item()} bytes differ from the packer's"
        assert not got[:, N:].any(), "padding rows must be zero"
        assert not got[:, :, N:].any(), "padding columns must be zero"
    assert r["planes"][0].any() and (not case.twin or r["planes"][1].any())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_out_is_matmul2_quant_forward_of_the_calls_own_probs(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    images, nW, H, N, D = case.shape
    with torch.no_grad():
        want = r["m2"].quant_forward(r["probs"], r["v"])
    assert r["out"].shape == want.shape == (images * nW, H, N, D)
    assert torch.equal(r["out"], want), f"{case.name}: max |diff| {(r['out'] - want).abs().max().item():.3e}"


def _ulps(r):
    """(U_t, U_k, U): torch and the kernel against the rounded float64 softmax, and the kernel against torch, where the stage
    reference is >= 2^-100"""
    live = r["live"]
    return (int(ulp_distance(r["p_ref"], r["p64"])[live].max()), int(ulp_distance(r["probs"], r["p64"])[live].max()),
            int(ulp_distance(r["probs"], r["p_ref"])[live].max()))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_softmax_is_as_close_to_float64_as_torchs(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    assert torch.isfinite(r["probs"]).all()
    assert float((r["probs"].sum(-1) - 1).abs().max()) < 1e-5
    U_t, U_k, U = _ulps(r)
    print(f"[fused wattn] {case.name}: ulps vs float64: torch {U_t}, kernel {U_k}; kernel vs torch {U}")
    _MARGINS.setdefault("softmax_ulp", {})[case.name] = dict(torch_vs_f64=U_t, kernel_vs_f64=U_k, kernel_vs_torch=U)
    assert U_k <= max(2 * U_t, fa.ULP_FLOOR), f"{case.name}: kernel {U_k} ulp, torch {U_t} ulp"
    if case.mask == "inf":
        dead = torch.isinf(r["mask"])[torch.arange(r["probs"].shape[0], device="cuda") % r["mask"].shape[0]].unsqueeze(1).expand_as(r["probs"])
        assert dead.any() and bool((r["probs"][dead] == 0).all()), "a -inf mask entry gives probability 0"
    if case.mask == "row":
        w, m = ROW_ALL_MASKED
        row = r["probs"][w::case.shape[1], :, m]
        assert bool((row > 2.0 ** -30).all()), "a row whose keys are all at -100 has ordinary probabilities"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_planes_against_the_unfused_chain(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    U = _ulps(r)[2]
    flips = fa._count_flips(eng, r["m2"], r["planes"], r["p_ref"], U, case.name)
    print(f"[fused wattn] {case.name}: {flips} plane bytes differ from the unfused chain's (U = {U})")
    _MARGINS.setdefault("plane_bytes_differing_from_unfused", {})[case.name] = flips
    with torch.no_grad():
        rel = ((r["out"] - r["out_ref"]).norm() / r["out_ref"].norm()).item()
    _MARGINS.setdefault("out_rel_diff_vs_unfused", {})[case.name] = rel
    if flips == 0:
        assert torch.equal(r["out"], r["out_ref"])


def _check_stages(r, what, skip_heads=()):
    """The three stage checks on one call's probs, planes and out; returns the ratios"""
    m2 = r["m2"]
    B_, H, M, N = r["probs"].shape
    s1, below = fw.check_window_probs(r["probs"], r["stage"], what)
    want, nan, grid = fr.attn_planes_of(r["probs"], H, **fa._pv_kw(m2))
    n = fr.check_planes(r["planes"], want, nan, grid, what)
    ref = fr.attn_consumer_stage(r["planes"], r["v"], H, sos=m2._sos, A_bit=m2.A_bit, B_bit=m2.B_bit, B_iv=m2.B_interval,
                                 A_iv=m2.A_interval, M=M, N=N)
    skip = np.zeros((1, H, 1, 1), bool)
    skip[0, list(skip_heads)] = True
    s3 = fr.check_out(r["out"], ref, N, what, skip=skip)
    return dict(probs_over_bound=s1, share_below_floor=below, plane_bytes_compared=n, out_over_bar=s3)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stages_against_the_float64_references(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    got = _check_stages(r, case.name)
    print(f"[fused wattn] {case.name}: |probs - p64| / bound {got['probs_over_bound']:.3f}; below 2^-100: {got['share_below_floor']:.4f}; "
          f"{got['plane_bytes_compared']} plane bytes exact; |out - ref| / bar {got['out_over_bar']:.3f}")
    _MARGINS.setdefault("stage_ratios", {})[case.name] = got
    assert got["plane_bytes_compared"] == r["probs"].numel() * len(r["planes"])
    masked = r["stage"]["masked"]
    share = float(np.broadcast_to(masked & (~masked).any(-1, keepdims=True), r["stage"]["p64"].shape).mean())
    assert got["share_below_floor"] <= share and (case.mask is None) == (share == 0.0)
    if case.mask == "shift" and case.bstd < 1.0:
        assert got["share_below_floor"] == share, "every masked key of a row with an unmasked key falls below 2^-100"


@pytest.mark.parametrize("twin", [True, False], ids=["sos", "plain"])
def test_a_zero_q_head_poisons_that_head_alone(eng, monkeypatch, twin):
    case = Case("w7_sos_mask" if twin else "w7_plain_mask", W7, twin, 8, "shift")
    H = case.shape[2]
    others = [h for h in range(H) if h != 1]
    bad = _run(eng, monkeypatch, case, ("zero_q", twin), seed=2690, zero_q_head=1)
    good = _run(eng, monkeypatch, case, ("healthy", twin), seed=2690)
    iv = bad["m1"].A_interval.reshape(-1)
    assert float(iv[1]) == 0.0 and bool((iv[others] > 0).all()), "the min-max interval of the zero head, and of it alone, is 0"
    what = f"zero q head, {'sos' if twin else 'plain'}"
    assert torch.isnan(bad["probs"][:, 1]).all(), "0 / 0 poisons every probability of the head"
    got = _check_stages(bad, what, skip_heads=(1,))
    _MARGINS.setdefault("degenerate", {})[what] = got
    assert torch.isfinite(bad["probs"][:, others]).all() and torch.isfinite(bad["out"][:, others]).all()
    assert fa._same_bits(bad["probs"][:, others], good["probs"][:, others])
    # (plain: matmul2's head-wise A interval comes from each run's own probabilities -- the other heads' are the same in both)
    assert fa._same_bits(bad["out"][:, others], good["out"][:, others])
    B_ = bad["probs"].shape[0]
    for a, b in zip(bad["planes"], good["planes"]):
        a, b = a.view(B_, H, *a.shape[1:]), b.view(B_, H, *b.shape[1:])
        assert torch.equal(a[:, others], b[:, others])


def test_a_row_of_nothing_but_neg_inf_is_nan_as_in_torch(eng):
    """max = -inf, -inf - -inf = NaN: that row of every head of that window is NaN in torch and in the kernel, nothing else is"""
    from ptq4vit_amd.utils.fuse import _matmul_side
    case = Case("mask_neg_inf", (1, 2, 2, 49, 32), True, 8, "inf")
    q, kT, v, bias, mask = _inputs(case, seed=2695)
    mask[1, 7, :] = -float("inf")
    m1, m2 = fa._modules(_fa_case(case), q, kT, v)
    with torch.no_grad():
        p_ref = _unfused_scores(m1, q, kT, bias, mask).softmax(dim=-1)
        out, probs = eng.window_attn_quant_forward(q=q, kT=kT, v=v, bias=bias, mask=mask, qk=_matmul_side(m1, 2), pv=_matmul_side(m2, 2),
                                                   want_probs=True)
    want = torch.zeros_like(probs, dtype=torch.bool)
    want[1, :, 7, :] = True
    assert torch.equal(torch.isnan(p_ref), want) and torch.equal(torch.isnan(probs), want)
    st = fw.window_float_stage(q, kT, m1.A_interval, m1.B_interval, m1.A_bit, m1.B_bit, bias, mask)
    worst, _ = fw.check_window_probs(probs, st, "one row of -inf")
    _MARGINS["row_of_neg_inf_probs_over_bound"] = worst
    keep = torch.ones(49, dtype=torch.bool, device="cuda")
    keep[7] = False                                  # (the NaN row's plane bytes are undefined: its `out` is not looked at)
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[1][:, keep]).all()


# ---- 6: the contract ---------------------------------------------------------------------------------------------------------------
def test_workspace_contract_and_envelope(eng, monkeypatch):
    r = run_case(eng, monkeypatch, CASES[0])          # (the exact, guarded, poisoned call)
    q, kT, v, bias, mask, (qk, pv) = r["q"], r["kT"], r["v"], r["bias"], r["mask"], r["sides"]
    kw = dict(q=q, kT=kT, v=v, bias=bias, qk=qk, pv=pv)
    torch.cuda.synchronize()
    with torch.no_grad():
        # the size asked for is the plain attention call's
        with Guard(eng, monkeypatch, 0x3C) as g:
            eng.attn_quant_forward(q=q, kT=kT, v=v, scale=1.0, qk=qk, pv=pv)
            assert g.finish()[0]["need"] == r["need"]
        # one byte less: refused, nothing launched
        before = eng.launch_counters()
        with Guard(eng, monkeypatch, 0xCD, declare=lambda n: n - 1) as g:
            with pytest.raises(RuntimeError, match="workspace too small"):
                eng.window_attn_quant_forward(mask=mask, **kw)
            reps = g.finish()
        assert eng.launch_counters() == before
        assert all(rep["touched"] == 0 and rep["guard_changed"] == 0 for rep in reps), reps
        # outside the envelope: refused before any launch
        with pytest.raises(RuntimeError, match="is no multiple of n_windows = 3"):
            eng.window_attn_quant_forward(mask=mask[:3], **kw)                        # 8 windows, a mask for 3
        with pytest.raises(ValueError, match="mask"):
            eng.window_attn_quant_forward(mask=mask[:, :-1], **kw)
        with pytest.raises(ValueError, match="bias"):
            eng.window_attn_quant_forward(mask=mask, **dict(kw, bias=bias[:-1]))
        for which in ("qk", "pv"):
            with pytest.raises(NotImplementedError, match="sub-blocks"):
                eng.window_attn_quant_forward(mask=mask, **dict(kw, **{which: dict(kw[which], blocks=(1, 1, 2, 2))}))
        with pytest.raises(NotImplementedError, match="split-of-softmax"):
            eng.window_attn_quant_forward(mask=mask, **dict(kw, qk=dict(qk, sos=True, split=pv["split"], A_interval=pv["A_interval"])))
        with pytest.raises(RuntimeError, match="is not the row operand"):
            eng.window_attn_quant_forward(mask=mask, **dict(kw, v=v[:, :, :-1]))
        assert eng.launch_counters() == before
        # no probabilities asked for: the same out; no mask: the no-mask case's out
        assert torch.equal(eng.window_attn_quant_forward(mask=mask, **kw), r["out"])
        assert eng.launch_counters()["asked"] > before["asked"]
        nomask = run_case(eng, monkeypatch, CASES[IDS.index("w7_sos_nomask")])
        assert not torch.equal(nomask["out"], r["out"])
        zero = eng.window_attn_quant_forward(mask=torch.zeros_like(mask), **kw)      # + 0.0: the same bits as no mask at all
        assert torch.equal(zero, eng.window_attn_quant_forward(mask=None, **kw))


# ---- module level: the tiny Swin -----------------------------------------------------------------------------------------------------
SWIN_KW = dict(img_size=56, embed_dim=24, depths=(2, 2), num_heads=(2, 4))


@pytest.fixture(scope="module")
def tiny():
    from ptq4vit_amd.configs import PTQ4ViT
    from ptq4vit_amd.utils import models, net_wrap
    from ptq4vit_amd.utils.quant_calib import HessianQuantCalibrator
    net = models.get_net("swin_tiny_patch4_window7_224", seed=0, device="cuda", **SWIN_KW)
    wrapped = net_wrap.wrap_modules_in_net(net, PTQ4ViT)
    images = torch.randn(4, 3, 56, 56, generator=torch.Generator().manual_seed(26)).cuda()
    HessianQuantCalibrator(net, wrapped, _Loader(images), sequential=False, batch_size=4).batching_quant_calib()
    return net, wrapped, images


def _window_names(net):
    from ptq4vit_amd.utils import models
    return [n for n, m in net.named_modules() if isinstance(m, models.WindowAttention)]


def _bias_of(att):
    n = att.window_size[0] * att.window_size[1]
    return att.relative_position_bias_table[att.relative_position_index.view(-1)].view(n, n, -1).permute(2, 0, 1).contiguous()


def _own_tensor_flips(eng, net, images):
    """The differing plane bytes of 4, counted on the UNFUSED net's own window tensors: (flips, probability bytes)"""
    from ptq4vit_amd.utils import fuse
    mods = dict(net.named_modules())
    seen, hooks = {}, []
    for n in _window_names(net):
        hooks.append(mods[n].register_forward_pre_hook(
            lambda mod, args, kwargs, key=n: seen.__setitem__((key, "mask"), kwargs.get("mask", args[1] if len(args) > 1 else None)), with_kwargs=True))
        for mm in ("matmul1", "matmul2"):
            hooks.append(getattr(mods[n], mm).register_forward_hook(
                lambda mod, inp, out, key=(n, mm): seen.__setitem__(key, tuple(t.detach() for t in inp))))
    try:
        with torch.no_grad():
            net(images)
    finally:
        for h in hooks:
            h.remove()
    flips = total = masks = 0
    for n in _window_names(net):
        att = mods[n]
        (q, kT), (p_ref, v), mask = seen[(n, "matmul1")], seen[(n, "matmul2")], seen[(n, "mask")]
        masks += mask is not None
        H = q.shape[1]
        with torch.no_grad():
            _, probs, planes = eng.window_attn_quant_forward(q=q, kT=kT, v=v, bias=_bias_of(att), mask=mask, qk=fuse._matmul_side(att.matmul1, H),
                                                             pv=fuse._matmul_side(att.matmul2, H), want_probs=True, want_planes=True)
        live = p_ref >= 2.0 ** -100
        U = int(ulp_distance(probs, p_ref)[live].max())
        flips += fa._count_flips(eng, att.matmul2, planes, p_ref, U, n)
        total += p_ref.numel() * len(planes)
    assert masks == 1, "one shifted block in the tiny Swin"
    return flips, total


def test_fused_net_logits_and_fallbacks(eng, tiny, monkeypatch):
    from ptq4vit_amd.utils import fuse, models
    net, wrapped, images = tiny
    watts = _window_names(net)
    assert len(watts) == 4
    flips, total = _own_tensor_flips(eng, net, images)
    calls = _count_fused_calls(eng, monkeypatch, "window_attn_quant_forward")
    plain_calls = _count_fused_calls(eng, monkeypatch, "attn_quant_forward")
    cls_forward = models.WindowAttention.forward
    mods = dict(net.named_modules())
    try:
        with torch.no_grad():
            y_u = net(images)
            assert not calls
            assert fuse.fuse_attention(net) == []
            assert fuse.fuse_window_attention(net) == watts and fuse.fuse_window_attention(net) == watts
            x0 = torch.empty(8, 49, mods[watts[0]].qkv.in_features, device="cuda")
            assert fuse.takes_fused_window_attention_path(mods[watts[0]], x0)
            assert fuse.takes_fused_window_attention_path(mods[watts[0]], x0, torch.zeros(4, 49, 49, device="cuda"))
            assert not fuse.takes_fused_window_attention_path(mods[watts[0]], x0, torch.zeros(3, 49, 49, device="cuda"))      # 8 % 3
            assert not fuse.takes_fused_window_attention_path(mods[watts[0]], x0, torch.zeros(4, 49, 49, device="cuda").double())
            assert not fuse.takes_fused_window_attention_path(mods[watts[0]], x0, torch.zeros(4, 49, 48, device="cuda"))
            y_f = net(images)
            assert len(calls) == len(watts) == 4 and not plain_calls, "the fused path did not run"
            for m in wrapped.values():
                m.mode = "raw"
            del calls[:]
            y_raw = net(images)
            assert not calls, "raw mode must take the original forward"
            fuse.unfuse_window_attention(net)
            assert torch.equal(net(images), y_raw)
            fuse.fuse_window_attention(net)
            for m in wrapped.values():
                m.mode = "quant_forward"
            ratio = fa._held_to_the_flips(y_f, y_u, y_raw, flips, total)
            print(f"[fused wattn] tiny Swin: {flips} of {total} plane bytes differ; |fused - unfused| / |unfused - raw| = {ratio:.3e}")
            _MARGINS["tiny_swin"] = dict(plane_bytes_differing=flips, plane_bytes=total, fused_over_quant_error=ratio)

            # all three fusions, in two orders
            assert len(fuse.fuse_mlp(net)) == 4 and fuse.fuse_attention(net) == []
            y_a = net(images)
            fuse.unfuse_window_attention(net)
            fuse.unfuse_mlp(net)
            fuse.unfuse_attention(net)
            fuse.fuse_attention(net)
            fuse.fuse_mlp(net)
            fuse.fuse_window_attention(net)
            del calls[:]
            y_b = net(images)
            assert len(calls) == 4 and torch.equal(y_a, y_b)
            fuse.unfuse_mlp(net)
            assert torch.equal(net(images), y_f)

            att = mods[watts[1]]                           # the shifted block: it is called with a mask
            probe = torch.randn(8, 49, att.qkv.in_features, device="cuda")
            pmask = torch.from_numpy(fw.shift_mask(4, 49, np.random.default_rng(5))).cuda()

            def unfused_twin(fn):
                """fn() on the fused net, then on the same net unfused, in whatever state it is in"""
                a = fn()
                fuse.unfuse_window_attention(net)
                b = fn()
                fuse.fuse_window_attention(net)
                return a, b

            # a forward hook on matmul1: it fires, that block takes the original forward, the output is the unfused net's
            fired = []
            h = att.matmul1.register_forward_hook(lambda mod, inp, out: fired.append(tuple(out.shape)))
            del calls[:]
            y_a, y_b = unfused_twin(lambda: net(images))
            assert len(fired) == 2 and len(calls) == 3
            assert torch.equal(y_a, y_b)
            h.remove()
            # a mask the fused path does not take (float64): the original forward
            del calls[:]
            m_a, m_b = unfused_twin(lambda: att(probe, mask=pmask.double()))
            assert not calls and torch.equal(m_a, m_b)
            m_a = att(probe, pmask)                        # (positional, float32: fused)
            assert len(calls) == 1
            # autograd recording: the original forward
            del calls[:]
            with torch.enable_grad():
                m_a, m_b = unfused_twin(lambda: att(probe.clone().requires_grad_(True), mask=pmask))
            assert not calls and torch.equal(m_a, m_b) and m_a.requires_grad
            # CPU tensors: the original forward
            att_cpu = copy.deepcopy(att).cpu()
            for m in att_cpu.modules():                    # (the intervals are plain attributes: .cpu() does not move them)
                for a in ("w_interval", "a_interval", "A_interval", "B_interval", "split"):
                    if torch.is_tensor(getattr(m, a, None)):
                        setattr(m, a, getattr(m, a).cpu())
            holder = torch.nn.Sequential(att_cpu)
            assert fuse.fuse_window_attention(holder) == ["0"]
            m_a = att_cpu(probe.cpu(), mask=pmask.cpu())
            assert fuse.unfuse_window_attention(holder) == ["0"]
            assert not calls and torch.equal(m_a, att_cpu(probe.cpu(), mask=pmask.cpu()))
            # everything back: fused again, and deterministic
            del calls[:]
            assert torch.equal(net(images), y_f) and len(calls) == 4
    finally:
        fuse.unfuse_window_attention(net)
        fuse.unfuse_mlp(net)
        fuse.unfuse_attention(net)
    # unfuse_window_attention restores the original forward
    for n in watts:
        m = dict(net.named_modules())[n]
        assert "forward" not in m.__dict__ and m.forward.__func__ is cls_forward
    assert fuse.unfuse_window_attention(net) == []
    with torch.no_grad():
        del calls[:]
        assert torch.equal(net(images), y_u) and not calls


def test_second_calibration_of_a_fused_net_gives_the_unfused_intervals(eng, tiny, monkeypatch):
    from ptq4vit_amd.utils import fuse
    from ptq4vit_amd.utils.quant_calib import HessianQuantCalibrator
    net, wrapped, images = tiny
    fuse.unfuse_window_attention(net)
    net_u = copy.deepcopy(net)
    wrapped_u = _wrapped_of(net_u, wrapped)
    net_f = copy.deepcopy(net)
    wrapped_f = _wrapped_of(net_f, wrapped)
    assert len(fuse.fuse_window_attention(net_f)) == 4
    HessianQuantCalibrator(net_u, wrapped_u, _Loader(images), sequential=False, batch_size=4).batching_quant_calib()
    HessianQuantCalibrator(net_f, wrapped_f, _Loader(images), sequential=False, batch_size=4).batching_quant_calib()
    iu, ifu = _intervals(wrapped_u), _intervals(wrapped_f)
    assert iu.keys() == ifu.keys() and len(iu) >= len(wrapped)
    for k in iu:
        assert torch.equal(iu[k], ifu[k]), k
    # ... and the fused net is still fused, and runs fused
    calls = _count_fused_calls(eng, monkeypatch, "window_attn_quant_forward")
    with torch.no_grad():
        net_f(images)
    assert len(calls) == 4
