"""GPU: the fused int8 qkv + attention forward (p4v_qkv_attn_quant_forward, engine.qkv_attn_quant_forward,
utils/fuse.py::fuse_qkv_attention).

k_qkv_heads computes the qkv layer's int8 GEMM and quantises every output element scale * acc + bias with the quantiser of the
MatMul operand it belongs to, straight into matmul1's two operand planes and matmul2's column plane; the rest of the chain is
p4v_attn_quant_forward's on those planes.  There is no transcendental between the GEMM and the quantisers: everything here is held
byte for byte / bit for bit, per case, on a poisoned workspace of exactly the size asked for.

1. qkv_out (the optional fp32 copy of what the planes were quantised from) equals engine.linear_quant_forward of the same layer
   bit for bit, and -- except for the zero block -- lies within the Linear stage bound of tests/fused_reference.py: the float64
   product of the oracle's quantisers on the raw x and W, |qkv_out - v64| <= 2^-24 (2 |o64| + |v64|) + 2^-126 (the scale product
   and acc * S1: 2^-24 |o| each; the bias addition: 2^-24 |v| -- the bound fc1's pre-GELU value is held to there);
2. the Q, K^T and V planes equal, byte for byte and padding included, what the library's single-plane packer makes of the call's
   own qkv_out, sliced and permuted as Attention.forward does, and the oracle's quant_int of the same slices on the CPU;
3. probs, P1 / P2 and out are bit-identical to engine.attn_quant_forward(q, kT, v, ...) on the slices of the call's own qkv_out,
   as contiguous copies (P4V_QKV_CONTIGUOUS = 1) and as strided views (0);
4. zero_v_block: the v third of Wqkv is zero, its min-max weight interval 0, its columns of qkv_out NaN (the scale table carries
   the reference's 0 / 0), matmul2's min-max B interval NaN: out is NaN, the q and k planes and probs are bit-identical to `base`
   on the same x, the V plane's bytes lie on the grid;
5. the contract: exact workspace under two poisons, one byte less refused with no launch, the envelope refused with no launch;
6. module level on the mini ViT: fuse_qkv_attention's logits are fuse_attention's bit for bit, with fuse_mlp in either order; one
   call per block; hooked / uncalibrated / calibration-mode / CPU / autograd states fall back and reproduce the unfused logits; a
   second calibration of the fused net gives bit-identical intervals; unfuse_attention restores.

Shapes: see CASES -- each the smallest that reaches one way the scatter can go wrong.  With P4V_FUSED_QKV_OUT set the measured
margins are written there, under "qkv" (profiles/r29_fused_qkv_margins.json).
"""
import copy
import json
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import fused_reference as fr
from tests.fused_common import _Loader, _count_fused_calls, _intervals, _wrapped_of, merge_margins
from tests.workspace_guard import Guard

pytestmark = pytest.mark.gpu

SPLIT = 2.0 ** -5
FACTORS = {"q": (1.0, 0.8, 1.25), "k": (0.9, 1.15, 1.0), "v": (1.2, 1.0, 0.85), "p": (1.1, 0.9, 1.0), "w": (1.05, 0.95, 1.1)}
_MARGINS = {}

Case = namedtuple("Case", "name B N H D K sos bias n_V w_bit a_bit qk_bits pv_bits zero_v",
                  defaults=(True, True, 3, 8, 8, (8, 8), (8, 8), False))
#               id             B  Ntok  H  D    in_features
CASES = [Case("base",          2, 50,   3, 64,  192),     # one row tile crossing an image boundary
         Case("n197",          3, 197,  3, 64,  192),     # several row tiles, boundaries mid-tile, b64 v plane, Kp = 256
         Case("d40",           2, 50,   3, 40,  120),     # K1p padding, column tiles straddling heads and the q / k / v boundaries
         Case("d128",          2, 50,   2, 128, 64),      # a head fills a column tile; two k-tiles in k_attn_qk
         Case("d80",           1, 130,  2, 80,  48),      # in_features padded to 64, an unpadded row tile + 2 rows
         Case("n5",            1, 5,    1, 64,  64),      # matmul2 with one k-tile (not b64)
         Case("n1025",         1, 1025, 1, 64,  64),      # ktiles = 17: the other column-plane geometry
         Case("plain",         2, 50,   3, 64,  192, sos=False),
         Case("nobias_nv1",    2, 50,   3, 64,  192, bias=False, n_V=1),
         Case("mixbit",        2, 50,   3, 64,  192, w_bit=4, a_bit=8, qk_bits=(8, 4), pv_bits=(4, 8)),
         Case("zero_v_block",  2, 50,   3, 64,  192, zero_v=True)]
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    yield engine
    engine.release_workspace()
    merge_margins(os.environ.get("P4V_FUSED_QKV_OUT"), "qkv", _MARGINS, IDS)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same_with_nan(a, b):
    """equal where either is a number, NaN where the other is"""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _minmax(t, dims, qmax, factors):
    """the min-max rule per head / block, absmax / (q - 0.5), times a different factor each (a wrong index shows); 0 and NaN stay"""
    return t.abs().amax(dim=dims) / (qmax - 0.5) * torch.tensor(factors[:t.shape[1]], device=t.device)


def _slices(qkv_out, H, contiguous=True):
    """q, kT, v of a qkv tensor [B][N][3 * H * D] as Attention.forward takes them"""
    B, N, C3 = qkv_out.shape
    t = qkv_out.reshape(B, N, 3, H, C3 // (3 * H)).permute(2, 0, 3, 1, 4)
    if contiguous:
        t = t.contiguous()
    q, k, v = t.unbind(0)
    return q, k.transpose(-2, -1), v


def _inputs(case):
    # (zero_v_block: base's x, W and bias, the v third of W zeroed)
    g = torch.Generator().manual_seed(2900 + IDS.index("base" if case.zero_v else case.name))
    C3 = 3 * case.H * case.D
    x = torch.randn(case.B, case.N, case.K, generator=g)
    W = torch.randn(C3, case.K, generator=g) * case.K ** -0.5
    b = torch.randn(C3, generator=g) * 0.2 if case.bias else None
    if case.zero_v:
        W[2 * C3 // 3:] = 0.0
    return x.cuda(), W.cuda(), None if b is None else b.cuda()


_RUNS = {}


def run_case(eng, monkeypatch, case):
    """One fused call per case (exact, guarded, poisoned workspace) and the unfused qkv layer next to it; shared by the tests."""
    if case.name in _RUNS:
        return _RUNS[case.name]
    B, N, H, D = case.B, case.N, case.H, case.D
    x, W, bias = _inputs(case)
    wq, aq = 2 ** (case.w_bit - 1), 2 ** (case.a_bit - 1)
    with torch.no_grad():
        w_iv = _minmax(W.reshape(1, case.n_V, -1), (0, 2), wq, FACTORS["w"])
        a_iv = x.abs().amax().reshape(1) / (aq - 0.5)
        lin = dict(weight=W, bias=bias, w_interval=w_iv, a_interval=a_iv, w_bit=case.w_bit, a_bit=case.a_bit, n_V=case.n_V, n_H=1, n_a=1)
        ref = eng.linear_quant_forward(x=x, **lin)
        q, kT, v = _slices(ref, H)
        (qa, qb), (pa, pb) = case.qk_bits, case.pv_bits
        qk = dict(A_interval=_minmax(q, (0, 2, 3), 2 ** (qa - 1), FACTORS["q"]), B_interval=_minmax(kT, (0, 2, 3), 2 ** (qb - 1), FACTORS["k"]),
                  split=None, A_bit=qa, B_bit=qb, sos=False)
        pv = dict(B_interval=_minmax(v, (0, 2, 3), 2 ** (pb - 1), FACTORS["v"]), A_bit=pa, B_bit=pb, sos=case.sos)
        if case.sos:
            pv["split"] = torch.tensor(SPLIT, device="cuda")
            pv["A_interval"] = torch.tensor(float(np.float32(SPLIT) / np.float32(2 ** (pa - 1) - 1)), device="cuda")   # split / (q - 1)
        else:
            pv["split"] = None
            pv["A_interval"] = torch.tensor(FACTORS["p"][:H], device="cuda") / (2 ** (pa - 1) - 0.5)       # probabilities: absmax <= 1
        scale = D ** -0.5
        with Guard(eng, monkeypatch, 0xCD) as g:
            out, qkv_out, probs, planes = eng.qkv_attn_quant_forward(x=x, qkv=lin, scale=scale, qk=qk, pv=pv, want_qkv=True, want_probs=True,
                                                                     want_planes=True)
            reps = g.finish()
        assert len(reps) == 1 and reps[0]["guard_changed"] == 0 and 0 < reps[0]["touched"] <= reps[0]["need"], reps
    r = dict(x=x, lin=lin, qk=qk, pv=pv, scale=scale, ref=ref, out=out, qkv_out=qkv_out, probs=probs, planes=planes, need=reps[0]["need"])
    _RUNS[case.name] = r
    return r


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_qkv_out_is_linear_quant_forward_bit_for_bit(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    got, ref = r["qkv_out"], r["ref"]
    assert got.shape == ref.shape == (case.B, case.N, 3 * case.H * case.D)
    if case.zero_v:
        C2 = 2 * case.H * case.D
        assert torch.isnan(got[..., C2:]).all() and torch.isfinite(got[..., :C2]).all(), "the NaN block stays in its own columns"
        assert _same_with_nan(got, ref) and _same_bits(got[..., :C2], ref[..., :C2])
        return
    assert torch.isfinite(got).all()
    assert _same_bits(got, ref), f"{case.name}: {int((got != ref).sum())} elements differ from linear_quant_forward's"
    lin = r["lin"]
    o64, v64, _ = fr.mlp_float_stage(r["x"], lin["weight"], lin["bias"], lin["w_interval"], lin["a_interval"], case.w_bit, case.a_bit)
    bound = 2.0 ** -24 * (2.0 * np.abs(o64) + np.abs(v64)) + 2.0 ** -126
    ratio = float((np.abs(fr.as_np(got).reshape(v64.shape).astype(np.float64) - v64) / bound).max())
    print(f"[fused qkv] {case.name}: |qkv_out - v64| / bound {ratio:.3f}")
    _MARGINS.setdefault("qkv_out_over_linear_bound", {})[case.name] = ratio
    assert ratio <= 1.0, f"{case.name}: |qkv_out - v64| is {ratio:.3f} of 2^-24 (2 |o64| + |v64|)"


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def _operands(case, r):
    """(name, the operand as the plane lays it out [Z][rows][cols], its head-wise interval, its bit width) for Q, K^T, V"""
    q, kT, v = _slices(r["qkv_out"], case.H)
    Z = case.B * case.H
    return (("Q", q.reshape(Z, case.N, case.D), r["qk"]["A_interval"], case.qk_bits[0]),
            ("Kt", kT.transpose(-2, -1).reshape(Z, case.N, case.D), r["qk"]["B_interval"], case.qk_bits[1]),
            ("V", v.transpose(-2, -1).reshape(Z, case.D, case.N), r["pv"]["B_interval"], case.pv_bits[1]))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_planes_are_the_packers_and_the_oracles_bytes_of_the_calls_own_qkv(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    Z, H, N, D = case.B * case.H, case.H, case.N, case.D
    up = lambda n, m: (n + m - 1) // m * m
    Q, Kt, V = r["planes"][:3]
    assert Q.shape == (Z, up(N, 128), up(D, 64)) and Kt.shape == (Z, up(N, 128), up(D, 64))
    assert V.shape[0] == Z and V.shape[1] >= D and V.shape[2] == up(N, 64)
    assert len(r["planes"]) == (5 if case.sos else 4)
    compared = 0
    for (name, t, iv, bit), got in zip(_operands(case, r), (Q, Kt, V)):
        qm = 2 ** (bit - 1)
        rows, cols = t.shape[1:]
        # the library's single-plane packer (k_pack1), padded columns included: one scale per z
        scales = iv.reshape(-1)[torch.arange(Z, device="cuda") % H]
        _, ref = eng.pack_plane_i8(t.reshape(Z * rows, cols), mode="sym", scales=scales, rows_per_scale=rows, lo=-qm, hi=qm - 1)
        ref = ref.reshape(Z, rows, -1)
        assert ref.shape[2] == got.shape[2]
        nan = torch.isnan(t)
        if not case.zero_v:
            assert not nan.any()
        assert torch.equal(got[:, :rows], ref), f"{case.name} {name}: {int((got[:, :rows] != ref).sum())} bytes differ from the packer's"
        assert not got[:, rows:].any(), f"{case.name} {name}: padding rows must be zero"
        assert not got[:, :, cols:].any(), f"{case.name} {name}: padding columns must be zero"
        assert got.any()
        # the oracle's quant_int of the same slices on the CPU (NaN entries: on the grid)
        want, m = fr.int_plane(fr.as_np(t), fr.as_np(iv).reshape(-1)[np.arange(Z) % H].reshape(Z, 1, 1), -qm, qm - 1)
        compared += fr.check_planes([got], [want], m, [(-qm, qm - 1)], f"{case.name} {name}")
    _MARGINS.setdefault("plane_bytes_exact", {})[case.name] = compared
    assert compared == (3 if not case.zero_v else 2) * Z * N * D


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contiguous", ["1", "0"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_chain_is_attn_quant_forward_on_the_calls_own_slices(eng, monkeypatch, case, contiguous):
    r = run_case(eng, monkeypatch, case)
    monkeypatch.setenv("P4V_QKV_CONTIGUOUS", contiguous)
    q, kT, v = _slices(r["qkv_out"], case.H, contiguous=os.environ["P4V_QKV_CONTIGUOUS"] == "1")
    assert q.is_contiguous() == (contiguous == "1")
    with torch.no_grad():
        out, probs, planes = eng.attn_quant_forward(q=q, kT=kT, v=v, scale=r["scale"], qk=r["qk"], pv=r["pv"], want_probs=True, want_planes=True)
    assert len(planes) == len(r["planes"]) - 3 == (2 if case.sos else 1)
    for got, ref in zip(r["planes"][3:], planes):
        assert torch.equal(got, ref), f"{case.name}: {int((got != ref).sum())} bytes of matmul2's row plane differ"
    assert _same_bits(r["probs"], probs), f"{case.name}: probs differ"
    if case.zero_v:
        assert torch.isnan(out).all() and torch.isnan(r["out"]).all()
    else:
        assert torch.isfinite(r["out"]).all() and _same_bits(r["out"], out), f"{case.name}: out differs"
    assert r["out"].shape == (case.B, case.H, case.N, case.D)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def test_zero_v_block_poisons_v_alone(eng, monkeypatch):
    bad, good = run_case(eng, monkeypatch, CASES[IDS.index("zero_v_block")]), run_case(eng, monkeypatch, CASES[IDS.index("base")])
    assert torch.equal(bad["x"], good["x"])
    w_iv = bad["lin"]["w_interval"].reshape(-1)
    assert float(w_iv[2]) == 0.0 and bool((w_iv[:2] > 0).all()), "the min-max interval of the zero block, and of it alone, is 0"
    assert torch.isnan(bad["pv"]["B_interval"]).all(), "matmul2's min-max B interval of a NaN v"
    assert torch.isnan(bad["out"]).all(), "out is the reference's NaN"
    assert torch.isfinite(good["out"]).all()
    for i in (0, 1):
        assert torch.equal(bad["planes"][i], good["planes"][i])
    assert _same_bits(bad["probs"], good["probs"]) and torch.isfinite(bad["probs"]).all()
    for a, b in zip(bad["planes"][3:], good["planes"][3:]):
        assert torch.equal(a, b)
    V = bad["planes"][2]
    assert bool(((V >= -128) & (V <= 127)).all()) and not V[:, 64:].any() and not V[:, :, 50:].any()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def test_workspace_contract_and_envelope(eng, monkeypatch):
    case = CASES[0]
    r = run_case(eng, monkeypatch, case)              # (the exact, guarded call on 0xCD)
    x, lin, scale, qk, pv = r["x"], r["lin"], r["scale"], r["qk"], r["pv"]
    call = lambda **kw: eng.qkv_attn_quant_forward(**{**dict(x=x, qkv=lin, scale=scale, qk=qk, pv=pv), **kw})
    torch.cuda.synchronize()
    with torch.no_grad():
        # the other poison: 0xA5 -- the same result, every plane byte the consumers read defined by the call
        with Guard(eng, monkeypatch, 0xA5) as g:
            out, qkv_out, probs, planes = call(want_qkv=True, want_probs=True, want_planes=True)
            reps = g.finish()
        assert len(reps) == 1 and reps[0]["guard_changed"] == 0 and 0 < reps[0]["touched"] <= reps[0]["need"] == r["need"], reps
        assert _same_bits(out, r["out"]) and _same_bits(qkv_out, r["qkv_out"]) and _same_bits(probs, r["probs"])
        assert all(torch.equal(a, b) for a, b in zip(planes, r["planes"]))
        # one byte less: refused, nothing launched
        before = eng.launch_counters()
        with Guard(eng, monkeypatch, 0xCD, declare=lambda n: n - 1) as g:
            with pytest.raises(RuntimeError, match="workspace too small"):
                call()
            reps = g.finish()
        assert eng.launch_counters() == before
        assert all(rep["touched"] == 0 and rep["guard_changed"] == 0 for rep in reps), reps
        # outside the envelope: refused before any launch
        for bad in (dict(n_H=2), dict(n_a=2), dict(postgelu=True)):
            with pytest.raises(NotImplementedError, match="qkv"):
                call(qkv=dict(lin, **bad))
        wide = torch.cat([lin["weight"], lin["weight"][:3]])                   # out_features = 3 H D + 3
        with pytest.raises((ValueError, RuntimeError), match="3 x"):       # (the C ABI's own refusal: tests/test_fused_qkv_host.py)
            call(qkv=dict(lin, weight=wide, bias=None, n_V=1, w_interval=lin["w_interval"][:1]))
        for which in ("qk", "pv"):
            with pytest.raises(NotImplementedError, match="sub-blocks"):
                call(**{which: dict(r[which], blocks=(1, 1, 2, 2))})
        with pytest.raises(NotImplementedError, match="split-of-softmax"):
            call(qk=dict(qk, sos=True, split=pv["split"]))
        with pytest.raises(RuntimeError, match="scale is NaN"):
            call(scale=float("nan"))
        assert eng.launch_counters() == before
        # nothing optional asked for: the same out
        assert _same_bits(call(), r["out"])
        assert eng.launch_counters()["asked"] > before["asked"]


# ---- 6: module level, the mini ViT ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mini():
    from ptq4vit_amd.configs import PTQ4ViT
    from ptq4vit_amd.utils import models, net_wrap
    from ptq4vit_amd.utils.quant_calib import HessianQuantCalibrator
    g = np.load("tests/golden/minivit_ptq4vit.npz", allow_pickle=False)
    kw = json.loads(str(g["model_kwargs"]))
    net = models.get_net("vit_tiny_patch16_224", seed=0, device="cuda", **kw)
    wrapped = net_wrap.wrap_modules_in_net(net, PTQ4ViT)
    images = torch.from_numpy(g["images"][:4]).cuda()
    HessianQuantCalibrator(net, wrapped, _Loader(images), sequential=False, batch_size=4).batching_quant_calib()
    return net, wrapped, images


def _attention_names(net):
    from ptq4vit_amd.utils import models
    return [n for n, m in net.named_modules() if isinstance(m, models.Attention)]


def test_fused_net_logits_are_fuse_attentions_and_fallbacks(eng, mini, monkeypatch):
    from ptq4vit_amd.utils import fuse, models
    net, wrapped, images = mini
    attns = _attention_names(net)
    mods = dict(net.named_modules())
    assert len(attns) == 2
    new = _count_fused_calls(eng, monkeypatch, "qkv_attn_quant_forward")
    old = _count_fused_calls(eng, monkeypatch, "attn_quant_forward")
    cls_forward = models.Attention.forward
    reset = lambda: (new.__delitem__(slice(None)), old.__delitem__(slice(None)))
    try:
        with torch.no_grad():
            y_u = net(images)
            assert fuse.fuse_attention(net) == attns
            y_a = net(images)
            assert len(old) == len(attns) and not new, "a fuse_attention-only net makes no call of the new kernel"
            reset()
            assert fuse.fuse_qkv_attention(net) == attns and fuse.fuse_qkv_attention(net) == attns          # over fuse_attention's; idempotent
            assert all(fuse.takes_fused_qkv_attention_path(mods[n], torch.empty(4, 5, mods[n].qkv.in_features, device="cuda")) for n in attns)
            y_q = net(images)
            assert len(new) == len(attns) and not old, "one call of the new kernel per block"
            assert _same_bits(y_q, y_a), f"max |diff| {(y_q - y_a).abs().max().item():.3e}"
            # with fuse_mlp, in either order
            fuse.fuse_mlp(net)
            y_qm = net(images)
            fuse.unfuse_attention(net)
            fuse.fuse_attention(net)
            y_am = net(images)
            fuse.unfuse_attention(net)
            fuse.unfuse_mlp(net)
            fuse.fuse_qkv_attention(net)
            fuse.fuse_mlp(net)
            reset()
            y_mq = net(images)
            assert len(new) == len(attns) and not old
            assert _same_bits(y_qm, y_am) and _same_bits(y_mq, y_am)
            fuse.unfuse_mlp(net)
            assert _same_bits(net(images), y_q)

            att = mods[attns[0]]
            probe = torch.randn(4, 17, att.qkv.in_features, device="cuda")

            def unfused_twin(fn):
                """fn() on the fused net, then on the same net unfused, in whatever state it is in"""
                a = fn()
                fuse.unfuse_attention(net)
                b = fn()
                fuse.fuse_qkv_attention(net)
                return a, b

            # a forward hook on qkv: it fires, that block runs fuse_attention's path (qkv as a module), the logits are unchanged
            fired = []
            h = att.qkv.register_forward_hook(lambda mod, inp, out: fired.append(tuple(out.shape)))
            reset()
            assert not fuse.takes_fused_qkv_attention_path(att, probe) and fuse.takes_fused_attention_path(att, probe)
            y_h, y_b = unfused_twin(lambda: net(images))
            assert len(fired) == 2 and len(new) == len(attns) - 1 and len(old) == 1
            assert _same_bits(y_h, y_q) and _same_bits(y_b, y_u)
            h.remove()
            # a hook on matmul1: the original forward for that block
            h = att.matmul1.register_forward_hook(lambda mod, inp, out: None)
            reset()
            m_a, m_b = unfused_twin(lambda: att(probe))
            assert not new and not old and _same_bits(m_a, m_b)
            h.remove()
            # an uncalibrated qkv / calibration mode on qkv: fuse_attention's path; raw mode everywhere: the original forward
            for state in ("uncalibrated", "calibration", "raw"):
                saved = [(m, m.mode, m.calibrated) for m in wrapped.values()]
                if state == "uncalibrated":
                    att.qkv.calibrated = None
                    att.qkv.mode = "raw"
                elif state == "calibration":
                    att.qkv.mode = "calibration_step1"
                else:
                    for m in wrapped.values():
                        m.mode = "raw"
                reset()
                assert not fuse.takes_fused_qkv_attention_path(att, probe)
                y_s, y_b = unfused_twin(lambda: net(images))
                assert _same_bits(y_s, y_b), state
                assert len(new) == (0 if state == "raw" else len(attns) - 1), (state, len(new), len(old))
                for m, mode, cal in saved:
                    m.mode, m.calibrated = mode, cal
                if state == "calibration":
                    att.qkv.raw_input = att.qkv.raw_out = None
            # autograd recording: the original forward
            reset()
            with torch.enable_grad():
                m_a, m_b = unfused_twin(lambda: att(probe.clone().requires_grad_(True)))
            assert not new and not old and torch.equal(m_a, m_b)
            # CPU tensors: the original forward
            att_cpu = copy.deepcopy(att).cpu()
            for m in att_cpu.modules():                    # (the intervals are plain attributes: .cpu() does not move them)
                for a in ("w_interval", "a_interval", "A_interval", "B_interval", "split"):
                    if torch.is_tensor(getattr(m, a, None)):
                        setattr(m, a, getattr(m, a).cpu())
            holder = torch.nn.Sequential(att_cpu)
            assert fuse.fuse_qkv_attention(holder) == ["0"]
            m_a = att_cpu(probe.cpu())
            assert fuse.unfuse_attention(holder) == ["0"]
            assert not new and not old and torch.equal(m_a, att_cpu(probe.cpu()))
            # everything back: fused again, and deterministic
            reset()
            assert _same_bits(net(images), y_q) and len(new) == len(attns) and not old
    finally:
        fuse.unfuse_attention(net)
        fuse.unfuse_mlp(net)
    # unfuse_attention restores the class forward after either fuse call, in either order
    for first, second in ((fuse.fuse_attention, fuse.fuse_qkv_attention), (fuse.fuse_qkv_attention, fuse.fuse_attention)):
        assert first(net) == attns and second(net) == attns
        assert fuse.unfuse_attention(net) == attns and fuse.unfuse_attention(net) == []
        for n in attns:
            assert "forward" not in mods[n].__dict__ and mods[n].forward.__func__ is cls_forward
    with torch.no_grad():
        reset()
        assert _same_bits(net(images), y_u) and not new and not old


def test_second_calibration_of_a_fused_net_gives_the_unfused_intervals(eng, mini, monkeypatch):
    from ptq4vit_amd.utils import fuse
    from ptq4vit_amd.utils.quant_calib import HessianQuantCalibrator
    net, wrapped, images = mini
    fuse.unfuse_attention(net)
    net_u = copy.deepcopy(net)
    wrapped_u = _wrapped_of(net_u, wrapped)
    net_f = copy.deepcopy(net)
    wrapped_f = _wrapped_of(net_f, wrapped)
    assert len(fuse.fuse_qkv_attention(net_f)) == 2
    HessianQuantCalibrator(net_u, wrapped_u, _Loader(images), sequential=False, batch_size=4).batching_quant_calib()
    HessianQuantCalibrator(net_f, wrapped_f, _Loader(images), sequential=False, batch_size=4).batching_quant_calib()
    iu, ifu = _intervals(wrapped_u), _intervals(wrapped_f)
    assert iu.keys() == ifu.keys() and len(iu) >= len(wrapped)
    for k in iu:
        assert torch.equal(iu[k], ifu[k]), k
    # ... and the fused net is still fused, and runs fused
    calls = _count_fused_calls(eng, monkeypatch, "qkv_attn_quant_forward")
    with torch.no_grad():
        net_f(images)
    assert len(calls) == 2
