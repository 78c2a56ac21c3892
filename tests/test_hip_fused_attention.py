"""GPU: the fused int8 attention forward (p4v_attn_quant_forward, engine.attn_quant_forward, utils/fuse.py::fuse_attention).

k_attn_qk computes matmul1's int8 GEMM, `* scale`, the softmax over the keys and matmul2's A quantiser and writes matmul2's int8
row plane(s); matmul2 is the unfused forward sweep on those planes.  What is held here, per case, on a poisoned workspace of
exactly the size asked for:

1. quantiser and layout: the planes the call left are, byte for byte, padding included and per z, what k_pack_dual (split of
   softmax) / the single-plane packer (plain head-wise A interval) makes of the call's OWN fp32 probabilities; padding rows and
   columns are zero;
2. matmul2 from planes: `out` is matmul2.quant_forward(probs, v), bit for bit;
3. softmax: probs and torch's softmax(matmul1.quant_forward(q, kT) * scale, -1), both in fp32 ulps against the float64 softmax of
   the same fp32 scores (CPU, rounded to fp32): U_k <= max(2 U_t, 8).  Both sides call ROCm's expf on identical arguments; the
   freedom is the order of the row sum and the final division.  8 ulp: OpenCL's 3-ulp bound on exp for the numerator, the same
   for the denominator's terms, the division and the final rounding, rounded up;
4. against the unfused chain: a plane byte may differ from the unfused k_pack_dual byte by one grid step only, and only where the
   unfused pre-rounding value t lies within (U + 1) * 2^-23 * max(|t|, 1) of a half-integer (U: kernel-to-torch ulps of 3);
5. the contract: exact workspace, one byte less refused with no launch, sub-blocks / a split-of-softmax q k^T / mismatched
   qk.N, pv.K refused with no launch, null probs;
6. module level on the mini ViT: fuse_attention's names, logits fused vs unfused, fuse_mlp + fuse_attention in both orders,
   raw / hooked / CPU / autograd states fall back bit-identically, a second calibration of the fused net gives the unfused net's
   intervals, unfuse_attention restores, P4V_QKV_CONTIGUOUS 0 and 1.

Shapes (the smallest that reach every edge): 197 queries and keys (a full 128-row tile and a ragged one, six full 32-key tiles
and a ragged one, Kp = 256), head_dim 64 and 40 (ragged k-tile), 50 keys (less than one 64-byte piece row), 577 keys (ViT-B/384).

With P4V_FUSED_ATTN_OUT set the measured margins are written there (profiles/r22_fused_attn_margins.json).
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests.fused_common import _Loader, _count_fused_calls, _intervals, _wrapped_of, ulp_distance
from tests.workspace_guard import Guard

pytestmark = pytest.mark.gpu

SPLIT = 2.0 ** -5                 # of the reference's grid 2^-i, i < 20 (matmul.py:636)
HEAD_FACTORS = {"qA": (1.0, 0.8, 1.25), "qB": (0.9, 1.15, 1.0), "pA": (1.1, 0.9, 1.0), "pB": (1.2, 1.0, 0.85)}
ULP_FLOOR = 8
_MARGINS = {}

#          id             (batch, H, N, D)    twin   pv bits  qk (A, B) bits  q factor  strided
CASES = [("sos_w8a8",    (2, 3, 197, 64),    True,  8,       (8, 8),         1.0,      False),
         ("sos_w6a6",    (2, 3, 197, 64),    True,  6,       (6, 6),         1.0,      False),
         ("plain_w8a8",  (2, 3, 197, 64),    False, 8,       (8, 8),         1.0,      False),
         ("sos_qk_a8b4", (2, 3, 197, 64),    True,  8,       (8, 4),         1.0,      False),
         ("sos_d40",     (2, 3, 197, 40),    True,  8,       (8, 8),         1.0,      False),
         ("sos_n50",     (2, 3, 50, 64),     True,  8,       (8, 8),         1.0,      False),
         ("sos_n577",    (1, 2, 577, 64),    True,  8,       (8, 8),         1.0,      False),
         ("sos_wide",    (2, 3, 197, 64),    True,  8,       (8, 8),         8.0,      False),
         ("sos_strided", (2, 3, 197, 64),    True,  8,       (8, 8),         1.0,      True)]
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    yield engine
    engine.release_workspace()
    path = os.environ.get("P4V_FUSED_ATTN_OUT")
    if _MARGINS and path:
        path = os.path.abspath(path)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        old = {}
        if os.path.exists(path):
            with open(path) as fh:
                old = json.load(fh)
        old.update(_MARGINS)
        with open(path, "w") as fh:
            json.dump(old, fh, indent=1, sort_keys=True)
            fh.write("\n")


def _inputs(case):
    """q, kT, v as Attention.forward hands them over: views of the qkv Linear's output [B][N][3][H][D]."""
    name, (B, H, N, D), _, _, _, qf, strided = case
    g = torch.Generator().manual_seed(2200 + IDS.index(name))
    qkv = torch.randn(B, N, 3, H, D, generator=g)
    qkv[:, :, 0] *= qf
    qkv = qkv.cuda().permute(2, 0, 3, 1, 4)
    if not strided:
        qkv = qkv.contiguous()
    q, k, v = qkv.unbind(0)
    if strided:
        assert not q.is_contiguous() and not v.is_contiguous()
    return q, k.transpose(-2, -1), v


def _headwise(x, dims, qmax, factors):
    """absmax / (q - 0.5) per head, times a different factor per head (a wrong head index shows)"""
    H = x.shape[1]
    f = torch.tensor(factors[:H], device=x.device)
    return (x.abs().amax(dim=dims) / (qmax - 0.5) * f).view(1, H, 1, 1, 1, 1, 1)


def _modules(case, q, kT, v):
    from ptq4vit_amd.quant_layers.matmul import PTQSLBatchingQuantMatMul, SoSPTQSLBatchingQuantMatMul
    _, _, twin, pv_bits, (qa, qb), _, _ = case
    m1 = PTQSLBatchingQuantMatMul(A_bit=qa, B_bit=qb, mode="quant_forward")
    m1.A_interval = _headwise(q, (0, 2, 3), m1.A_qmax, HEAD_FACTORS["qA"])
    m1.B_interval = _headwise(kT, (0, 2, 3), m1.B_qmax, HEAD_FACTORS["qB"])
    m1.calibrated = True
    if twin:
        m2 = SoSPTQSLBatchingQuantMatMul(A_bit=pv_bits, B_bit=pv_bits, mode="quant_forward", split=torch.tensor(SPLIT, device="cuda"))
        assert float(m2.A_interval) == float(np.float32(SPLIT) / np.float32(m2.A_qmax - 1))       # A_interval = split / (q - 1)
    else:
        m2 = PTQSLBatchingQuantMatMul(A_bit=pv_bits, B_bit=pv_bits, mode="quant_forward")
    m2.B_interval = _headwise(v, (0, 2, 3), m2.B_qmax, HEAD_FACTORS["pB"])
    m2.calibrated = True
    return m1, m2


_RUNS = {}


def run_case(eng, monkeypatch, case):
    """One fused call per case (exact, guarded, poisoned workspace) and the unfused chain next to it; shared by the tests."""
    name, (B, H, N, D), twin = case[0], case[1], case[2]
    if name in _RUNS:
        return _RUNS[name]
    from ptq4vit_amd.utils.fuse import _matmul_side
    q, kT, v = _inputs(case)
    scale = D ** -0.5
    m1, m2 = _modules(case, q, kT, v)
    with torch.no_grad():
        # the unfused chain
        u_ref = m1.quant_forward(q, kT) * scale
        gap = float((u_ref.amax(-1, keepdim=True) - u_ref).max())
        assert gap < 80.0, f"{name}: max - u = {gap}: a probability would be subnormal"
        p_ref = u_ref.softmax(dim=-1)
        if not twin:
            m2.A_interval = _headwise(p_ref, (0, 2, 3), m2.A_qmax, HEAD_FACTORS["pA"])
        out_ref = m2.quant_forward(p_ref, v)
        p64 = torch.softmax(u_ref.double().cpu(), dim=-1).float().cuda()
        assert bool((p64 >= 2.0 ** -126).all()), "every probability is a normal fp32 number"
        sides = _matmul_side(m1, H), _matmul_side(m2, H)
        with Guard(eng, monkeypatch, 0xCD) as g:
            out, probs, planes = eng.attn_quant_forward(q=q, kT=kT, v=v, scale=scale, qk=sides[0], pv=sides[1], want_probs=True,
                                                        want_planes=True)
            reps = g.finish()
        assert len(reps) == 1 and reps[0]["guard_changed"] == 0 and 0 < reps[0]["touched"] <= reps[0]["need"], reps
    r = dict(m1=m1, m2=m2, q=q, kT=kT, v=v, scale=scale, sides=sides, out=out, probs=probs, planes=planes, u_ref=u_ref, p_ref=p_ref,
             p64=p64, out_ref=out_ref, need=reps[0]["need"], gap=gap)
    _RUNS[name] = r
    return r


def _packed(eng, m2, p):
    """matmul2's row plane(s) as the unfused forward packs them from the fp32 probabilities `p` [B][H][M][N]: padded [Z][M][Kp]"""
    B, H, M, N = p.shape
    Z, q = B * H, m2.A_qmax
    p2 = p.reshape(Z * M, N)
    if m2._sos:
        _, _, p1, p2_ = eng.debug_pack_dual(p2, sos=True, scale=float(m2.split), lo=0, hi=q - 1, qmax=q)
        return p1.reshape(Z, M, -1), p2_.reshape(Z, M, -1)
    a_iv = m2.A_interval.reshape(-1)
    scales = a_iv[torch.arange(Z, device=a_iv.device) % H]
    _, p1 = eng.pack_plane_i8(p2, mode="sym", scales=scales, rows_per_scale=M, lo=-q, hi=q - 1)
    return (p1.reshape(Z, M, -1),)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_planes_are_the_packers_bytes_of_the_calls_own_probs(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    B, H, N, D = case[1]
    M = N
    want = _packed(eng, r["m2"], r["probs"])
    assert len(want) == len(r["planes"]) == (2 if case[2] else 1)
    for got, ref in zip(r["planes"], want):
        assert got.shape[0] == B * H and got.shape[1] % 128 == 0 and got.shape[1] >= M and got.shape[2] == ref.shape[2] == (N + 63) // 64 * 64
        for z in range(B * H):
            assert torch.equal(got[z, :M], ref[z]), f"{case[0]} z {z}: {(got[z, :M] != ref[z]).sum().item()} bytes differ from the packer's"
        assert not got[:, M:].any(), "padding rows must be zero"
        assert not got[:, :, N:].any(), "padding columns must be zero"
    assert r["planes"][0].any() and (not case[2] or r["planes"][1].any())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_out_is_matmul2_quant_forward_of_the_calls_own_probs(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    B, H, N, D = case[1]
    with torch.no_grad():
        want = r["m2"].quant_forward(r["probs"], r["v"])
    assert r["out"].shape == want.shape == (B, H, N, D)
    assert torch.equal(r["out"], want), f"{case[0]}: max |diff| {(r['out'] - want).abs().max().item():.3e}"


def _ulps(r):
    """(U_t, U_k, U): torch and the kernel against the rounded float64 softmax, and the kernel against torch"""
    return (int(ulp_distance(r["p_ref"], r["p64"]).max()), int(ulp_distance(r["probs"], r["p64"]).max()),
            int(ulp_distance(r["probs"], r["p_ref"]).max()))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_softmax_is_as_close_to_float64_as_torchs(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    assert torch.isfinite(r["probs"]).all()
    rows = r["probs"].sum(-1)
    assert float((rows - 1).abs().max()) < 1e-5
    U_t, U_k, U = _ulps(r)
    print(f"[fused attn] {case[0]}: max - u up to {r['gap']:.1f}; ulps vs float64: torch {U_t}, kernel {U_k}; kernel vs torch {U}")
    _MARGINS.setdefault("softmax_ulp", {})[case[0]] = dict(torch_vs_f64=U_t, kernel_vs_f64=U_k, kernel_vs_torch=U, max_minus_u=r["gap"])
    assert U_k <= max(2 * U_t, ULP_FLOOR), f"{case[0]}: kernel {U_k} ulp, torch {U_t} ulp"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_planes_against_the_unfused_chain(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    U = _ulps(r)[2]
    flips = _count_flips(eng, r["m2"], r["planes"], r["p_ref"], U, case[0])
    print(f"[fused attn] {case[0]}: {flips} plane bytes differ from the unfused chain's (U = {U})")
    _MARGINS.setdefault("plane_bytes_differing_from_unfused", {})[case[0]] = flips
    with torch.no_grad():
        rel = ((r["out"] - r["out_ref"]).norm() / r["out_ref"].norm()).item()
    _MARGINS.setdefault("out_rel_diff_vs_unfused", {})[case[0]] = rel
    if flips == 0:
        assert torch.equal(r["out"], r["out_ref"])


def _count_flips(eng, m2, planes, p_ref, U, what):
    """Bytes of `planes` that differ from the unfused packer's bytes of `p_ref`, each held to one grid step next to a rounding tie."""
    B, H, M, N = p_ref.shape
    q1 = m2.A_qmax - 1
    p = p_ref.reshape(B * H, M, N).double()
    if m2._sos:
        split = float(m2.split)
        a_int = float(np.float32(split) / np.float32(q1))            # pack_value: a_int = s / qm1 in fp32
        ts = [p.clamp(split, 1.0) * q1, p.clamp(0.0, split) / a_int]
    else:
        a_iv = m2.A_interval.reshape(-1).double()
        ts = [p / a_iv[torch.arange(B * H, device=p.device) % H].view(-1, 1, 1)]
    flips = 0
    for got, ref, t in zip(planes, _packed(eng, m2, p_ref), ts):
        a, b = got[:, :M, :N].to(torch.int32), ref[:, :, :N].to(torch.int32)
        diff = a != b
        if diff.any():
            near = ((t - torch.floor(t) - 0.5).abs() <= (U + 1) * 2.0 ** -23 * t.abs().clamp(min=1.0))
            assert ((a - b).abs()[diff] == 1).all(), f"{what}: a byte differs by more than one grid step"
            assert near[diff].all(), f"{what}: {(diff & ~near).sum().item()} bytes differ away from a rounding tie"
        flips += int(diff.sum())
    return flips


# ---- 5: the contract ------------------------------------------------------------------------------------------------------------
def test_workspace_contract_and_envelope(eng, monkeypatch):
    case = CASES[0]
    r = run_case(eng, monkeypatch, case)          # (the exact, guarded, poisoned call)
    q, kT, v, scale, (qk, pv) = r["q"], r["kT"], r["v"], r["scale"], r["sides"]
    torch.cuda.synchronize()
    with torch.no_grad():
        # one byte less: refused, nothing launched
        before = eng.launch_counters()
        with Guard(eng, monkeypatch, 0xCD, declare=lambda n: n - 1) as g:
            with pytest.raises(RuntimeError, match="workspace too small"):
                eng.attn_quant_forward(q=q, kT=kT, v=v, scale=scale, qk=qk, pv=pv)
            reps = g.finish()
        assert eng.launch_counters() == before
        assert all(rep["touched"] == 0 and rep["guard_changed"] == 0 for rep in reps), reps
        # outside the envelope: refused before any launch
        for which in (0, 1):
            sides = [dict(qk), dict(pv)]
            sides[which]["blocks"] = (1, 1, 2, 2)
            with pytest.raises(NotImplementedError, match="sub-blocks"):
                eng.attn_quant_forward(q=q, kT=kT, v=v, scale=scale, qk=sides[0], pv=sides[1])
        sos_qk = dict(qk, sos=True, split=pv["split"], A_interval=pv["A_interval"])
        with pytest.raises(NotImplementedError, match="split-of-softmax"):
            eng.attn_quant_forward(q=q, kT=kT, v=v, scale=scale, qk=sos_qk, pv=pv)
        with pytest.raises(RuntimeError, match="is not the row operand"):
            eng.attn_quant_forward(q=q, kT=kT, v=v[:, :, :-1], scale=scale, qk=qk, pv=pv)      # qk.N = 197, pv.K = 196
        assert eng.launch_counters() == before
        # no probabilities asked for: the same out
        out = eng.attn_quant_forward(q=q, kT=kT, v=v, scale=scale, qk=qk, pv=pv)
        assert torch.equal(out, r["out"])
        assert eng.launch_counters()["asked"] > before["asked"]


# ---- 6: module level, the mini ViT -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mini():
    from ptq4vit_amd.configs import PTQ4ViT
    from ptq4vit_amd.utils import models, net_wrap
    from ptq4vit_amd.utils.quant_calib import HessianQuantCalibrator
    g = np.load("tests/golden/minivit_ptq4vit.npz", allow_pickle=False)
    kw = json.loads(str(g["model_kwargs"]))
    assert kw["img_size"] == 32
    net = models.get_net("vit_tiny_patch16_224", seed=0, device="cuda", **kw)
    assert isinstance(net, models.VisionTransformer)
    wrapped = net_wrap.wrap_modules_in_net(net, PTQ4ViT)
    images = torch.from_numpy(g["images"][:4]).cuda()
    HessianQuantCalibrator(net, wrapped, _Loader(images), sequential=False, batch_size=4).batching_quant_calib()
    return net, wrapped, images


def _attention_names(net):
    from ptq4vit_amd.utils import models
    return [n for n, m in net.named_modules() if isinstance(m, models.Attention)]


def _own_tensor_flips(eng, net, images):
    """The differing plane bytes of 4, counted on the UNFUSED net's own attention tensors: (flips, probability bytes).  With 0
    flips in every block the fused net sees the same tensors block after block, and its logits are the unfused net's."""
    from ptq4vit_amd.utils import fuse
    mods = dict(net.named_modules())
    seen = {}
    hooks = []
    for n in _attention_names(net):
        for mm in ("matmul1", "matmul2"):
            hooks.append(getattr(mods[n], mm).register_forward_hook(
                lambda mod, inp, out, key=(n, mm): seen.__setitem__(key, tuple(t.detach() for t in inp))))
    try:
        with torch.no_grad():
            net(images)
    finally:
        for h in hooks:
            h.remove()
    flips = total = 0
    for n in _attention_names(net):
        att = mods[n]
        (q, kT), (p_ref, v) = seen[(n, "matmul1")], seen[(n, "matmul2")]
        H = q.shape[1]
        with torch.no_grad():
            _, probs, planes = eng.attn_quant_forward(q=q, kT=kT, v=v, scale=att.scale, qk=fuse._matmul_side(att.matmul1, H),
                                                      pv=fuse._matmul_side(att.matmul2, H), want_probs=True, want_planes=True)
        U = int(ulp_distance(probs, p_ref).max())
        flips += _count_flips(eng, att.matmul2, planes, p_ref, U, n)
        total += p_ref.numel() * len(planes)
    return flips, total


def _held_to_the_flips(y_f, y_u, y_raw, flips, total):
    """Fused against unfused logits: bit-identical when no plane byte differs.  Otherwise the bar is what `flips` bytes can explain.
    A flip moves one probability by one grid step; the rounding of every element moves it by a uniform error of variance
    step^2 / 12; so a share f of flipped bytes enters with r0 = sqrt(12 f) of the amplitude the rounding noise has.  The quantisers
    downstream round again: a perturbation d << step flips an element with probability d / step, by a whole step each, which
    turns the energy d^2 into d * step -- relative to the rounding noise r -> 12^(1/4) sqrt(r), applied once (the perturbed
    tensors are re-quantised by the next module; further stages act on ever fewer elements' worth of change).  Never above 1:
    a tie rounded the other way is another rounding of the same value, of the kind |unfused - raw| is made of."""
    ratio = ((y_f - y_u).norm() / (y_u - y_raw).norm()).item()
    if flips == 0:
        assert torch.equal(y_f, y_u), f"no plane byte differs, the logits do: ratio {ratio:.3e}"
    else:
        r0 = (12.0 * flips / total) ** 0.5
        assert ratio <= min(1.0, 12.0 ** 0.25 * r0 ** 0.5), (ratio, flips, total)
    return ratio


def test_fused_net_logits_and_fallbacks(eng, mini, monkeypatch):
    from ptq4vit_amd.utils import fuse, models
    net, wrapped, images = mini
    attns = _attention_names(net)
    assert len(attns) == 2
    flips, total = _own_tensor_flips(eng, net, images)
    calls = _count_fused_calls(eng, monkeypatch, "attn_quant_forward")
    cls_forward = models.Attention.forward
    mods = dict(net.named_modules())
    try:
        with torch.no_grad():
            y_u = net(images)
            assert not calls
            assert fuse.fuse_attention(net) == attns
            assert fuse.fuse_attention(net) == attns                      # idempotent
            assert all(fuse.takes_fused_attention_path(mods[n], torch.empty(4, 5, mods[n].qkv.in_features, device="cuda")) for n in attns)
            y_f = net(images)
            assert len(calls) == len(attns), "the fused path did not run"
            for m in wrapped.values():
                m.mode = "raw"
            del calls[:]
            y_raw = net(images)
            assert not calls, "raw mode must take the original forward"
            fuse.unfuse_attention(net)
            assert torch.equal(net(images), y_raw)
            fuse.fuse_attention(net)
            for m in wrapped.values():
                m.mode = "quant_forward"
            ratio = _held_to_the_flips(y_f, y_u, y_raw, flips, total)
            print(f"[fused attn] mini ViT: {flips} of {total} plane bytes differ; |fused - unfused| / |unfused - raw| = {ratio:.3e}")
            _MARGINS["minivit"] = dict(plane_bytes_differing=flips, plane_bytes=total, fused_over_quant_error=ratio)

            # fuse_mlp + fuse_attention compose, in either order
            fuse.fuse_mlp(net)
            y_am = net(images)
            fuse.unfuse_attention(net)
            fuse.unfuse_mlp(net)
            fuse.fuse_mlp(net)
            fuse.fuse_attention(net)
            del calls[:]
            y_ma = net(images)
            assert len(calls) == len(attns) and torch.equal(y_am, y_ma)
            fuse.unfuse_mlp(net)
            assert torch.equal(net(images), y_f)

            att = mods[attns[0]]
            # (the net's own 17 tokens: the fp32 fake-quant forward that autograd and the CPU take views its operands in the
            # block geometry of the calibration tensors)
            probe = torch.randn(4, 17, att.qkv.in_features, device="cuda")

            def unfused_twin(fn):
                """fn() on the fused net, then on the same net unfused, in whatever state it is in"""
                a = fn()
                fuse.unfuse_attention(net)
                b = fn()
                fuse.fuse_attention(net)
                return a, b

            # a forward hook on matmul1: it fires, that block takes the original forward, the output is the unfused net's
            fired = []
            h = att.matmul1.register_forward_hook(lambda mod, inp, out: fired.append(tuple(out.shape)))
            del calls[:]
            y_a, y_b = unfused_twin(lambda: net(images))
            assert len(fired) == 2 and len(calls) == len(attns) - 1
            assert torch.equal(y_a, y_b)
            del calls[:]
            m_a, m_b = unfused_twin(lambda: att(probe))
            assert not calls and torch.equal(m_a, m_b)
            h.remove()
            # autograd recording: the original forward
            del calls[:]
            with torch.enable_grad():
                m_a, m_b = unfused_twin(lambda: att(probe.clone().requires_grad_(True)))
            assert not calls and torch.equal(m_a, m_b)
            # CPU tensors: the original forward
            att_cpu = copy.deepcopy(att).cpu()
            for m in att_cpu.modules():                    # (the intervals are plain attributes: .cpu() does not move them)
                for a in ("w_interval", "a_interval", "A_interval", "B_interval", "split"):
                    if torch.is_tensor(getattr(m, a, None)):
                        setattr(m, a, getattr(m, a).cpu())
            holder = torch.nn.Sequential(att_cpu)
            assert fuse.fuse_attention(holder) == ["0"]
            m_a = att_cpu(probe.cpu())
            assert fuse.unfuse_attention(holder) == ["0"]
            assert not calls and torch.equal(m_a, att_cpu(probe.cpu()))
            # everything back: fused again, and deterministic
            del calls[:]
            assert torch.equal(net(images), y_f) and len(calls) == len(attns)
    finally:
        fuse.unfuse_attention(net)
        fuse.unfuse_mlp(net)
    # unfuse_attention restores the original forward
    for n in attns:
        m = dict(net.named_modules())[n]
        assert "forward" not in m.__dict__ and m.forward.__func__ is cls_forward
    assert fuse.unfuse_attention(net) == []
    with torch.no_grad():
        del calls[:]
        assert torch.equal(net(images), y_u) and not calls
    # ... an instance-attribute forward that was there before included
    att = mods[attns[1]]
    mine = lambda x: cls_forward(att, x)
    att.forward = mine
    try:
        assert fuse.fuse_attention(net) == attns and att.__dict__["forward"] is not mine
        assert fuse.unfuse_attention(net) == attns and att.__dict__["forward"] is mine
    finally:
        att.__dict__.pop("forward", None)


@pytest.mark.parametrize("contiguous", ["1", "0"])
def test_both_qkv_layouts_take_the_fused_path(eng, mini, monkeypatch, contiguous):
    from ptq4vit_amd.utils import fuse
    net, wrapped, images = mini
    monkeypatch.setenv("P4V_QKV_CONTIGUOUS", contiguous)
    fuse.unfuse_attention(net)
    flips, total = _own_tensor_flips(eng, net, images)
    calls = _count_fused_calls(eng, monkeypatch, "attn_quant_forward")
    try:
        with torch.no_grad():
            y_u = net(images)
            for m in wrapped.values():
                m.mode = "raw"
            y_raw = net(images)
            for m in wrapped.values():
                m.mode = "quant_forward"
            assert not calls
            fuse.fuse_attention(net)
            y_f = net(images)
            assert len(calls) == 2
            _MARGINS.setdefault("minivit_qkv_contiguous", {})[contiguous] = _held_to_the_flips(y_f, y_u, y_raw, flips, total)
    finally:
        fuse.unfuse_attention(net)


def test_second_calibration_of_a_fused_net_gives_the_unfused_intervals(eng, mini, monkeypatch):
    from ptq4vit_amd.utils import fuse
    from ptq4vit_amd.utils.quant_calib import HessianQuantCalibrator
    net, wrapped, images = mini
    fuse.unfuse_attention(net)
    net_u = copy.deepcopy(net)
    wrapped_u = _wrapped_of(net_u, wrapped)
    net_f = copy.deepcopy(net)
    wrapped_f = _wrapped_of(net_f, wrapped)
    assert len(fuse.fuse_attention(net_f)) == 2
    HessianQuantCalibrator(net_u, wrapped_u, _Loader(images), sequential=False, batch_size=4).batching_quant_calib()
    HessianQuantCalibrator(net_f, wrapped_f, _Loader(images), sequential=False, batch_size=4).batching_quant_calib()
    iu, ifu = _intervals(wrapped_u), _intervals(wrapped_f)
    assert iu.keys() == ifu.keys() and len(iu) >= len(wrapped)
    for k in iu:
        assert torch.equal(iu[k], ifu[k]), k
    # ... and the fused net is still fused, and runs fused
    calls = _count_fused_calls(eng, monkeypatch, "attn_quant_forward")
    with torch.no_grad():
        net_f(images)
    assert len(calls) == 2
