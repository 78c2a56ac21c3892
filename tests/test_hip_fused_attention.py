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

7. the float64 stage references (tests/fused_reference.py; their own test: tests/test_fused_reference_cpu.py), on every case:
   probs against the float64 softmax of the exact integer product of the oracle's quantisers on the RAW q and k^T
   (|probs - p64| <= p64 U_row 2^-23, U_row = 10 + N / 64 + 5 max |u|; below 2^-100: 0 <= probs <= 2^-99); the planes against the
   oracle's sos_planes / quant_int of the call's own probs on the CPU, exactly; `out` against the int64 GEMM of the call's own
   planes with quant_int(v), scaled in float64, at the int8-forward bar 2e-6 sqrt(K).  1, 2 and 3 compare with this library's
   other kernels, which are pinned to the oracle at their own tests' shapes only; 7 has no kernel of the library in it;
8. degenerate intervals (a zero q / k^T / v head under the min-max rule), next to the same call on healthy data: probs (v: out)
   of that head all NaN, its plane bytes on the grid, every other head's probs, planes and out bit-identical.

Shapes (the smallest that reach every edge): 197 queries and keys (a full 128-row tile and a ragged one, six full 32-key tiles
and a ragged one, Kp = 256), head_dim 64 and 40 (ragged k-tile), 50 keys (less than one 64-byte piece row), 577 keys (ViT-B/384);
head_dim 128 and 80 (the ktiles >= 2 score tile, split-of-softmax and plain; 80: a ragged second k-tile), one query for 197 keys,
130 queries for 64 keys (M > N, keys exactly one 64-byte piece, 2 rows in the second row tile), 256 x 256 (no padding anywhere),
5 x 5 (fewer keys than one register quad stride), 1025 x 1025 (33 key tiles, matmul2 with ktiles = 17), Dv = 96 != D; matmul2 with
A_bit != B_bit (2 / 8 -- q - 1 = 1 --, 8 / 4, plain 4 / 8), the split at both ends of its grid (1 and 2^-19); k^T one vector repeated
(every key ties: probs = float32(1 / N) bit for bit); q x 24 (max - u up to 186: expf underflows through the subnormals to 0, over 10 %
of the rows nearly one-hot -- the one case exempt from the `max - u < 80` / all-normal guard; its ulp comparison with torch is
taken where p64 >= 2^-100, the rest is 7's second clause).

With P4V_FUSED_ATTN_OUT set the measured margins are written there, under "attention" (profiles/r24_fused_edges_margins.json; the
nine older cases alone: profiles/r22_fused_attn_margins.json).
"""
import copy
import json
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import fused_reference as fr
from tests.fused_common import _Loader, _count_fused_calls, _intervals, _wrapped_of, merge_margins, ulp_distance
from tests.workspace_guard import Guard

pytestmark = pytest.mark.gpu

SPLIT = 2.0 ** -5                 # of the reference's grid 2^-i, i < 20 (matmul.py:636)
HEAD_FACTORS = {"qA": (1.0, 0.8, 1.25), "qB": (0.9, 1.15, 1.0), "pA": (1.1, 0.9, 1.0), "pB": (1.2, 1.0, 0.85)}
ULP_FLOOR = 8
_MARGINS = {}

Case = namedtuple("Case", "name shape twin pv_bits qk_bits qf strided split special", defaults=(SPLIT, None))
S197, S197D = (2, 3, 197, 197, 64, 64), (1, 2, 197, 197, 64, 64)
#               id                (batch, H, M, N, D, Dv)      twin   pv (A, B) bits  qk (A, B) bits  q factor  strided  split  special
CASES = [Case("sos_w8a8",         S197,                        True,  (8, 8),         (8, 8),         1.0,      False),
         Case("sos_w6a6",         S197,                        True,  (6, 6),         (6, 6),         1.0,      False),
         Case("plain_w8a8",       S197,                        False, (8, 8),         (8, 8),         1.0,      False),
         Case("sos_qk_a8b4",      S197,                        True,  (8, 8),         (8, 4),         1.0,      False),
         Case("sos_d40",          (2, 3, 197, 197, 40, 40),    True,  (8, 8),         (8, 8),         1.0,      False),
         Case("sos_n50",          (2, 3, 50, 50, 64, 64),      True,  (8, 8),         (8, 8),         1.0,      False),
         Case("sos_n577",         (1, 2, 577, 577, 64, 64),    True,  (8, 8),         (8, 8),         1.0,      False),
         Case("sos_wide",         S197,                        True,  (8, 8),         (8, 8),         8.0,      False),
         Case("sos_strided",      S197,                        True,  (8, 8),         (8, 8),         1.0,      True),
         # head_dim above 64: the ktiles >= 2 score tile of both instances (matmul2's column plane is then not b64 either)
         Case("sos_d128",         (1, 2, 197, 197, 128, 128),  True,  (8, 8),         (8, 8),         1.0,      False),
         Case("plain_d128",       (1, 2, 197, 197, 128, 128),  False, (8, 8),         (8, 8),         1.0,      False),
         Case("sos_d80",          (1, 2, 197, 197, 80, 80),    True,  (8, 8),         (8, 8),         1.0,      False),
         # M != N, Dv != D, no padding at all, fewer keys than a register quad stride, matmul2 ktiles = 17
         Case("sos_m1",           (2, 3, 1, 197, 64, 64),      True,  (8, 8),         (8, 8),         1.0,      False),
         Case("sos_m130_n64",     (1, 2, 130, 64, 64, 64),     True,  (8, 8),         (8, 8),         1.0,      False),
         Case("sos_n256",         (1, 2, 256, 256, 64, 64),    True,  (8, 8),         (8, 8),         1.0,      False),
         Case("sos_n5",           (2, 3, 5, 5, 16, 16),        True,  (8, 8),         (8, 8),         1.0,      False),
         Case("sos_n1025",        (1, 1, 1025, 1025, 64, 64),  True,  (8, 8),         (8, 8),         1.0,      False),
         Case("sos_dv96",         (1, 2, 197, 197, 64, 96),    True,  (8, 8),         (8, 8),         1.0,      False),
         # matmul2's quantiser settings: A_bit != B_bit, q - 1 = 1, both ends of the split grid
         Case("sos_pv_a2b8",      S197D,                       True,  (2, 8),         (8, 8),         4.0,      False),   # (q x 4: 176 p >= 0.5 -- with q - 1 = 1 plane 1 is 0 below that)
         Case("sos_pv_a8b4",      S197D,                       True,  (8, 4),         (8, 8),         1.0,      False),
         Case("plain_pv_a4b8",    S197D,                       False, (4, 8),         (8, 8),         1.0,      False),
         Case("sos_split_1",      S197D,                       True,  (8, 8),         (8, 8),         1.0,      False,   1.0),
         Case("sos_split_2e-19",  S197D,                       True,  (8, 8),         (8, 8),         1.0,      False,   2.0 ** -19),
         # every key ties for the maximum; rows that are nearly one-hot, expf underflowing through the subnormals to 0
         Case("sos_keys_equal",   (1, 2, 70, 70, 64, 64),      True,  (8, 8),         (8, 8),         1.0,      False,   SPLIT, "keys_equal"),
         Case("sos_peaked",       S197D,                       True,  (8, 8),         (8, 8),         24.0,     False,   SPLIT, "peaked")]
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    yield engine
    engine.release_workspace()
    merge_margins(os.environ.get("P4V_FUSED_ATTN_OUT"), "attention", _MARGINS, IDS)


def _inputs(case, device="cuda"):
    """q, kT, v as Attention.forward hands them over: views of the qkv Linear's output [B][N][3][H][D] -- three tensors of their
    own where the queries and keys differ in number or v in head dimension."""
    name, (B, H, M, N, D, Dv), qf, strided = case.name, case.shape, case.qf, case.strided
    g = torch.Generator().manual_seed(2200 + IDS.index(name))
    if M == N and D == Dv:
        qkv = torch.randn(B, N, 3, H, D, generator=g)
        qkv[:, :, 0] *= qf
        if case.special == "keys_equal":
            qkv[:, :, 1] = qkv[:, :1, 1]
        qkv = qkv.to(device).permute(2, 0, 3, 1, 4)
        if not strided:
            qkv = qkv.contiguous()
        q, k, v = qkv.unbind(0)
    else:
        assert not strided and case.special is None
        q, k, v = (torch.randn(B, n, H, d, generator=g).to(device).permute(0, 2, 1, 3).contiguous() for n, d in ((M, D), (N, D), (N, Dv)))
        q = q * qf
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
    twin, (pa, pb), (qa, qb) = case.twin, case.pv_bits, case.qk_bits
    m1 = PTQSLBatchingQuantMatMul(A_bit=qa, B_bit=qb, mode="quant_forward")
    m1.A_interval = _headwise(q, (0, 2, 3), m1.A_qmax, HEAD_FACTORS["qA"])
    m1.B_interval = _headwise(kT, (0, 2, 3), m1.B_qmax, HEAD_FACTORS["qB"])
    m1.calibrated = True
    if twin:
        m2 = SoSPTQSLBatchingQuantMatMul(A_bit=pa, B_bit=pb, mode="quant_forward", split=torch.tensor(case.split, device="cuda"))
        assert float(m2.A_interval) == float(np.float32(case.split) / np.float32(m2.A_qmax - 1))       # A_interval = split / (q - 1)
    else:
        m2 = PTQSLBatchingQuantMatMul(A_bit=pa, B_bit=pb, mode="quant_forward")
    m2.B_interval = _headwise(v, (0, 2, 3), m2.B_qmax, HEAD_FACTORS["pB"])
    m2.calibrated = True
    return m1, m2


_RUNS = {}


def run_case(eng, monkeypatch, case):
    """One fused call per case (exact, guarded, poisoned workspace) and the unfused chain next to it; shared by the tests."""
    name, (B, H, M, N, D, Dv), twin = case[0], case[1], case[2]
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
        if case.special != "peaked":                  # (the one case made of underflowing rows: held by the float64 stage reference)
            assert gap < 80.0, f"{name}: max - u = {gap}: a probability would be subnormal"
        p_ref = u_ref.softmax(dim=-1)
        if not twin:
            m2.A_interval = _headwise(p_ref, (0, 2, 3), m2.A_qmax, HEAD_FACTORS["pA"])
        out_ref = m2.quant_forward(p_ref, v)
        p64 = torch.softmax(u_ref.double().cpu(), dim=-1).float().cuda()
        if case.special != "peaked":
            assert bool((p64 >= 2.0 ** -126).all()), "every probability is a normal fp32 number"
        sides = _matmul_side(m1, H), _matmul_side(m2, H)
        with Guard(eng, monkeypatch, 0xCD) as g:
            out, probs, planes = eng.attn_quant_forward(q=q, kT=kT, v=v, scale=scale, qk=sides[0], pv=sides[1], want_probs=True,
                                                        want_planes=True)
            reps = g.finish()
        assert len(reps) == 1 and reps[0]["guard_changed"] == 0 and 0 < reps[0]["touched"] <= reps[0]["need"], reps
    r = dict(m1=m1, m2=m2, q=q, kT=kT, v=v, scale=scale, sides=sides, out=out, probs=probs, planes=planes, u_ref=u_ref, p_ref=p_ref,
             p64=p64, out_ref=out_ref, need=reps[0]["need"], gap=gap, live=None)
    if case.special == "peaked":                      # the ulp comparison with torch: where the float64 reference is >= 2^-100
        r["live"] = torch.from_numpy(_stage_reference(r)[1] >= fr.P_FLOOR).cuda()
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
    B, H, M, N, D, Dv = case[1]
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
    B, H, M, N, D, Dv = case[1]
    with torch.no_grad():
        want = r["m2"].quant_forward(r["probs"], r["v"])
    assert r["out"].shape == want.shape == (B, H, M, Dv)
    assert torch.equal(r["out"], want), f"{case[0]}: max |diff| {(r['out'] - want).abs().max().item():.3e}"


def _ulps(r):
    """(U_t, U_k, U): torch and the kernel against the rounded float64 softmax, and the kernel against torch"""
    live = (lambda d: d) if r["live"] is None else (lambda d: d[r["live"]])      # (sos_peaked: entries with p64 >= 2^-100)
    return (int(live(ulp_distance(r["p_ref"], r["p64"])).max()), int(live(ulp_distance(r["probs"], r["p64"])).max()),
            int(live(ulp_distance(r["probs"], r["p_ref"])).max()))


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


# ---- the float64 stage references (tests/fused_reference.py) ----------------------------------------------------------------------
def _pv_kw(m2):
    return dict(sos=m2._sos, A_bit=m2.A_bit, split=m2.split if m2._sos else None, A_iv=m2.A_interval)


def _stage_reference(r):
    """(u64, p64) of the case's raw inputs and matmul1's intervals, computed once per case"""
    if "stage1" not in r:
        m1 = r["m1"]
        r["stage1"] = fr.attn_float_stage(r["q"], r["kT"], m1.A_interval, m1.B_interval, m1.A_bit, m1.B_bit, r["scale"])
    return r["stage1"]


def _check_stages(r, what, skip_heads=()):
    """The three stage checks on one call's probs, planes and out; returns the ratios.  `skip_heads`: heads whose planes hold
    undefined bytes (NaN probabilities): their `out` is not compared."""
    m2 = r["m2"]
    B, H, M, N = r["probs"].shape
    u64, p64 = _stage_reference(r)
    s1 = fr.check_probs(r["probs"], u64, p64, what)
    want, nan, grid = fr.attn_planes_of(r["probs"], H, **_pv_kw(m2))
    n = fr.check_planes(r["planes"], want, nan, grid, what)
    ref = fr.attn_consumer_stage(r["planes"], r["v"], H, sos=m2._sos, A_bit=m2.A_bit, B_bit=m2.B_bit, B_iv=m2.B_interval,
                                 A_iv=m2.A_interval, M=M, N=N)
    skip = np.zeros((1, H, 1, 1), bool)
    skip[0, list(skip_heads)] = True
    s3 = fr.check_out(r["out"], ref, N, what, skip=skip)
    return dict(probs_over_bound=s1, plane_bytes_compared=n, out_over_bar=s3)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stages_against_the_float64_references(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    got = _check_stages(r, case.name)
    print(f"[fused attn] {case.name}: |probs - p64| / bound {got['probs_over_bound']:.3f}; {got['plane_bytes_compared']} plane bytes exact; "
          f"|out - ref| / bar {got['out_over_bar']:.3f}")
    _MARGINS.setdefault("stage_ratios", {})[case.name] = got
    assert got["plane_bytes_compared"] == r["probs"].numel() * len(r["planes"])


def test_equal_keys_give_one_over_n_bit_for_bit(eng, monkeypatch):
    """expf(0) = 1, the row sum is the exact integer N, the division is IEEE: float32(1 / N) and nothing else"""
    case = CASES[IDS.index("sos_keys_equal")]
    r = run_case(eng, monkeypatch, case)
    N = case.shape[3]
    assert bool((r["kT"] == r["kT"][..., :1]).all())
    want = torch.full_like(r["probs"], float(np.float32(1.0) / np.float32(N)))
    assert torch.equal(r["probs"], want), f"{int((r['probs'] != want).sum())} probabilities are not float32(1 / {N})"


def test_peaked_rows_underflow(eng, monkeypatch):
    """the premise of sos_peaked on the call itself: probabilities that underflowed to 0 next to rows that are nearly one-hot"""
    r = run_case(eng, monkeypatch, CASES[IDS.index("sos_peaked")])
    assert r["gap"] > 150.0
    assert bool((r["probs"] == 0).any()) and float((r["probs"] < 2.0 ** -100).float().mean()) >= 0.1
    assert float((r["probs"].amax(-1) > 0.999).float().mean()) >= 0.1


# ---- degenerate intervals: a head of zeros under the min-max rule -----------------------------------------------------------------------
DEGEN_SHAPE = (2, 3, 70, 70, 64, 64)


def _degen_inputs(zero, device="cuda"):
    """q, kT, v of DEGEN_SHAPE, head 1 of `zero` ("q", "kT", "v" or None) zeroed"""
    g = torch.Generator().manual_seed(2290)
    B, H, M, N, D, Dv = DEGEN_SHAPE
    t = {n: torch.randn(B, H, r, c, generator=g).to(device) for n, (r, c) in (("q", (M, D)), ("kT", (D, N)), ("v", (N, Dv)))}
    if zero is not None:
        t[zero][:, 1] = 0.0
    return t["q"], t["kT"], t["v"]


def _degen_run(eng, monkeypatch, twin, zero):
    """The fused call on the data of a case of DEGEN_SHAPE with head 1 of `zero` ("q", "kT", "v" or None) zeroed; min-max intervals"""
    key = ("degen", twin, zero)
    if key in _RUNS:
        return _RUNS[key]
    from ptq4vit_amd.quant_layers.matmul import PTQSLBatchingQuantMatMul
    from ptq4vit_amd.utils.fuse import _matmul_side
    case = Case("degen", DEGEN_SHAPE, twin, (8, 8), (8, 8), 1.0, False)
    B, H, M, N, D, Dv = DEGEN_SHAPE
    q, kT, v = _degen_inputs(zero)
    m1, m2 = _modules(case, q, kT, v)
    if not twin:                                     # (a fixed head-wise interval: the same in the healthy and the degenerate run)
        m2.A_interval = (torch.tensor([0.9, 1.1, 1.0], device="cuda") / (m2.A_qmax - 0.5)).view(1, H, 1, 1, 1, 1, 1)
    assert isinstance(m2, PTQSLBatchingQuantMatMul)
    scale = D ** -0.5
    sides = _matmul_side(m1, H), _matmul_side(m2, H)
    with torch.no_grad(), Guard(eng, monkeypatch, 0xCD) as gd:
        out, probs, planes = eng.attn_quant_forward(q=q, kT=kT, v=v, scale=scale, qk=sides[0], pv=sides[1], want_probs=True, want_planes=True)
        reps = gd.finish()
    assert len(reps) == 1 and reps[0]["guard_changed"] == 0 and 0 < reps[0]["touched"] <= reps[0]["need"], reps
    r = dict(m1=m1, m2=m2, q=q, kT=kT, v=v, scale=scale, out=out, probs=probs, planes=planes)
    _RUNS[key] = r
    return r


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("twin", [True, False], ids=["sos", "plain"])
@pytest.mark.parametrize("zero", ["q", "kT", "v"])
def test_a_zero_head_poisons_that_head_alone(eng, monkeypatch, twin, zero):
    bad, good = _degen_run(eng, monkeypatch, twin, zero), _degen_run(eng, monkeypatch, twin, None)
    B, H = DEGEN_SHAPE[:2]
    others = [h for h in range(H) if h != 1]
    iv = {"q": bad["m1"].A_interval, "kT": bad["m1"].B_interval, "v": bad["m2"].B_interval}[zero].reshape(-1)
    assert float(iv[1]) == 0.0 and bool((iv[others] > 0).all()), "the min-max interval of the zero head, and of it alone, is 0"
    what = f"zero {zero} head, {'sos' if twin else 'plain'}"
    if zero == "v":
        assert torch.isnan(bad["out"][:, 1]).all(), "out of the head whose v interval is 0 is the reference's NaN"
        assert _same_bits(bad["probs"], good["probs"])
        assert all(torch.equal(a, b) for a, b in zip(bad["planes"], good["planes"]))
        got = _check_stages(bad, what)
    else:
        assert torch.isnan(bad["probs"][:, 1]).all(), "0 / 0 poisons every probability of the head"
        got = _check_stages(bad, what, skip_heads=(1,))          # (the NaN head's plane bytes: on the grid, checked there)
    _MARGINS.setdefault("degenerate", {})[what] = got
    assert torch.isfinite(bad["probs"][:, others]).all() and torch.isfinite(bad["out"][:, others]).all()
    assert _same_bits(bad["probs"][:, others], good["probs"][:, others])
    assert _same_bits(bad["out"][:, others], good["out"][:, others])
    for a, b in zip(bad["planes"], good["planes"]):
        a, b = a.view(B, H, *a.shape[1:]), b.view(B, H, *b.shape[1:])
        assert torch.equal(a[:, others], b[:, others])


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
