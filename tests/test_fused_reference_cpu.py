"""CPU: the stage references of the fused int8 forwards (tests/fused_reference.py) held against an fp32 emulation of each chain.

The emulation is plain torch on the CPU in the kernels' order of operations -- the int32 accumulator times the fp32 scale
product, `* scale`, the row maximum, expf, the row sum, one IEEE division; `+ bias`, v * 0.5 * (1 + erf(v * 0.70710678)) -- followed
by the oracle's quantisers into planes padded as the calls pad them and by an fp32 consumer.  It must pass all three stage
checks at every shape of the GPU files' case tables (a reference that an honest fp32 chain cannot meet would be no yardstick),
and the float-stage bounds must leave it room: at the shapes added with this file at most 0.33 (attention; measured up to 0.27, the
peaked case) and 0.28 (MLP, activations up to +-50 included; measured up to 0.26) of the bound.  Those figures are measured on
this emulation, not on the kernels.  The nine older attention cases are held to the bound itself: `sos_wide` (q x 8) sits at 0.355.

The premises of the special cases are asserted here on the references alone: the peaked case, the all-keys-equal case, the
wide MLP case, the degenerate intervals."""
import numpy as np
import pytest
import torch

from oracle.ptq4vit_oracle import qmax_of
from tests import fused_reference as fr
from tests import test_hip_fused_attention as A
from tests import test_hip_fused_mlp as L

F32 = np.float32
ATTN_ROOM, MLP_ROOM = 0.33, 0.28
N_OLD_ATTN = A.IDS.index("sos_d128")          # the cases before it predate the stage references


def _rup(n, m):
    return (n + m - 1) // m * m


def _padded(planes, rows, cols):
    """[Z][M][N] (or [M][N]) integer planes as int8 in zeros of [Z][rows][cols]"""
    out = []
    for k in planes:
        p = np.zeros(k.shape[:-2] + (rows, cols), np.int8)
        p[..., :k.shape[-2], :k.shape[-1]] = k
        out.append(p)
    return out


# ---- attention -------------------------------------------------------------------------------------------------------------------
def _attn_intervals(case, q, kT, v):
    qa, qb = (qmax_of(b) for b in case.qk_bits)
    pb = qmax_of(case.pv_bits[1])
    H = q.shape[1]
    return dict(A1=A._headwise(q, (0, 2, 3), qa, A.HEAD_FACTORS["qA"]).reshape(H), B1=A._headwise(kT, (0, 2, 3), qb, A.HEAD_FACTORS["qB"]).reshape(H),
                B2=A._headwise(v, (0, 2, 3), pb, A.HEAD_FACTORS["pB"]).reshape(H))


def _emulate_attention(case, q, kT, v, iv, A2=None):
    """probs (fp32 torch), planes (padded int8), out (fp32) of the chain in fp32; A2: matmul2's head-wise A interval of a plain case"""
    B, H, M, N, D, Dv = case.shape
    (qa, qb), (pa, pb) = case.qk_bits, case.pv_bits
    scale = D ** -0.5
    qi, qn = fr.int_plane(q, iv["A1"].view(1, H, 1, 1).numpy(), -qmax_of(qa), qmax_of(qa) - 1)
    ki, kn = fr.int_plane(kT, iv["B1"].view(1, H, 1, 1).numpy(), -qmax_of(qb), qmax_of(qb) - 1)
    acc = torch.from_numpy(qi) @ torch.from_numpy(ki)
    s1 = (iv["A1"] * iv["B1"]).view(1, H, 1, 1)
    s1 = torch.where(torch.from_numpy(qn.any((0, 2, 3)) | kn.any((0, 2, 3))).view(1, H, 1, 1), torch.full_like(s1, float("nan")), s1)
    u = acc.float() * s1 * torch.tensor(scale, dtype=torch.float32)
    e = torch.exp(u - u.amax(-1, keepdim=True))
    probs = e / e.sum(-1, keepdim=True)
    if not case.twin and A2 is None:
        A2 = A._headwise(torch.nan_to_num(probs), (0, 2, 3), qmax_of(pa), A.HEAD_FACTORS["pA"]).reshape(H)
    pv = dict(sos=case.twin, A_bit=pa, split=F32(case.split), A_iv=F32(case.split) / F32(qmax_of(pa) - 1) if case.twin else A2)
    want, nan, grid = fr.attn_planes_of(probs, H, sos=pv["sos"], A_bit=pa, split=pv["split"], A_iv=pv["A_iv"])
    planes = _padded(want, _rup(M, 128), _rup(N, 64))
    vi, vn = fr.int_plane(v, iv["B2"].view(1, H, 1, 1).numpy(), -qmax_of(pb), qmax_of(pb) - 1)
    vi = torch.from_numpy(vi)
    b2 = torch.where(torch.from_numpy(vn.any((0, 2, 3))), torch.full_like(iv["B2"], float("nan")), iv["B2"]).view(1, H, 1, 1)
    pl = [torch.from_numpy(k.reshape(B, H, M, N).astype(np.int64)) for k in want]
    if case.twin:
        out = (pl[0] @ vi).float() * (torch.tensor(1.0 / (qmax_of(pa) - 1), dtype=torch.float32) * b2) + \
            (pl[1] @ vi).float() * (torch.tensor(float(pv["A_iv"])) * b2)
    else:
        out = (pl[0] @ vi).float() * (A2.view(1, H, 1, 1) * b2)
    return probs, planes, out, pv


def _attn_stages(case, q, kT, v, iv, skip_heads=(), A2=None):
    B, H, M, N, D, Dv = case.shape
    probs, planes, out, pv = _emulate_attention(case, q, kT, v, iv, A2)
    u64, p64 = fr.attn_float_stage(q, kT, iv["A1"], iv["B1"], *case.qk_bits, D ** -0.5)
    s1 = fr.check_probs(probs, u64, p64, case.name)
    want, nan, grid = fr.attn_planes_of(probs, H, **pv)
    assert fr.check_planes(planes, want, nan, grid, case.name) == int((~nan).sum()) * len(planes)
    ref = fr.attn_consumer_stage(planes, v, H, sos=case.twin, A_bit=case.pv_bits[0], B_bit=case.pv_bits[1], B_iv=iv["B2"], A_iv=pv["A_iv"], M=M, N=N)
    skip = np.zeros((1, H, 1, 1), bool)
    skip[0, list(skip_heads)] = True
    s3 = fr.check_out(out, ref, N, case.name, skip=skip)
    return dict(s1=s1, s3=s3, probs=probs, planes=planes, out=out, u64=u64, p64=p64, ref=ref)


_ATTN = {}


def _attn_run(case):
    if case.name not in _ATTN:
        q, kT, v = A._inputs(case, device="cpu")
        _ATTN[case.name] = _attn_stages(case, q, kT, v, _attn_intervals(case, q, kT, v))
    return _ATTN[case.name]


@pytest.mark.parametrize("case", A.CASES, ids=A.IDS)
def test_fp32_attention_chain_passes_the_three_stages(case):
    r = _attn_run(case)
    print(f"[fused reference] attention {case.name}: emulation at {r['s1']:.3f} of the probs bound, {r['s3']:.3f} of the out bar")
    assert r["s1"] <= (ATTN_ROOM if A.IDS.index(case.name) >= N_OLD_ATTN else 1.0) and r["s3"] <= 1.0


def test_a_wrong_probability_fails_stage_one():
    """the yardstick bites: one probability moved by its row's bound and a half, one M / N swap"""
    case = A.CASES[A.IDS.index("sos_m130_n64")]
    r = _attn_run(case)
    bad = r["probs"].clone()
    U = 10 + case.shape[3] / 64 + 5 * np.abs(r["u64"][0, 1, 7]).max()
    bad[0, 1, 7, 3] *= 1 + 1.5 * U * 2.0 ** -23
    with pytest.raises(AssertionError, match="of the bound"):
        fr.check_probs(bad, r["u64"], r["p64"], "moved")
    with pytest.raises(AssertionError):
        fr.check_probs(r["probs"].transpose(-2, -1), r["u64"], r["p64"], "swapped")
    planes = [p.copy() for p in r["planes"]]
    planes[0][1, 129, 63] += 1
    want, nan, grid = fr.attn_planes_of(r["probs"], 2, sos=True, A_bit=8, split=F32(case.split))
    with pytest.raises(AssertionError, match="bytes differ"):
        fr.check_planes(planes, want, nan, grid, "flipped")
    planes = [p.copy() for p in r["planes"]]
    planes[1][0, 130, 0] = 1
    with pytest.raises(AssertionError, match="padding rows"):
        fr.check_planes(planes, want, nan, grid, "padding")
    with pytest.raises(AssertionError, match="of 2e-6"):
        fr.check_out(r["out"] * (1 + 2e-5), r["ref"], case.shape[3], "scaled")


def test_premise_of_the_peaked_case():
    r = _attn_run(A.CASES[A.IDS.index("sos_peaked")])
    p64 = r["p64"]
    assert (p64 < fr.P_FLOOR).mean() >= 0.1, "at least 10 % of the entries below 2^-100"
    assert (p64.max(-1) > 0.999).mean() >= 0.1, "at least 10 % of the rows nearly one-hot"
    gap = (r["u64"].max(-1, keepdims=True) - r["u64"]).max()
    assert gap > 150.0, gap
    assert bool((r["probs"] == 0).any()), "the fp32 chain underflows to 0"


def test_premise_of_the_equal_keys_case():
    case = A.CASES[A.IDS.index("sos_keys_equal")]
    r = _attn_run(case)
    N = case.shape[3]
    assert (r["p64"] == 1.0 / N).all()
    assert torch.equal(r["probs"], torch.full_like(r["probs"], float(F32(1.0) / F32(N))))


@pytest.mark.parametrize("twin", [True, False], ids=["sos", "plain"])
@pytest.mark.parametrize("zero", ["q", "kT", "v"])
def test_premise_of_the_zero_heads(twin, zero):
    case = A.Case("degen", A.DEGEN_SHAPE, twin, (8, 8), (8, 8), 1.0, False)
    q, kT, v = A._degen_inputs(zero, device="cpu")
    iv = _attn_intervals(case, q, kT, v)
    key = {"q": "A1", "kT": "B1", "v": "B2"}[zero]
    assert float(iv[key][1]) == 0.0 and all(float(t[h]) > 0 for k, t in iv.items() for h in range(3) if (k, h) != (key, 1))
    A2 = torch.tensor([0.9, 1.1, 1.0]) / (qmax_of(8) - 0.5)
    r = _attn_stages(case, q, kT, v, iv, skip_heads=() if zero == "v" else (1,), A2=None if twin else A2)
    if zero == "v":
        assert np.isnan(r["ref"][:, 1]).all() and not np.isnan(r["ref"][:, [0, 2]]).any() and not np.isnan(r["p64"]).any()
    else:
        assert np.isnan(r["p64"][:, 1]).all() and not np.isnan(r["p64"][:, [0, 2]]).any()


# ---- MLP -------------------------------------------------------------------------------------------------------------------------
def _minmax_layers(case, xf=1.0):
    """x, fc1 / fc2 as dicts (weight, bias, w_iv [n_V], a_iv, w_bit, a_bit) on min-max intervals; the `wide` case: fc2's as the GPU
    file sets them"""
    g = torch.Generator().manual_seed(3000 + L.IDS.index(case.name))
    x = torch.randn(*case.rows, case.k_in, generator=g) * case.xf * xf
    dims = ((case.hidden, case.k_in), (L.N_OUT, case.hidden))
    layers = []
    for i, (n, k) in enumerate(dims):
        w = (torch.rand(n, k, generator=g) * 2 - 1) / k ** 0.5
        b = (torch.rand(n, generator=g) * 2 - 1) / k ** 0.5 if case.bias else None
        layers.append(dict(weight=w, bias=b, w_bit=case.bits[i][0], a_bit=case.bits[i][1], nV=case.nV[i]))
    h = torch.nn.functional.gelu(torch.nn.functional.linear(x, layers[0]["weight"], layers[0]["bias"]))
    for lay, inp, pos in ((layers[0], x, False), (layers[1], h, case.twin)):
        wq, aq = qmax_of(lay["w_bit"]), qmax_of(lay["a_bit"])
        lay["w_iv"] = lay["weight"].reshape(lay["nV"], -1).abs().amax(1) / (wq - 0.5)
        lay["a_iv"] = (inp.max() if pos else inp.abs().max()) / (aq - 0.5)
        lay["a_neg"] = F32(0.16997124254703522 / aq)
    if case.special == "wide":
        lay = layers[1]
        lay["a_iv"], lay["w_iv"] = L.wide_fc2_intervals(h, lay["weight"], qmax_of(lay["a_bit"]), qmax_of(lay["w_bit"]), lay["nV"])
    return x, layers[0], layers[1]


def _emulate_mlp(case, x, fc1, fc2):
    M = x.numel() // x.shape[-1]
    q1 = qmax_of(fc1["a_bit"])
    xi, xn = fr.int_plane(x.reshape(M, -1), F32(fc1["a_iv"]), -q1, q1 - 1)
    wi, wn, s = fr._weight_plane(fc1["weight"], fc1["w_iv"], fc1["w_bit"])
    acc = torch.from_numpy(xi) @ torch.from_numpy(wi).T
    s1 = fc1["a_iv"].float() * torch.from_numpy(s).view(1, -1)
    s1 = torch.where(torch.from_numpy(wn.any(-1)).view(1, -1), torch.full_like(s1, float("nan")), s1)
    v = acc.float() * s1
    if fc1["bias"] is not None:
        v = v + fc1["bias"]
    hidden = v * 0.5 * (1.0 + torch.erf(v * torch.tensor(0.70710678118654752440, dtype=torch.float32)))
    want, nan, grid = fr.mlp_planes_of(hidden, twin=case.twin, a_bit=fc2["a_bit"], a_iv=fc2["a_iv"], a_neg=fc2["a_neg"])
    planes = _padded(want, _rup(M, 128), _rup(case.hidden, 64))
    w2, _, s2 = fr._weight_plane(fc2["weight"], fc2["w_iv"], fc2["w_bit"])
    w2, s2 = torch.from_numpy(w2), torch.from_numpy(s2).view(1, -1)
    out = (torch.from_numpy(want[0].astype(np.int64)) @ w2.T).float() * (fc2["a_iv"].float() * s2)
    if case.twin:
        out = out + (torch.from_numpy(want[1].astype(np.int64)) @ w2.T).float() * (torch.tensor(float(fc2["a_neg"])) * s2)
    if fc2["bias"] is not None:
        out = out + fc2["bias"]
    return hidden, planes, out, want


def _mlp_stages(case, x, fc1, fc2, out_defined=True):
    M = x.numel() // x.shape[-1]
    hidden, planes, out, _ = _emulate_mlp(case, x, fc1, fc2)
    o64, v64, g64 = fr.mlp_float_stage(x, fc1["weight"], fc1["bias"], fc1["w_iv"], fc1["a_iv"], fc1["w_bit"], fc1["a_bit"])
    s1 = fr.check_hidden(hidden, o64, v64, g64, case.name)
    want, nan, grid = fr.mlp_planes_of(hidden, twin=case.twin, a_bit=fc2["a_bit"], a_iv=fc2["a_iv"], a_neg=fc2["a_neg"])
    assert fr.check_planes(planes, want, nan, grid, case.name) == int((~nan).sum()) * len(planes)
    s3 = 0.0
    if out_defined:
        ref = fr.mlp_consumer_stage(planes, fc2["weight"], fc2["bias"], fc2["w_iv"], fc2["w_bit"], twin=case.twin, a_iv=fc2["a_iv"],
                                    a_neg=fc2["a_neg"], M=M, hidden=case.hidden)
        s3 = fr.check_out(out.reshape(M, -1), ref, case.hidden, case.name)
    return dict(s1=s1, s3=s3, hidden=hidden, planes=planes, want=want, v64=v64, g64=g64, o64=o64)


@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_fp32_mlp_chain_passes_the_three_stages(case):
    r = _mlp_stages(case, *_minmax_layers(case))
    print(f"[fused reference] mlp {case.name}: emulation at {r['s1']:.3f} of E_g, {r['s3']:.3f} of the out bar")
    assert r["s1"] <= MLP_ROOM and r["s3"] <= 1.0


def test_premise_of_the_wide_mlp_case():
    case = L.CASES[L.IDS.index("twin_wide")]
    x, fc1, fc2 = _minmax_layers(case)
    r = _mlp_stages(case, x, fc1, fc2)
    q = qmax_of(fc2["a_bit"])
    g64 = r["g64"]
    want, _, _ = fr.mlp_planes_of(g64.astype(F32), twin=True, a_bit=fc2["a_bit"], a_iv=fc2["a_iv"], a_neg=fc2["a_neg"])
    assert want[0].min() == 0 and want[0].max() == q - 1 and want[1].min() == -q and want[1].max() == 0, "lo and hi on both reference planes"
    assert r["v64"].max() > 6.0 and r["v64"].min() < -6.0, "erff saturated on both sides"
    # ... and with activations up to +-50 the bound still leaves the fp32 chain its room
    r = _mlp_stages(case, *_minmax_layers(case, xf=3.0))
    assert np.abs(r["v64"]).max() > 50.0 and r["s1"] <= MLP_ROOM


def test_a_wrong_hidden_entry_fails_stage_one():
    case = L.CASES[L.IDS.index("twin_h198_nV3")]
    x, fc1, fc2 = _minmax_layers(case)
    r = _mlp_stages(case, x, fc1, fc2)
    bad = r["hidden"].clone().reshape(-1, case.hidden)
    E = 2.0 ** -24 * (3 * abs(r["o64"][5, 66]) + 12 * abs(r["v64"][5, 66])) + 2.0 ** -126
    bad[5, 66] += float(2.5 * E) + float(np.spacing(F32(abs(bad[5, 66]))))
    with pytest.raises(AssertionError, match="of E_g"):
        fr.check_hidden(bad, r["o64"], r["v64"], r["g64"], "moved")
    # the block edge one column off: column 66 on block 0's interval
    w_iv = fc1["w_iv"].clone()
    assert float(w_iv[0]) != float(w_iv[1])
    o64, v64, g64 = fr.mlp_float_stage(x, fc1["weight"], fc1["bias"], w_iv, fc1["a_iv"], fc1["w_bit"], fc1["a_bit"])
    shifted = r["hidden"].clone().reshape(-1, case.hidden)
    shifted[:, 66] = shifted[:, 66] * (w_iv[0] / w_iv[1])
    with pytest.raises(AssertionError, match="of E_g"):
        fr.check_hidden(shifted, o64, v64, g64, "edge")


@pytest.mark.parametrize("twin", [True, False], ids=["twin", "plain"])
def test_premise_of_the_zero_weight_block(twin):
    case = L.Case("degen", twin, L.W8A8, (2, 1), 200, True)
    fc1m, fc2m, x = L._degen_layers(twin, True, device="cpu")
    w_iv = fc1m.w_interval.reshape(-1)
    assert float(w_iv[1]) == 0.0 and float(w_iv[0]) > 0
    as_dict = lambda m: dict(weight=m.weight.detach(), bias=m.bias.detach(), w_iv=m.w_interval.reshape(-1), a_iv=m.a_interval.reshape(()),
                             w_bit=m.w_bit, a_bit=m.a_bit, nV=m.n_V, a_neg=getattr(m, "a_neg_interval", None))
    r = _mlp_stages(case, x, as_dict(fc1m), as_dict(fc2m), out_defined=False)
    assert np.isnan(r["g64"][:, 100:]).all() and not np.isnan(r["g64"][:, :100]).any()
