"""GPU: the fused int8 MLP forward (p4v_mlp_quant_forward, engine.mlp_quant_forward, utils/fuse.py).

fc1's int8 GEMM ends in the exact GELU and fc2's activation quantiser and writes fc2's int8 row plane(s); fc2 is the unfused
forward sweep on those planes.  What is held here, per case, on a poisoned workspace of exactly the size asked for:

1. quantiser and layout: the planes the call left are, byte for byte and padding included, what k_pack_dual (twin) / the
   single-plane packer (plain fc2) makes of the call's OWN fp32 hidden tensor; padding rows are zero;
2. fc2 from planes: `out` is fc2.quant_forward(hidden), bit for bit;
3. GELU: hidden against torch's gelu(fc1.quant_forward(x)) in fp32 ulps -- expected 0 (both sides call ROCm's erff), asserted
   <= 32 (twice the 16-ulp bound OpenCL C gives erf, which both implementations are built to);
4. against the unfused chain: a plane byte may differ from the unfused one by one grid step only, and only where the unfused
   t = g / s lies within (U + 1) * 2^-23 * max(|t|, 1) of a half-integer (U: the ulp distance measured in 3);
5. the contract: exact workspace, one byte less refused with no launch, n_a = 2 / n_H = 2 refused with no launch, null hidden;
6. module level on the mini ViT: fuse_mlp's names, logits fused vs unfused, raw / hooked states fall back bit-identically, a
   second calibration of the fused net gives the unfused net's intervals, unfuse_mlp restores.

7. the float64 stage references (tests/fused_reference.py; their own test: tests/test_fused_reference_cpu.py), on every case:
   hidden against the float64 GELU of the exact integer product of the oracle's quantisers on the RAW x and W1
   (|hidden - g64| <= 2^-24 (3 |o64| + 12 |v64|) + 2^-126); the planes against the oracle's twin_planes / quant_int of the call's
   own hidden tensor on the CPU, exactly; `out` against the int64 GEMM of the call's own planes with quant_int(W2), each twin
   plane on its own scale, in float64, at the int8-forward bar 2e-6 sqrt(K).  1, 2 and 3 compare with this library's other
   kernels, which are pinned to the oracle at their own tests' shapes only; 7 has no kernel of the library in it;
8. a degenerate interval (fc1 n_V = 2, its second weight row block zero under the min-max rule), next to the same call on the
   healthy weight: hidden NaN in exactly those columns and bit-identical elsewhere, plane bytes on the grid there and
   byte-identical elsewhere; `out` is not compared (a NaN hidden entry has no defined byte).

Shapes (the smallest that reach every edge): 2 x 197 = 394 rows (three full 128-row tiles and a ragged one), in_features 96
(one and a half k-tiles), hidden 200 (ragged against the 128 tile and Kp = 256; with fc1 n_V = 2 the block edge at 100 falls
inside a wave's 32 columns) and 256, out_features 72; 1 x 5 rows (a single ragged row tile), 2 x 128 rows (no padding row),
in_features 48, 64 and 192 (below one k-tile, exactly one, three), hidden 72 and 128 (below the 128 tile, exactly one), hidden 198
with fc1 n_V = 3 and fc2 n_V = 1 (blocks of 66 columns: the edges at 66 and 132 inside a wave's 32); fc1 W4A8 with fc2 W8A4,
fc2 a_bit = 2 (q - 1 = 1) twin and plain; x x 12 with fc2's intervals set, not searched (|v| beyond 6 on both sides: erff saturated on
both sides; both clamp ends of both twin planes reached -- asserted on the CPU quantiser's planes).  Plane 2 of every twin case is
asserted non-zero next to plane 1.

With P4V_FUSED_MLP_OUT set the measured margins are written there, under "mlp" (profiles/r24_fused_edges_margins.json; the seven
older cases alone: profiles/r20_fused_mlp_margins.json).
"""
import copy
import json
import os
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import fused_reference as fr
from tests.fused_common import _Loader, _count_fused_calls, _intervals, _wrapped_of, merge_margins, ulp_distance
from tests.workspace_guard import Guard

pytestmark = pytest.mark.gpu

ROWS, K_IN, N_OUT = (2, 197), 96, 72
ULP_BAR = 32
_MARGINS = {}

W8A8 = ((8, 8), (8, 8))
Case = namedtuple("Case", "name twin bits nV hidden bias rows k_in xf special", defaults=(ROWS, K_IN, 1.0, None))
#               id                    twin   (w, a) bits of fc1, fc2  nV of fc1, fc2  hidden bias  rows      in_features  x factor  special
CASES = [Case("twin_w8a8",            True,  W8A8,                    (1, 1),         200,   True),
         Case("twin_w6a6",            True,  ((6, 6), (6, 6)),        (1, 1),         200,   True),
         Case("plain_w8a8",           False, W8A8,                    (1, 1),         200,   True),
         Case("twin_w8a8_nV2",        True,  W8A8,                    (2, 2),         200,   True),
         Case("plain_w6a6_nV2",       False, ((6, 6), (6, 6)),        (2, 2),         200,   True),
         Case("twin_w8a8_nobias",     True,  W8A8,                    (1, 1),         200,   False),
         Case("twin_w8a8_h256",       True,  W8A8,                    (2, 2),         256,   True),
         # rows: one ragged row tile; an exact multiple of 128
         Case("twin_rows5",           True,  W8A8,                    (1, 1),         200,   True, (1, 5)),
         Case("twin_rows256",         True,  W8A8,                    (1, 1),         200,   True, (2, 128)),
         # in_features below one k-tile, exactly one, three
         Case("twin_in48",            True,  W8A8,                    (1, 1),         200,   True, ROWS,     48),
         Case("plain_in64",           False, W8A8,                    (1, 1),         200,   True, ROWS,     64),
         Case("twin_in192",           True,  W8A8,                    (1, 1),         200,   True, ROWS,     192),
         # hidden below the 128 tile, exactly one tile; three fc1 blocks of 66 columns: the edges at 66 and 132 inside a wave's 32
         Case("twin_h72",             True,  W8A8,                    (1, 1),         72,    True),
         Case("plain_h128",           False, W8A8,                    (1, 1),         128,   True),
         Case("twin_h198_nV3",        True,  W8A8,                    (3, 1),         198,   True),
         # w_bit != a_bit, fc1 and fc2 of different widths, q - 1 = 1 on fc2's activation
         Case("twin_w4a8_w8a4",       True,  ((4, 8), (8, 4)),        (1, 1),         200,   True),
         Case("twin_fc2_a2",          True,  ((8, 8), (8, 2)),        (1, 1),         200,   True),
         Case("plain_fc2_a2",         False, ((8, 8), (8, 2)),        (1, 1),         200,   True),
         # erff saturated on both sides; fc2's intervals set so that both clamp ends of both planes are reached
         Case("twin_wide",            True,  W8A8,                    (1, 1),         200,   True, ROWS,     K_IN,        12.0,     "wide")]
IDS = [c[0] for c in CASES]


def wide_fc2_intervals(h, W2, a_qmax, w_qmax, nV):
    """fc2's intervals of the `wide` case, set and not searched: the positive range a quarter of the largest activation (the
    upper quarter clamps at q - 1), min-max weights.  (a_interval, w_interval [n_V])"""
    return h.max() / (4.0 * (a_qmax - 0.5)), W2.reshape(nV, -1).abs().amax(1) / (w_qmax - 0.5)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    yield engine
    engine.release_workspace()
    merge_margins(os.environ.get("P4V_FUSED_MLP_OUT"), "mlp", _MARGINS, IDS)


def _modules(case):
    """fc1 / fc2 of one case, calibrated by a real calibration_step2 on seeded normal data; and the input."""
    from ptq4vit_amd.quant_layers.linear import PostGeluPTQSLBatchingQuantLinear, PTQSLBatchingQuantLinear
    name, twin, bits, nV, hidden, bias = case[:6]
    torch.manual_seed(1000 + IDS.index(name))
    kw = [dict(w_bit=bits[i][0], a_bit=bits[i][1], metric="L2_norm", search_round=2, eq_alpha=0.01, eq_beta=1.2, eq_n=40, n_V=nV[i], n_H=1,
               n_a=1) for i in (0, 1)]
    fc1 = PTQSLBatchingQuantLinear(case.k_in, hidden, bias=bias, **kw[0]).cuda()
    fc2 = (PostGeluPTQSLBatchingQuantLinear if twin else PTQSLBatchingQuantLinear)(hidden, N_OUT, bias=bias, **kw[1]).cuda()
    x = torch.randn(*case.rows, case.k_in, device="cuda") * case.xf
    with torch.no_grad():
        for fc, inp in ((fc1, x), (fc2, F.gelu(F.linear(x, fc1.weight, fc1.bias)))):
            if case.special == "wide" and fc is fc2:
                a_iv, w_iv = wide_fc2_intervals(inp, fc.weight, fc.a_qmax, fc.w_qmax, fc.n_V)
                fc.w_interval = w_iv.view(fc.n_V, 1, 1, 1)
                fc._set_a_interval(a_iv.view(1, 1))
                fc.calibrated = True
            else:
                fc.raw_input, fc.raw_out, fc.raw_grad = inp, F.linear(inp, fc.weight, fc.bias), None
                fc.calibration_step2()
            fc.mode = "quant_forward"
    return fc1, fc2, x


_RUNS = {}


def run_case(eng, monkeypatch, case):
    """One fused call per case (exact, guarded, poisoned workspace) and the unfused chain next to it; shared by the tests."""
    name = case[0]
    if name in _RUNS:
        return _RUNS[name]
    from ptq4vit_amd.utils.fuse import _layer
    fc1, fc2, x = _modules(case)
    with torch.no_grad():
        with Guard(eng, monkeypatch, 0xCD) as g:
            out, hidden, planes = eng.mlp_quant_forward(x=x, fc1=_layer(fc1), fc2=_layer(fc2), want_hidden=True, want_planes=True)
            reps = g.finish()
        assert len(reps) == 1 and reps[0]["guard_changed"] == 0 and 0 < reps[0]["touched"] <= reps[0]["need"], reps
        v_ref = fc1.quant_forward(x)
        h_ref = F.gelu(v_ref)
        out_ref = fc2.quant_forward(h_ref)
    r = dict(fc1=fc1, fc2=fc2, x=x, out=out, hidden=hidden, planes=planes, h_ref=h_ref, out_ref=out_ref, need=reps[0]["need"], twin=case.twin)
    _RUNS[name] = r
    return r


def _unfused_planes(eng, case, fc2, h):
    """fc2's row plane(s) as the unfused forward packs them from the fp32 tensor `h`: (padded planes [M][Kp])."""
    twin = case[1]
    h2 = h.reshape(-1, h.shape[-1])
    q = fc2.a_qmax
    a_iv = fc2._positive_a_interval().reshape(-1)
    if twin:
        _, _, p1, p2 = eng.debug_pack_dual(h2, sos=False, scale=float(a_iv[0]), lo=-q, hi=q - 1, qmax=q, const_scale=fc2.a_neg_interval)
        return p1, p2
    _, p1 = eng.pack_plane_i8(h2, mode="sym", scales=a_iv, rows_per_scale=h2.shape[0], lo=-q, hi=q - 1)
    return (p1,)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_planes_are_the_packers_bytes_of_the_calls_own_hidden(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    M, hidden = r["x"].shape[0] * r["x"].shape[1], case[4]
    want = _unfused_planes(eng, case, r["fc2"], r["hidden"])
    assert len(want) == len(r["planes"]) == (2 if case[1] else 1)
    for got, ref in zip(r["planes"], want):
        assert got.shape[0] % 128 == 0 and got.shape[0] >= M and got.shape[1] == ref.shape[1] == (hidden + 63) // 64 * 64
        assert torch.equal(got[:M], ref), f"{case[0]}: {(got[:M] != ref).sum().item()} bytes differ from the packer's"
        assert not got[M:].any(), "padding rows must be zero"
        assert not got[:, hidden:].any(), "padding columns must be zero"
    assert r["planes"][0].any() and (not case[1] or r["planes"][1].any())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_out_is_fc2_quant_forward_of_the_calls_own_hidden(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    with torch.no_grad():
        want = r["fc2"].quant_forward(r["hidden"])
    assert r["out"].shape == want.shape == (*case.rows, N_OUT)
    assert torch.equal(r["out"], want), f"{case[0]}: max |diff| {(r['out'] - want).abs().max().item():.3e}"


def _measured_ulps(r):
    return int(ulp_distance(r["hidden"], r["h_ref"]).max())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gelu_matches_torch_on_fc1_quant_forward(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    assert torch.isfinite(r["hidden"]).all()
    U = _measured_ulps(r)
    print(f"[fused mlp] {case[0]}: hidden vs torch gelu(fc1.quant_forward(x)): max {U} ulp")
    _MARGINS.setdefault("gelu_max_ulp", {})[case[0]] = U
    assert U <= ULP_BAR, f"{case[0]}: {U} ulp"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_planes_against_the_unfused_chain(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    U = _measured_ulps(r)
    fc2 = r["fc2"]
    M = r["x"].shape[0] * r["x"].shape[1]
    hidden = case[4]
    scales = [float(fc2._positive_a_interval().reshape(-1)[0])] + ([float(np.float32(fc2.a_neg_interval))] if case[1] else [])
    h = r["h_ref"].reshape(M, hidden).double()
    flips = 0
    for got, ref, s in zip(r["planes"], _unfused_planes(eng, case, fc2, r["h_ref"]), scales):
        a, b = got[:M, :hidden].to(torch.int32), ref[:, :hidden].to(torch.int32)
        diff = a != b
        if diff.any():
            t = h / s
            near = ((t - torch.floor(t) - 0.5).abs() <= (U + 1) * 2.0 ** -23 * t.abs().clamp(min=1.0))
            assert ((a - b).abs()[diff] == 1).all(), f"{case[0]}: a byte differs by more than one grid step"
            assert near[diff].all(), f"{case[0]}: {(diff & ~near).sum().item()} bytes differ away from a rounding tie"
        flips += int(diff.sum())
    print(f"[fused mlp] {case[0]}: {flips} plane bytes differ from the unfused chain's (U = {U})")
    _MARGINS.setdefault("plane_bytes_differing_from_unfused", {})[case[0]] = flips
    with torch.no_grad():
        rel = ((r["out"] - r["out_ref"]).norm() / r["out_ref"].norm()).item()
    _MARGINS.setdefault("out_rel_diff_vs_unfused", {})[case[0]] = rel
    if flips == 0:
        assert torch.equal(r["out"], r["out_ref"])


# ---- the float64 stage references (tests/fused_reference.py) ----------------------------------------------------------------------
def _neg(fc2):
    return getattr(fc2, "a_neg_interval", None)


def _check_stages(r, what, out_defined=True):
    """The three stage checks on one call's hidden, planes and out; returns the ratios.  `out_defined`: False when a plane holds
    undefined bytes (NaN hidden entries) -- every output sums over them, `out` is not compared."""
    fc1, fc2, twin = r["fc1"], r["fc2"], r["twin"]
    M, hidden = r["hidden"].numel() // r["hidden"].shape[-1], r["hidden"].shape[-1]
    if "stage1" not in r:
        r["stage1"] = fr.mlp_float_stage(r["x"], fc1.weight, fc1.bias, fc1.w_interval, fc1.a_interval, fc1.w_bit, fc1.a_bit)
    s1 = fr.check_hidden(r["hidden"], *r["stage1"], what)
    a_iv = fc2._positive_a_interval()
    want, nan, grid = fr.mlp_planes_of(r["hidden"], twin=twin, a_bit=fc2.a_bit, a_iv=a_iv, a_neg=_neg(fc2))
    n = fr.check_planes(r["planes"], want, nan, grid, what)
    got = dict(hidden_over_bound=s1, plane_bytes_compared=n)
    if out_defined:
        ref = fr.mlp_consumer_stage(r["planes"], fc2.weight, fc2.bias, fc2.w_interval, fc2.w_bit, twin=twin, a_iv=a_iv, a_neg=_neg(fc2),
                                    M=M, hidden=hidden)
        got["out_over_bar"] = fr.check_out(r["out"].reshape(M, -1), ref, hidden, what)
    return got, want


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stages_against_the_float64_references(eng, monkeypatch, case):
    r = run_case(eng, monkeypatch, case)
    got, want = _check_stages(r, case.name)
    print(f"[fused mlp] {case.name}: |hidden - g64| / E_g {got['hidden_over_bound']:.3f}; {got['plane_bytes_compared']} plane bytes exact; "
          f"|out - ref| / bar {got['out_over_bar']:.3f}")
    _MARGINS.setdefault("stage_ratios", {})[case.name] = got
    assert got["plane_bytes_compared"] == r["hidden"].numel() * len(r["planes"])
    if case.special == "wide":                       # the premise: both clamp ends of both planes, and a saturated erff on both sides
        q = r["fc2"].a_qmax
        assert want[0].min() == 0 and want[0].max() == q - 1 and want[1].min() == -q and want[1].max() == 0
        v64 = r["stage1"][1]
        assert v64.max() > 6.0 and v64.min() < -6.0


# ---- degenerate intervals: a weight row block of zeros under the min-max rule -----------------------------------------------------------
def _degen_run(eng, monkeypatch, twin, zero):
    """fc1 with n_V = 2 on min-max intervals, its second row block zeroed (`zero`) or healthy; fc2's intervals are those of the
    healthy hidden tensor in both runs."""
    key = ("degen", twin, zero)
    if key in _RUNS:
        return _RUNS[key]
    from ptq4vit_amd.utils.fuse import _layer
    fc1, fc2, x = _degen_layers(twin, zero)
    with torch.no_grad():
        with Guard(eng, monkeypatch, 0xCD) as g:
            out, hid, planes = eng.mlp_quant_forward(x=x, fc1=_layer(fc1), fc2=_layer(fc2), want_hidden=True, want_planes=True)
            reps = g.finish()
    assert len(reps) == 1 and reps[0]["guard_changed"] == 0 and 0 < reps[0]["touched"] <= reps[0]["need"], reps
    r = dict(fc1=fc1, fc2=fc2, x=x, out=out, hidden=hid, planes=planes, twin=twin)
    _RUNS[key] = r
    return r


def _degen_layers(twin, zero, device="cuda"):
    from ptq4vit_amd.quant_layers.linear import PostGeluPTQSLBatchingQuantLinear, PTQSLBatchingQuantLinear
    hidden = 200
    torch.manual_seed(1090)
    kw = dict(w_bit=8, a_bit=8, metric="L2_norm", search_round=1, eq_alpha=0.01, eq_beta=1.2, eq_n=40, n_H=1, n_a=1)
    fc1 = PTQSLBatchingQuantLinear(K_IN, hidden, bias=True, n_V=2, **kw).to(device)
    fc2 = (PostGeluPTQSLBatchingQuantLinear if twin else PTQSLBatchingQuantLinear)(hidden, N_OUT, bias=True, n_V=1, **kw).to(device)
    x = torch.randn(*ROWS, K_IN, device=device)
    with torch.no_grad():
        h = F.gelu(F.linear(x, fc1.weight, fc1.bias))
        if zero:
            fc1.weight[hidden // 2:] = 0.0
        fc1.w_interval = (fc1.weight.reshape(2, -1).abs().amax(1) / (fc1.w_qmax - 0.5)).view(2, 1, 1, 1)
        fc1._set_a_interval((x.abs().max() / (fc1.a_qmax - 0.5)).view(1, 1))
        fc2.w_interval = (fc2.weight.abs().max() / (fc2.w_qmax - 0.5)).view(1, 1, 1, 1)
        fc2._set_a_interval(((h.max() if twin else h.abs().max()) / (fc2.a_qmax - 0.5)).view(1, 1))
        for fc in (fc1, fc2):
            fc.calibrated, fc.mode = True, "quant_forward"
    return fc1, fc2, x


@pytest.mark.parametrize("twin", [True, False], ids=["twin", "plain"])
def test_a_zero_weight_block_poisons_its_columns_alone(eng, monkeypatch, twin):
    """Departs from the reference, whose fake-quantised weight rows are NaN and whose hidden ROWS are NaN with them after fc2
    only: here the hidden tensor is NaN in the block's columns, and the planes hold grid bytes there."""
    bad, good = _degen_run(eng, monkeypatch, twin, True), _degen_run(eng, monkeypatch, twin, False)
    half = bad["hidden"].shape[-1] // 2
    w_iv = bad["fc1"].w_interval.reshape(-1)
    assert float(w_iv[1]) == 0.0 and float(w_iv[0]) > 0 and float(w_iv[0]) == float(good["fc1"].w_interval.reshape(-1)[0])
    assert torch.isnan(bad["hidden"][..., half:]).all() and torch.isfinite(bad["hidden"][..., :half]).all()
    assert torch.equal(bad["hidden"][..., :half], good["hidden"][..., :half])
    what = f"zero fc1 weight block, {'twin' if twin else 'plain'}"
    got, _ = _check_stages(bad, what, out_defined=False)       # (NaN columns: bytes on the grid; the others the CPU quantiser's)
    _check_stages(good, what + " (healthy)")
    _MARGINS.setdefault("degenerate", {})[what] = got
    M = bad["hidden"].numel() // bad["hidden"].shape[-1]
    for a, b in zip(bad["planes"], good["planes"]):
        assert torch.equal(a[:M, :half], b[:M, :half])


# ---- 5: the contract ------------------------------------------------------------------------------------------------------------
def test_workspace_contract_and_envelope(eng, monkeypatch):
    from ptq4vit_amd.utils.fuse import _layer
    case = CASES[0]
    r = run_case(eng, monkeypatch, case)          # (the exact, guarded, poisoned call)
    fc1, fc2, x = r["fc1"], r["fc2"], r["x"]
    torch.cuda.synchronize()
    with torch.no_grad():
        # one byte less: refused, nothing launched
        before = eng.launch_counters()
        with Guard(eng, monkeypatch, 0xCD, declare=lambda n: n - 1) as g:
            with pytest.raises(RuntimeError, match="workspace too small"):
                eng.mlp_quant_forward(x=x, fc1=_layer(fc1), fc2=_layer(fc2))
            reps = g.finish()
        assert eng.launch_counters() == before
        assert all(rep["touched"] == 0 and rep["guard_changed"] == 0 for rep in reps), reps
        # outside the envelope: refused before any launch
        for key in ("n_a", "n_H"):
            for which in (0, 1):
                layers = [_layer(fc1), _layer(fc2)]
                layers[which][key] = 2
                with pytest.raises(NotImplementedError, match="n_H = n_a = 1"):
                    eng.mlp_quant_forward(x=x, fc1=layers[0], fc2=layers[1])
        assert eng.launch_counters() == before
        # no hidden tensor asked for: the same out
        out = eng.mlp_quant_forward(x=x, fc1=_layer(fc1), fc2=_layer(fc2))
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


def test_fused_net_logits_and_fallbacks(eng, mini, monkeypatch):
    from ptq4vit_amd.utils import fuse, models
    net, wrapped, images = mini
    mlps = [n for n, m in net.named_modules() if isinstance(m, models.Mlp)]
    assert len(mlps) == 2
    calls = _count_fused_calls(eng, monkeypatch, "mlp_quant_forward")
    cls_forward = models.Mlp.forward
    try:
        with torch.no_grad():
            y_u = net(images)
            assert not calls
            assert fuse.fuse_mlp(net) == mlps
            assert fuse.fuse_mlp(net) == mlps                      # idempotent
            y_f = net(images)
            assert len(calls) == len(mlps), "the fused path did not run"
            for m in wrapped.values():
                m.mode = "raw"
            y_raw = net(images)
            assert len(calls) == len(mlps), "raw mode must take the original forward"
            for m in wrapped.values():
                m.mode = "quant_forward"
            assert torch.equal(y_f.argmax(-1), y_u.argmax(-1))
            ratio = ((y_f - y_u).norm() / (y_u - y_raw).norm()).item()
            print(f"[fused mlp] mini ViT: |fused - unfused| / |unfused - raw| = {ratio:.3e}")
            _MARGINS["minivit_fused_over_quant_error"] = ratio
            assert ratio <= 1e-2

            mods = dict(net.named_modules())
            probe = torch.randn(4, 17, mods[mlps[0]].fc1.in_features, device="cuda")

            def unfused_twin(fn):
                """fn() on the fused net, then on the same net unfused, in whatever state it is in"""
                a = fn()
                fuse.unfuse_mlp(net)
                b = fn()
                fuse.fuse_mlp(net)
                return a, b

            # one fc2 in raw mode: that MLP takes the original forward -- the net and the MLP itself as on the unfused net
            mods[mlps[0]].fc2.mode = "raw"
            del calls[:]
            y_a, y_b = unfused_twin(lambda: net(images))
            assert len(calls) == len(mlps) - 1
            assert torch.equal(y_a, y_b)
            del calls[:]
            m_a, m_b = unfused_twin(lambda: mods[mlps[0]](probe))
            assert not calls and torch.equal(m_a, m_b)
            mods[mlps[0]].fc2.mode = "quant_forward"

            # a forward hook on fc1: it fires, that MLP takes the original forward, the output is the unfused net's
            fired = []
            h = mods[mlps[0]].fc1.register_forward_hook(lambda mod, inp, out: fired.append(tuple(out.shape)))
            del calls[:]
            y_a, y_b = unfused_twin(lambda: net(images))
            assert len(fired) == 2 and len(calls) == len(mlps) - 1
            assert torch.equal(y_a, y_b)
            del calls[:]
            m_a, m_b = unfused_twin(lambda: mods[mlps[0]](probe))
            assert not calls and torch.equal(m_a, m_b)
            h.remove()
            # ... a pre-hook on the activation likewise
            h = mods[mlps[1]].act.register_forward_pre_hook(lambda mod, inp: fired.append("act"))
            del calls[:]
            m_a, m_b = unfused_twin(lambda: mods[mlps[1]](probe))
            assert not calls and fired[-1] == "act" and torch.equal(m_a, m_b)
            h.remove()
            # autograd recording: the original forward
            del calls[:]
            with torch.enable_grad():
                mods[mlps[0]](probe.clone().requires_grad_(True))
            assert not calls
            # everything back: fused again, and deterministic
            del calls[:]
            assert torch.equal(net(images), y_f) and len(calls) == len(mlps)
    finally:
        fuse.unfuse_mlp(net)
    # unfuse_mlp restores the original forward
    for n in mlps:
        m = dict(net.named_modules())[n]
        assert "forward" not in m.__dict__ and m.forward.__func__ is cls_forward
    assert fuse.unfuse_mlp(net) == []
    with torch.no_grad():
        del calls[:]
        assert torch.equal(net(images), y_u) and not calls


def test_second_calibration_of_a_fused_net_gives_the_unfused_intervals(eng, mini, monkeypatch):
    from ptq4vit_amd.utils import fuse
    from ptq4vit_amd.utils.quant_calib import HessianQuantCalibrator
    net, wrapped, images = mini
    fuse.unfuse_mlp(net)
    net_u = copy.deepcopy(net)
    wrapped_u = _wrapped_of(net_u, wrapped)
    net_f = copy.deepcopy(net)
    wrapped_f = _wrapped_of(net_f, wrapped)
    assert len(fuse.fuse_mlp(net_f)) == 2
    HessianQuantCalibrator(net_u, wrapped_u, _Loader(images), sequential=False, batch_size=4).batching_quant_calib()
    HessianQuantCalibrator(net_f, wrapped_f, _Loader(images), sequential=False, batch_size=4).batching_quant_calib()
    iu, ifu = _intervals(wrapped_u), _intervals(wrapped_f)
    assert iu.keys() == ifu.keys() and len(iu) >= len(wrapped)
    for k in iu:
        assert torch.equal(iu[k], ifu[k]), k
    # ... and the fused net is still fused, and runs fused
    calls = _count_fused_calls(eng, monkeypatch, "mlp_quant_forward")
    with torch.no_grad():
        net_f(images)
    assert len(calls) == 2
