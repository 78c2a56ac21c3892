"""GPU: the caller-workspace contract of the C ABI (include/ptq4vit_hip.h, Conventions) as a C caller meets it -- d_workspace of
EXACTLY *_workspace_bytes(desc), aligned to the documented minimum and no more, holding arbitrary bytes on entry.

Every other GPU test reaches the library through engine.workspace(), which pads the size by 5 % + 1 MiB, hands the padded size to
the library and keeps the buffer between calls: an under-reported size, a store past the last carved buffer and a read of scratch
nobody wrote in this call all go unseen.  Here engine.workspace is replaced by tests/workspace_guard.py::Guard (exact, guarded,
minimally aligned, poisoned before every call) and the universal assertion is

    the guarded / exact / poisoned call returns the SAME BITS as the ordinary call on the same inputs,

for two poisons of the view (0xFF: NaN as fp32, -1 as int8 / int32, "set" as a flag byte; 0x00), with both guards intact and,
for an arena, the slack between the members' exact needs untouched.  Bit-identity holds because the kernels are deterministic and
no plan may depend on the buffer.  The poison is applied before EVERY call, the granular calls of a stepper included: the header
gives no entry point the right to find an earlier call's data.

Part B (the arena gap, p4v_debug_set_arena_gap + p4v_debug_arena_ranges): the end guards see only the last carved buffer.  With
unused bytes behind every allocation and the record of every range a call's allocations ever covered, every byte outside those
ranges must still hold the poison, and the results must not move.  The gap is 4096 (the slack *_workspace_bytes adds), raised per
case to 1/50 of the case's plain size where that is more: the condition that the unallocated share is >= 1 % of the workspace
keeps the test from checking nothing (at least one gap of the call's largest pass can never be covered by another pass's buffers,
and 1/50 of the plain size is >= 1 % of the size with up to ~50 gaps in it).

What the runs measured is written to the file $P4V_WORKSPACE_OUT names, when it is set (committed as
profiles/r17_workspace_contract.json): per case the size, the highest touched offset under each poison, their ratio, the
unallocated share with the gap on, the counts of guard / slack / unallocated bytes found changed."""
import contextlib
import io
import json
import os
import time

import numpy as np
import pytest
import torch

from tests import search_round_cases, sweep_plan_cases
from tests.helpers import load_golden
from tests.workspace_guard import Guard, summarise

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x00)
_REF = {}          # case id -> the ordinary call's results, computed once and left unchanged
_PROFILE = {}


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    yield engine
    engine.debug_arena_gap(0)
    engine.release_workspace()
    path = os.environ.get("P4V_WORKSPACE_OUT")
    if _PROFILE and path:
        path = os.path.abspath(path)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        old = {}
        if os.path.exists(path):
            try:
                old = json.load(open(path))
            except Exception:      # noqa: BLE001
                old = {}
        old.update(_PROFILE)
        with open(path, "w") as fh:
            json.dump(dict(sorted(old.items())), fh, indent=1)


@pytest.fixture(autouse=True)
def _nothing_more_on_the_gpu_after_a_fault():
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:      # noqa: BLE001
        pytest.exit(f"the GPU reported an error, the session ends here: {e}", returncode=3)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(ts):
    torch.cuda.synchronize()
    return [t.detach().clone() for t in ts if t is not None]


def _assert_same_bits(got, ref, what):
    assert len(got) == len(ref), f"{what}: {len(got)} result tensors vs {len(ref)}"
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}[{i}]: {a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}"
        ia, ib = (a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)) if a.dtype == torch.float32 else (a, b)
        n = int((ia != ib).sum())
        assert n == 0, f"{what}[{i}]: {n} of {a.numel()} values differ from the ordinary call's, e.g. {a.flatten()[:4].tolist()} vs {b.flatten()[:4].tolist()}"


def _reference(eng, cid, fn):
    if cid not in _REF:
        eng.release_workspace()
        _REF[cid] = _bits(fn(eng))
    return _REF[cid]


def _gap_for(need):
    return max(4096, (need // 50 + 255) // 256 * 256)


def _check_case(eng, monkeypatch, cid, fn, *, gap=True, arena=False):
    """The ordinary call, the guarded call under both poisons, and (gap) the guarded call with the arena gap on."""
    ref = _reference(eng, cid, fn)
    row = _PROFILE.setdefault(cid, {})
    need = 0
    for poison in POISONS:
        with Guard(eng, monkeypatch, poison) as g:
            got = _bits(fn(eng))
            reps = g.finish()
        s = summarise(reps)
        row[f"poison_{poison:02x}"] = s
        need = s["need"]
        print(f"[workspace] {cid} poison {poison:#04x}: {s}")
        assert s["calls"] >= 1 and s["touched"] > 0, f"{cid}: the guard saw no engine call"
        assert s["touched"] <= s["need"]
        assert s["guard_changed"] == 0, f"{cid} poison {poison:#04x}: {s['guard_changed']} guard bytes changed ({reps})"
        assert s["slack_changed"] == 0, f"{cid} poison {poison:#04x}: {s['slack_changed']} bytes of the arena's slack changed ({reps})"
        if arena:
            assert any("slack_bytes" in r for r in reps), f"{cid}: no arena was carved"
        _assert_same_bits(got, ref, f"{cid} poison {poison:#04x}")
    row["need"] = need
    row["touched_over_need"] = max(row[f"poison_{p:02x}"]["touched"] for p in POISONS) / need
    if not gap:
        return
    gp = _gap_for(need)
    try:
        eng.debug_arena_gap(gp)
        with Guard(eng, monkeypatch, POISONS[0], gap=gp) as g:
            got = _bits(fn(eng))
            reps = g.finish()
    finally:
        eng.debug_arena_gap(0)
    s = summarise(reps)
    row["gap"] = dict(s, gap=gp)
    print(f"[workspace] {cid} gap {gp}: {s}")
    assert s["need"] >= need
    assert s["guard_changed"] == 0, f"{cid} gap: {s['guard_changed']} guard bytes changed ({reps})"
    assert s["unalloc_changed"] == 0, f"{cid} gap: {s['unalloc_changed']} bytes outside every allocation changed ({reps})"
    assert s.get("unalloc_share_min", 0.0) >= 0.01, f"{cid} gap: unallocated share {s.get('unalloc_share_min')} < 1 % ({reps})"
    _assert_same_bits(got, ref, f"{cid} gap {gp}")


# ---- 1, 2: the smallest calibration per sweep kernel family and per path of the round drivers ---------------------------------------
@pytest.mark.parametrize("name,run,pruned", sweep_plan_cases.CASES, ids=[c[0] for c in sweep_plan_cases.CASES])
def test_sweep_plan_cases_on_an_exact_poisoned_workspace(eng, monkeypatch, name, run, pruned):
    _check_case(eng, monkeypatch, f"sweep/{name}", lambda e: run(e, pruned))


@pytest.mark.parametrize("mode", search_round_cases.MODES)
@pytest.mark.parametrize("name,run", search_round_cases.CASES, ids=[c[0] for c in search_round_cases.CASES])
def test_search_round_cases_on_an_exact_poisoned_workspace(eng, monkeypatch, name, run, mode):
    def fn(e):
        intervals, tables = run(e, mode)
        return intervals + tables
    _check_case(eng, monkeypatch, f"rounds/{name}/{mode}", fn)


# ---- 3: the reference's own layers at a pruning-eligible size (788 samples), default call ----------------------------------------------
def _prune_fixture(name):
    g = load_golden(name)
    p = dict(g["params"])
    kind = p.pop("kind")
    if kind == "linear":
        p.pop("oc")
        args = dict(weight=_t(g["weight"]), bias=_t(g["bias"]), x=_t(g["x"]), out=_t(g["out"]), grad=_t(g["grad"]), n_H=1, n_a=1, **p)
        return lambda e: e.linear_calibrate(**args)
    sos = p["sos"]
    B = torch.from_numpy(np.ascontiguousarray(g["B"]))
    Bd = B.cuda() if sos else B.transpose(-2, -1).contiguous().cuda().transpose(-2, -1)       # q.k^T: a transposed view
    args = dict(A=_t(g["A"]), B=Bd, out=_t(g["out"]), grad=_t(g["grad"]), **p)
    return lambda e: e.matmul_calibrate(**args)


@pytest.mark.parametrize("name", ["prune_linear_qkv_hessian_w8a8", "prune_postgelu_hessian_w8a8", "prune_matmul_qk_hessian_w8a8",
                                  "prune_matmul_sos_hessian_w8a8"])
def test_pruned_default_call_on_an_exact_poisoned_workspace(eng, monkeypatch, name):
    """The three-stage passes and the run-time slice choice (a value read back from the device: the sizing run cannot know it)."""
    call = _prune_fixture(name)
    staged = []

    def fn(e):
        e.prune_counters(reset=True)
        res = call(e)
        torch.cuda.synchronize()
        staged.append(e.prune_counters(reset=True)["staged"])
        return res
    _check_case(eng, monkeypatch, f"prune/{name}", fn)
    assert len(staged) >= 4 and all(n > 0 for n in staged), f"{name}: staged passes per call {staged} -- the pruning did not engage"


def test_two_tier_and_cross_checked_passes_on_an_exact_poisoned_workspace(eng, monkeypatch):
    """Beyond the issue's list: the four fixtures above leave stage B2 little to do, so the candidate planes kept across the stages of
    a pass (the plane cache at the top of the arena and its per-candidate `done` flags) are hardly read there.  The qkv-like layer
    of tests/test_hip_production_path.py::test_two_tier_pruning_is_exact_and_engages_on_a_spread_weight_profile (16 x 197 samples,
    metric weight spread over the samples: many survivors, second slice tier, stage B2 over the survivors), by the default call and
    under the engine's cross-check (variant 134217728: every pruned pass followed by the full sweep of the same pass -- one of the
    places where the real run does more than the sizing run can see)."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(31)
    b, T, K, N = 16, 197, 768, 2304
    x = torch.randn(b, T, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.02 * torch.linspace(0.5, 2.0, N)[:, None]
    bias = torch.randn(N, generator=g) * 0.02
    out = F.linear(x, w, bias)
    grad = torch.randn(out.shape, generator=g) * 1e-10 * torch.exp(1.1 * torch.randn(b, T, 1, generator=g))
    args = dict(weight=w.cuda(), bias=bias.cuda(), x=x.cuda(), out=out.cuda(), grad=grad.cuda(), w_bit=8, a_bit=8, n_V=3, n_H=1, n_a=1,
                metric="hessian", eq_alpha=0.01, eq_beta=1.2, eq_n=100, search_round=3)
    staged = []

    def fn(e):
        e.prune_counters(reset=True)
        two = e.linear_calibrate(**args)
        torch.cuda.synchronize()
        staged.append(e.prune_counters(reset=True))
        try:
            e.debug_variant(134217728)
            chk = e.linear_calibrate(**args)
            torch.cuda.synchronize()
        finally:
            e.debug_variant(0)
        return list(two[:2]) + list(chk[:2])
    _check_case(eng, monkeypatch, "prune/two_tier_spread_weight", fn)
    assert all(c["staged"] > c["staged_no_survivors"] for c in staged), f"no pass with survivors for stage B2: {staged}"
    ref = _REF["prune/two_tier_spread_weight"]
    assert torch.equal(ref[0], ref[2]) and torch.equal(ref[1], ref[3])


# ---- 4: quant_forward, the workspace sized by the bit-2 query ------------------------------------------------------------------------
def _linear_forward(name):
    def fn(e):
        g = load_golden(name)
        p = g["params"]
        return [e.linear_quant_forward(weight=_t(g["weight"]), bias=_t(g["bias"]) if "bias" in g else None, x=_t(g["x"]),
                                       w_interval=_t(g["w_interval"]), a_interval=_t(g["a_interval"]), w_bit=p["w_bit"], a_bit=p["a_bit"],
                                       n_V=p["n_V"], n_H=p.get("n_H", 1), n_a=p.get("n_a", 1), postgelu=p["postgelu"])]
    return fn


def _matmul_forward(name):
    def fn(e):
        g = load_golden(name)
        p = g["params"]
        return [e.matmul_quant_forward(A=_t(g["A"]), B=_t(g["B"]), A_interval=_t(np.asarray(g["A_interval"])), B_interval=_t(g["B_interval"]),
                                       split=_t(np.asarray(g["split"])) if p["sos"] else None, A_bit=p["A_bit"], B_bit=p["B_bit"], sos=p["sos"])]
    return fn


def _mmblk_forward(name):
    def fn(e):
        g = load_golden(name)
        p = g["params"]
        blocks = (p.get("n_V_A", 1), p.get("n_H_A", 1), p.get("n_V_B", 1), p.get("n_H_B", 1))
        return [e.matmul_blocks_quant_forward(A=_t(g["A"]), B=_t(g["B"]), A_interval=_t(np.asarray(g["A_interval"])),
                                              B_interval=_t(np.asarray(g["B_interval"])), split=None, A_bit=p["A_bit"], B_bit=p["B_bit"],
                                              blocks=blocks)]
    return fn


FORWARD = [("linear_qkv_hessian_w8a8", _linear_forward), ("postgelu_hessian_w8a8", _linear_forward), ("linear_blocks_nH2_na2", _linear_forward),
           ("matmul_qk_hessian_w8a8", _matmul_forward), ("matmul_sos_hessian_w8a8", _matmul_forward),
           ("mmblk_qk_hessian_vA2hA2_vB2hB3", _mmblk_forward)]


@pytest.mark.parametrize("name,make", FORWARD, ids=[f[0] for f in FORWARD])
def test_quant_forward_on_an_exact_poisoned_workspace(eng, monkeypatch, name, make):
    _check_case(eng, monkeypatch, f"forward/{name}", make(name))


# ---- 5: the granular steppers: init, one search per side, the poison renewed before every call ---------------------------------------
def _cands(e, p, iv):
    return e.candidate_multipliers(p["eq_alpha"], p["eq_beta"], p["eq_n"], iv.device).view(-1, 1) * iv.reshape(1, -1)


def _linear_stepper(e):
    g = load_golden("linear_qkv_hessian_w8a8")
    p = g["params"]
    st = e.LinearStepper(weight=_t(g["weight"]), bias=_t(g["bias"]), x=_t(g["x"]), out=_t(g["out"]), grad=_t(g["grad"]), w_bit=p["w_bit"],
                         a_bit=p["a_bit"], metric=p["metric"], eq_n=p["eq_n"], n_V=p["n_V"], n_H=1, n_a=1, postgelu=p["postgelu"])
    w, a = st.init_intervals()
    w2, sw, bw = st.search_w(_cands(e, p, w), w, a, want_scores=True)
    a2, sa, ba = st.search_a(_cands(e, p, a), w2, a, want_scores=True)
    return [w, a, w2, sw, bw, a2, sa, ba]


def _matmul_stepper(name):
    def fn(e):
        g = load_golden(name)
        p = g["params"]
        sos = p["sos"]
        st = e.MatMulStepper(A=_t(g["A"]), B=_t(g["B"]), out=_t(g["out"]), grad=_t(g["grad"]), A_bit=p["A_bit"], B_bit=p["B_bit"],
                             metric=p["metric"], eq_n=p["eq_n"], sos=sos)
        A_iv, B_iv = st.init_intervals()
        if sos:
            split, A2, s1, b1 = st.search_split(want_scores=True)
        else:
            split = None
            A2, s1, b1 = st.search_A(_cands(e, p, A_iv), A_iv, B_iv, want_scores=True)
        B2, s2, b2 = st.search_B(_cands(e, p, B_iv), A2, B_iv, split=split, want_scores=True)
        return [A_iv, B_iv, split, A2, s1, b1, B2, s2, b2]
    return fn


def _mmblk_stepper(e):
    g = load_golden("mmblk_qk_hessian_vA2hA2_vB2hB3")
    p = g["params"]
    blocks = (p["n_V_A"], p["n_H_A"], p["n_V_B"], p["n_H_B"])
    st = e.MatMulStepper(A=_t(g["A"]), B=_t(g["B"]), out=_t(g["out"]), grad=_t(g["grad"]), A_bit=p["A_bit"], B_bit=p["B_bit"],
                         metric=p["metric"], eq_n=p["eq_n"], blocks=blocks)
    A_iv, B_iv = st.init_intervals()
    H = st.H
    A2, s1, b1 = st.search_block("A", 1, 1, _cands(e, p, A_iv.view(H, -1)[:, 3]), A_iv, B_iv, want_scores=True)
    B2, s2, b2 = st.search_block("B", 1, 2, _cands(e, p, B_iv.view(H, -1)[:, 5]), A2, B_iv, want_scores=True)
    return [A_iv, B_iv, A2, s1, b1, B2, s2, b2]


def _conv_stepper(e):
    g = load_golden("conv_channelwise_hessian_a8_overlap")
    p = g["params"]
    st = e.ConvStepper(weight=_t(g["weight"]), bias=_t(g["bias"]), x=_t(g["x"]), out=_t(g["out"]), grad=_t(g["grad"]),
                       stride=(p["stride"], p["stride"]), padding=(0, 0), dilation=(1, 1), w_bit=p["w_bit"], a_bit=p["a_bit"],
                       metric=p["metric"], eq_n=p["eq_n"], channelwise=p["channelwise"])
    w, a = st.init_intervals()
    w2, sw, bw = st.search_w(_cands(e, p, w), w, a, want_scores=True)
    a2, sa, ba = st.search_a(_cands(e, p, a), w2, a, want_scores=True)
    return [w, a, w2, sw, bw, a2, sa, ba]


STEPPERS = [("linear", _linear_stepper), ("matmul_qk", _matmul_stepper("matmul_qk_hessian_w8a8")),
            ("matmul_sos", _matmul_stepper("matmul_sos_hessian_w8a8")), ("mmblk", _mmblk_stepper), ("conv", _conv_stepper)]


@pytest.mark.parametrize("name,fn", STEPPERS, ids=[s[0] for s in STEPPERS])
def test_granular_calls_on_an_exact_workspace_poisoned_before_every_call(eng, monkeypatch, name, fn):
    """The header gives the granular calls no carry-over: everything a search call needs arrives through its arguments, so the
    workspace is poisoned again before EVERY call of the sequence (workspace_guard wraps the steppers' call helpers)."""
    _check_case(eng, monkeypatch, f"stepper/{name}", fn)
    assert _PROFILE[f"stepper/{name}"]["poison_ff"]["calls"] >= 3


# ---- 6: a padded, dilated, rectangular conv; one operand on each quantiser -----------------------------------------------------------
def _convgeo(e):
    g = load_golden("convgeo_a_cw_hessian_a8_rect_dil")
    p = dict(g["params"])
    p.pop("kind")
    geo = {k: tuple(p.pop(k)) for k in ("stride", "padding", "dilation")}
    cw = p.pop("channelwise")
    ten = dict(weight=_t(g["weight"]), bias=_t(g["bias"]), x=_t(g["x"]), out=_t(g["out"]), grad=_t(g["grad"]))
    return list(e.conv_calibrate(**ten, **geo, channelwise=cw, **p)) + list(e.conv_calibrate(**ten, **geo, channelwise=cw, want_scores=True, **p))


def _mixbit(e):
    g = load_golden("mixbit_linear_w8a4_l2_v3")
    p = dict(g["params"])
    p.pop("kind"); p.pop("oc")
    ten = dict(weight=_t(g["weight"]), bias=_t(g["bias"]), x=_t(g["x"]), out=_t(g["out"]), grad=None, n_H=1, n_a=1)
    return list(e.linear_calibrate(**ten, **p)) + list(e.linear_calibrate(**ten, want_scores=True, **p))


@pytest.mark.parametrize("name,fn", [("convgeo_a_cw_hessian_a8_rect_dil", _convgeo), ("mixbit_linear_w8a4_l2_v3", _mixbit)],
                         ids=["convgeo_a_cw_hessian_a8_rect_dil", "mixbit_linear_w8a4_l2_v3"])
def test_further_fixtures_on_an_exact_poisoned_workspace(eng, monkeypatch, name, fn):
    _check_case(eng, monkeypatch, f"fixture/{name}", fn)


# ---- 7: inputs whose data pointers are only 4-byte aligned ---------------------------------------------------------------------------
def _one_float_in(t):
    """`t` as a contiguous view one float into a larger flat buffer: engine passes it through unchanged"""
    flat = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


MISALIGNED = {"linear_k1024_n64": dict(K=1024, N=64, seed=3), "postgelu_k1024_n64": dict(K=1024, N=64, seed=4, postgelu=True),
              "linear_k192_n128": dict(K=192, N=128, seed=1)}


def _sweep_kernels(eng, call):
    """kernel family of every sweep launch of `call()`, in launch order"""
    eng.stats_reset()
    eng.stats_enable(True)
    try:
        call()
        torch.cuda.synchronize()
        eng.stats_get()
        return [r["kernel"] for r in eng.stats_launches()]
    finally:
        eng.stats_enable(False)


@pytest.mark.parametrize("name", list(MISALIGNED))
def test_inputs_aligned_to_four_bytes_on_an_exact_poisoned_workspace(eng, monkeypatch, name):
    """The sizing run sees no pointers and plans k_sweep7 as if raw_out / the metric weight were 16-byte aligned; the real call
    checks and takes another kernel.  *_workspace_bytes must cover both.  Reference: the same misaligned call, ordinary workspace.
    Asserted for the K = 1024 layers: the aligned call runs on k_sweep7 and the misaligned one does not -- the real plan did part
    from the sizing plan.  (K = 192 runs on k_sweep6, which has no alignment predicate: same plan, the case pins that it stays so.)"""
    kw = dict(MISALIGNED[name])
    postgelu = kw.get("postgelu", False)

    def call(e, place):
        w, b, x, out, grad = sweep_plan_cases.linear_inputs(**kw)
        return e.linear_calibrate(weight=place(w), bias=b.cuda(), x=place(x), out=place(out), grad=place(grad),
                                  w_bit=8, a_bit=8, metric="hessian", n_V=1, n_H=1, n_a=1, postgelu=postgelu, prune=False, want_scores=True,
                                  **sweep_plan_cases.SEARCH)
    aligned = _sweep_kernels(eng, lambda: call(eng, lambda t: t.cuda()))
    misaligned = _sweep_kernels(eng, lambda: call(eng, _one_float_in))
    print(f"[workspace] misaligned/{name}: aligned {aligned}, misaligned {misaligned}")
    assert aligned and misaligned
    if kw["K"] >= 1024:
        assert any(k.startswith("k_sweep7") for k in aligned), aligned
        assert not any(k.startswith("k_sweep7") for k in misaligned), misaligned
    else:
        assert misaligned == aligned
    _check_case(eng, monkeypatch, f"misaligned/{name}", lambda e: call(e, _one_float_in))
    _PROFILE[f"misaligned/{name}"]["kernels"] = dict(aligned=aligned, misaligned=misaligned)


# ---- 8: the 12-member mixture as ONE group call: exact needs, no pad, the slack between the members poisoned --------------------------
def test_group_mixture_in_an_exact_poisoned_arena(eng, monkeypatch):
    from tests.test_hip_group import _jobs, _mixture
    specs = _mixture(eng)
    assert len(specs) == 12

    def fn(e):
        e.launch_counters(reset=True)
        jobs = e.calibrate_group(_jobs(e, specs))
        torch.cuda.synchronize()
        assert e.launch_counters(reset=True)["groups"] == 1
        return [t for j in jobs for t in j.outputs]
    # (the arena ranges are per calling thread and the members run on the library's threads: no gap run)
    _check_case(eng, monkeypatch, "group/mixture12", fn, gap=False, arena=True)


# ---- 9: one whole calibration on the grouped path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("group_calls", [None, 3], ids=["default-one-call", "three-concurrent-calls"])
def test_whole_deit_tiny_calibration_in_exact_poisoned_arenas(eng, monkeypatch, group_calls):
    """DeiT-tiny/224, PTQ4ViT configuration, 4 images, the calibrator's grouped search.  Every interval bit-identical to the
    unpatched calibration.
    default-one-call: what the calibrator does by itself at this size -- under 512 MiB of captured tensors it makes ONE
    p4v_calibrate_group call on the calling thread (asserted: one group, one arena).
    three-concurrent-calls: `group_calls = 3`, the path of the larger networks -- three p4v_calibrate_group calls at a time from three
    worker threads, each on its own side stream and its own exact, guarded, poisoned arena (asserted: >= 2 groups and >= 2 distinct
    (stream, slot) buffers), the guard's per-stream keying and the library's per-thread state under concurrent callers."""
    from ptq4vit_amd.configs import PTQ4ViT
    from ptq4vit_amd.utils import models, net_wrap
    from ptq4vit_amd.utils.quant_calib import HessianQuantCalibrator
    from tests.test_hip_production_path import _intervals
    torch.cuda.empty_cache()
    eng.release_workspace()
    net = models.get_net("deit_tiny_patch16_224", seed=0, device="cuda")
    with contextlib.redirect_stdout(io.StringIO()):
        wrapped = net_wrap.wrap_modules_in_net(net, PTQ4ViT)
    images = torch.randn(4, 3, 224, 224, generator=torch.Generator().manual_seed(0)).cuda()

    class Loader:
        batch_size = 4

        def __iter__(self):
            yield images, None

    def calibrate():
        for m in wrapped.values():
            m.mode = "raw"
        eng.launch_counters(reset=True)
        t0 = time.perf_counter()
        cal = HessianQuantCalibrator(net, wrapped, Loader(), sequential=False, batch_size=4)
        if group_calls:
            cal.search_grouped, cal.group_calls = True, group_calls
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            cal.batching_quant_calib()
        torch.cuda.synchronize()
        return _intervals(wrapped), eng.launch_counters(reset=True), time.perf_counter() - t0

    calibrate()                                           # (warm-up: module loading, torch's pool)
    ref, cnt, t_ref = calibrate()
    assert cnt["groups"] == (group_calls or 1), cnt
    row = _PROFILE.setdefault(f"network/deit_tiny_x4/{group_calls or 1}_group_calls", {"seconds_unpatched": t_ref, "groups": cnt["groups"]})
    for poison in POISONS:
        with Guard(eng, monkeypatch, poison) as g:
            calibrate()                                   # (the guarded buffers are allocated here; every call is checked all the same)
            got, cnt_g, t_g = calibrate()
            reps = g.finish()
        s = summarise(reps)
        buffers = {(r["stream"], r["slot"]) for r in reps}
        row[f"poison_{poison:02x}"] = dict(s, seconds=t_g, buffers=len(buffers))
        print(f"[workspace] DeiT-tiny x 4, {cnt['groups']} group calls, poison {poison:#04x}: {t_g:.3f} s guarded vs {t_ref:.3f} s unpatched; "
              f"{len(buffers)} buffers; {s}")
        assert cnt_g["groups"] == cnt["groups"] and s["calls"] >= 2 * cnt["groups"]
        assert len(buffers) == cnt["groups"] and all(slot == "arena" for _, slot in buffers), buffers
        if group_calls:
            assert cnt_g["groups"] >= 2 and len(buffers) >= 2
        assert all("slack_bytes" in r for r in reps)
        assert s["guard_changed"] == 0 and s["slack_changed"] == 0, reps
        n = 0
        for name in ref:
            assert len(ref[name]) == len(got[name])
            for a, b in zip(ref[name], got[name]):
                assert torch.equal(a, b), f"{name}: unpatched {a.flatten()[:4].tolist()} vs guarded {b.flatten()[:4].tolist()}"
                n += a.numel()
        assert n >= 100
    del net, wrapped, images
    torch.cuda.empty_cache()


# ---- 10: a declared size that is too small ----------------------------------------------------------------------------------------
def _small_linear(e):
    w, b, x, out, grad = sweep_plan_cases.linear_inputs(192, 128, seed=1)
    return e.linear_job(weight=w.cuda(), bias=b.cuda(), x=x.cuda(), out=out.cuda(), grad=grad.cuda(), w_bit=8, a_bit=8, metric="hessian",
                        n_V=1, n_H=1, n_a=1, **sweep_plan_cases.SEARCH)


def _small_matmul(e):
    A, B, out, grad = sweep_plan_cases.matmul_inputs(49, 64, 49, seed=7)
    return e.matmul_job(A=A.cuda(), B=B.cuda(), out=out.cuda(), grad=grad.cuda(), A_bit=8, B_bit=8, metric="hessian", **sweep_plan_cases.SEARCH)


def _small_conv(e):
    w, b, x, out, grad = sweep_plan_cases.conv_inputs(seed=10)
    return e.conv_job(weight=w.cuda(), bias=b.cuda(), x=x.cuda(), out=out.cuda(), grad=grad.cuda(), stride=(16, 16), padding=(0, 0),
                      dilation=(1, 1), w_bit=8, a_bit=32, metric="hessian", **sweep_plan_cases.SEARCH)


@pytest.mark.parametrize("name,make", [("linear", _small_linear), ("matmul", _small_matmul), ("conv", _small_conv)],
                         ids=["linear", "matmul", "conv"])
def test_a_declared_size_that_is_too_small_is_refused_and_harmless(eng, monkeypatch, name, make):
    """workspace_bytes = need // 2 on a pointer whose allocation holds the full size plus the guards (only the DECLARED size is
    wrong: a missing host check cannot leave allocated memory): P4V_ERR_WORKSPACE with a message, both guards intact, nothing
    stored past the declared size, and the next call on the same thread with the proper size gives the reference bits."""
    from ptq4vit_amd import _lib
    ref = _bits(eng.run_job(make(eng)).outputs)
    with Guard(eng, monkeypatch, 0xFF, declare=lambda n: n // 2) as g:
        with pytest.raises(RuntimeError, match=r"\(code -3\)"):
            eng.run_job(make(eng))
        assert _lib.load().p4v_last_error(), "P4V_ERR_WORKSPACE without a message"
        reps = g.finish()
        assert len(reps) == 1 and reps[0]["declared"] == reps[0]["need"] // 2
        assert reps[0]["guard_changed"] == 0, reps
        assert reps[0]["touched"] <= reps[0]["declared"], f"the refused call stored past the declared size: {reps}"
        g.declare = None
        got = _bits(eng.run_job(make(eng)).outputs)
        reps = g.finish()
        assert reps[-1]["declared"] == reps[-1]["need"] and reps[-1]["guard_changed"] == 0, reps
    _assert_same_bits(got, ref, f"{name}: the call after the refused one")
    _PROFILE[f"too_small/{name}"] = dict(need=reps[0]["need"], declared=reps[0]["declared"], touched_by_refused_call=reps[0]["touched"],
                                         guard_changed=reps[0]["guard_changed"])
