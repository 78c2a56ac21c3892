"""GPU: the cosine Linear search with weight column blocks / activation blocks (n_H, n_a > 1) -- k_pack_seg planes,
k_sweep_seg<false, EPI_COS>, k_finish_cos -- behind p4v_linear_calibrate, the granular entry points and p4v_calibrate_group.

Fixtures tests/golden/linblk_*.npz were made by running the reference's own classes (tools/gen_golden_linblk.py).  The bar for a
cosine table is tests/linblk_cases.py's: 32 ulp of the reference table's largest entry; a differing selection only where the
reference's own table has the two candidates within the same 32 ulp.
  1  the fused search (engine call with score tables, and the module) against the reference
  2  the granular chain = the fused call bit for bit; the tables of EVERY block (h > 0, a > 0 too) against the reference
  3  members of one p4v_calibrate_group call = the single calls, grouped launches
  4  the non-batching class PTQSLQuantLinear
  5  a shape beyond the fixtures (features cross a 128-row tile, samples cross two column tiles, cuts on k-tile boundaries)
     against the numpy oracle
  6  routes: the seg kernels with blocks, none of them without
  7  boundaries: post-GELU twin + cosine + blocks, K = 16384
  8  through the calibrators on the mini ViT: grouped and per module
"""
import copy
import json

import numpy as np
import pytest
import torch

from tests.helpers import assert_on_candidate_grid, candidate_grid, load_golden, record_margin
from tests.linblk_cases import (BATCHING, BEYOND, COS_BAR_ULP, NONBATCHING, as_columns, assert_cos_selection, assert_cos_table,
                                beyond_tensors, layer_params, table_ulp)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    return engine


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tensors(g):
    return dict(weight=_t(g["weight"]), bias=_t(g.get("bias")), x=_t(g["x"]), out=_t(g["out"]), grad=None)


def _module(g, cls=None):
    from ptq4vit_amd.quant_layers.linear import PTQSLBatchingQuantLinear, PTQSLQuantLinear
    p, oc, batching = layer_params(g)
    cls = cls or (PTQSLBatchingQuantLinear if batching else PTQSLQuantLinear)
    m = cls(g["x"].shape[-1], oc, bias="bias" in g, **p).cuda()
    m.weight.data = _t(g["weight"])
    if "bias" in g:
        m.bias.data = _t(g["bias"])
    m.raw_input, m.raw_out, m.raw_grad = _t(g["x"]), _t(g["out"]), None
    return m, p


def _ref_tables(g, p, r):
    """The reference's tables of round r: [column block h] (eq_n, n_V), [activation block a] (eq_n, 1)."""
    per = p["n_H"] + p["n_a"]
    tabs = [as_columns(t) for t in g["scores"][r * per:(r + 1) * per]]
    return tabs[:p["n_H"]], tabs[p["n_H"]:]


def _check_intervals(w_iv, a_iv, g, p, what):
    """Bit-identical, or one entry of the candidate table away -- further only where the reference's last table of that block ties
    within the bar (tests/helpers.py::assert_on_candidate_grid)."""
    wt, at = _ref_tables(g, p, p["search_round"] - 1)
    mult = candidate_grid(p["eq_alpha"], p["eq_beta"], p["eq_n"])
    w_ref = np.stack(wt, axis=-1).reshape(p["eq_n"], -1)            # column v * n_H + h: the order of w_interval (n_V, 1, n_H, 1)
    a_ref = np.concatenate(at, axis=1)                              # column a
    tie = lambda tab: COS_BAR_ULP * table_ulp(tab) / float(np.abs(tab).max())
    moved = assert_on_candidate_grid(np.asarray(w_iv), g["w_interval"], mult, what + " w_interval", max_steps=1, ref_scores=w_ref,
                                     tie_rtol=tie(w_ref))
    moved += assert_on_candidate_grid(np.asarray(a_iv), g["a_interval"], mult, what + " a_interval", max_steps=1, ref_scores=a_ref,
                                      tie_rtol=tie(a_ref))
    return moved


def _forward_close(got, g, what):
    got, ref = got.detach().cpu().numpy().astype(np.float64), g["quant_forward"].astype(np.float64)
    if got.shape != ref.shape:                                      # the larger fixture stores a corner of the output only
        got = got[:1, :8]
    assert got.shape == ref.shape, what
    err = np.abs(got - ref).max() / np.abs(ref).max()
    bar = 2e-6 * g["x"].shape[-1] ** 0.5                            # the project's bar for the int8 forward against the reference's
    record_margin("quant_forward_rel_err_over_bar", err / bar)
    assert err <= bar, f"{what}: quantised forward {err:.3e} > {bar:.3e}"


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BATCHING)
def test_fused_search_vs_reference(eng, name):
    g = load_golden(name)
    p, oc, _ = layer_params(g)
    w_iv, a_iv, scores, best = eng.linear_calibrate(want_scores=True, **_tensors(g), **p)
    torch.cuda.synchronize()
    scores, best = scores.cpu().numpy(), best.cpu().numpy()
    flips, worst = 0, 0.0
    for r in range(p["search_round"]):
        wt, at = _ref_tables(g, p, r)
        worst = max(worst, assert_cos_table(scores[r, 0], wt[0], what=f"{name}[round {r} w0]"),
                    assert_cos_table(scores[r, 1][:, :1], at[0], what=f"{name}[round {r} a0]"))
        flips += assert_cos_selection(best[r, 0], wt[0], what=f"{name}[round {r} w0]")
        flips += assert_cos_selection(best[r, 1][:1], at[0], what=f"{name}[round {r} a0]")
    moved = _check_intervals(w_iv.cpu().numpy(), a_iv.cpu().numpy(), g, p, name)
    print(f"[parity] {name}: tables within {worst:.1f} ulp, {flips} differing selections, {moved} intervals on another grid entry")


@pytest.mark.parametrize("name", BATCHING)
def test_module_vs_reference(eng, name):
    g = load_golden(name)
    m, p = _module(g)
    x = m.raw_input
    m.calibration_step2()
    assert m.calibrated and not hasattr(m, "raw_out")
    assert tuple(m.w_interval.shape) == g["w_interval"].shape and tuple(m.a_interval.shape) == g["a_interval"].shape
    moved = _check_intervals(m.w_interval.cpu().numpy(), m.a_interval.cpu().numpy(), g, p, name)
    m.mode = "quant_forward"
    with torch.no_grad():
        qf = m(x)
    if moved == 0:
        _forward_close(qf, g, name)


# ---- 2 ---------------------------------------------------------------------------------------------------------------
def _reference_layout_candidates(m):
    """linear.py:544-545: (eq_n + 1, n_V, 1, n_H, 1) and (n_a, 1, eq_n + 1), multipliers x the INITIAL intervals."""
    mult = torch.tensor(candidate_grid(m.eq_alpha, m.eq_beta, m.eq_n)).cuda()
    return mult.view(-1, 1, 1, 1, 1) * m.w_interval.unsqueeze(0), m.a_interval.unsqueeze(-1) * mult.view(1, 1, -1)


@pytest.mark.parametrize("name", BATCHING)
def test_granular_chain_equals_fused_call_and_every_block_table_vs_reference(eng, name):
    g = load_golden(name)
    fused, p = _module(g)
    fused.calibration_step2()
    m, _ = _module(g)
    m._initialize_intervals()
    w0, a0 = m.w_interval.clone(), m.a_interval.clone()
    wc, ac = _reference_layout_candidates(m)
    for _ in range(m.search_round):
        m._search_best_w_interval(wc)
        m._search_best_a_interval(ac)
    torch.cuda.synchronize()
    assert torch.equal(m.w_interval, fused.w_interval) and torch.equal(m.a_interval, fused.a_interval)
    # the same chain block by block: the table of every step against the reference's
    st = m._stepper()
    w, a = w0.reshape(-1), a0.reshape(-1)
    ac_major = ac.reshape(m.n_a, -1).t().contiguous()
    flips, worst = 0, 0.0
    for r in range(m.search_round):
        wt, at = _ref_tables(g, p, r)
        for h in range(m.n_H):
            w, s, b = st.search_w(wc, w, a, want_scores=True, block=h)
            worst = max(worst, assert_cos_table(s.cpu().numpy(), wt[h], what=f"{name}[round {r} w{h}]"))
            flips += assert_cos_selection(b.cpu().numpy(), wt[h], what=f"{name}[round {r} w{h}]")
        for k in range(m.n_a):
            a, s, b = st.search_a(ac_major, w, a, want_scores=True, block=k)
            worst = max(worst, assert_cos_table(s.cpu().numpy()[:, :1], at[k], what=f"{name}[round {r} a{k}]"))
            flips += assert_cos_selection(b.cpu().numpy()[:1], at[k], what=f"{name}[round {r} a{k}]")
    assert torch.equal(w, fused.w_interval.reshape(-1)) and torch.equal(a, fused.a_interval.reshape(-1))
    print(f"[granular] {name}: {m.search_round * (m.n_H + m.n_a)} tables within {worst:.1f} ulp, {flips} differing selections")
    if flips == 0:
        np.testing.assert_array_equal(w.cpu().numpy(), g["w_interval"].reshape(-1))
        np.testing.assert_array_equal(a.cpu().numpy(), g["a_interval"].reshape(-1))


# ---- 3 ---------------------------------------------------------------------------------------------------------------
def test_group_members_equal_the_single_calls(eng):
    def jobs():
        out = []
        for name in BATCHING:
            g = load_golden(name)
            out.append(eng.linear_job(**_tensors(g), **layer_params(g)[0]))
        g = load_golden("linear_blocks_nH2_na2")              # a difference-metric member next to them (fp32 candidate planes)
        p = dict(g["params"])
        p.pop("kind"); p.pop("oc")
        out.append(eng.linear_job(weight=_t(g["weight"]), bias=_t(g.get("bias")), x=_t(g["x"]), out=_t(g["out"]), grad=_t(g["grad"]), **p))
        return out
    single = [eng.run_job(j) for j in jobs()]
    torch.cuda.synchronize()
    eng.launch_counters(reset=True)
    grouped = eng.calibrate_group(jobs())
    torch.cuda.synchronize()
    cnt = eng.launch_counters(reset=True)
    for i, (a, b) in enumerate(zip(single, grouped)):
        for x, y in zip(a.outputs, b.outputs):
            assert torch.equal(x, y), f"member {i}: single {x.flatten()[:4].tolist()} vs grouped {y.flatten()[:4].tolist()}"
    assert cnt["groups"] == 1 and cnt["issued"] < cnt["asked"], cnt
    print(f"[group] launches asked for {cnt['asked']}, issued {cnt['issued']} in {cnt['rounds']} rounds")


# ---- 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NONBATCHING)
def test_nonbatching_module_vs_reference(eng, name, monkeypatch):
    g = load_golden(name)
    m, p = _module(g)
    seen = []
    orig = eng.linear_job

    def spy(**kw):
        job = orig(**dict(kw, want_scores=True))
        seen.append(job)
        return job

    monkeypatch.setattr(eng, "linear_job", spy)
    x = m.raw_input
    with torch.no_grad():
        qf = m.calibration_step2(x)
    torch.cuda.synchronize()
    assert m.calibrated and len(seen) == 1
    scores = seen[0].scores.cpu().numpy().astype(np.float64) / g["x"].shape[0]      # sum over the images of token means -> ONE mean
    best = seen[0].best.cpu().numpy()
    flips = 0
    for r in range(p["search_round"]):
        wt, at = _ref_tables(g, p, r)
        assert_cos_table(scores[r, 0], wt[0], what=f"{name}[round {r} w0]")
        assert_cos_table(scores[r, 1][:, :1], at[0], what=f"{name}[round {r} a0]")
        flips += assert_cos_selection(best[r, 0], wt[0], what=f"{name}[round {r} w0]")
        flips += assert_cos_selection(best[r, 1][:1], at[0], what=f"{name}[round {r} a0]")
    moved = _check_intervals(m.w_interval.cpu().numpy(), m.a_interval.cpu().numpy(), g, p, name)
    if moved == 0:
        _forward_close(qf, g, name)


# ---- 5 ---------------------------------------------------------------------------------------------------------------
def test_shape_beyond_the_fixtures_vs_oracle(eng):
    from oracle.ptq4vit_oracle import LinearOracle
    w, bias, x, out = beyond_tensors()
    hp = BEYOND["hp"]
    o = LinearOracle(w, bias, **hp)
    o.calibration_step2(x, out, None)
    common = dict(weight=_t(w), bias=_t(bias), x=_t(x), out=_t(out), grad=None)
    w_f, a_f, _, _ = eng.linear_calibrate(**common, **hp)
    st = eng.LinearStepper(**common, **{k: v for k, v in hp.items() if k not in ("eq_alpha", "eq_beta", "search_round")})
    wi, ai = st.init_intervals()
    mult = eng.candidate_multipliers(hp["eq_alpha"], hp["eq_beta"], hp["eq_n"], wi.device).view(-1, 1)
    wc, ac = mult * wi.reshape(1, -1), mult * ai.reshape(1, -1)
    flips, worst, i = 0, 0.0, 0
    for h in range(hp["n_H"]):
        wi, s, b = st.search_w(wc, wi, ai, want_scores=True, block=h)
        worst = max(worst, assert_cos_table(s.cpu().numpy(), o.trace[i][1], what=f"beyond[{o.trace[i][0]}]"))
        flips += assert_cos_selection(b.cpu().numpy(), o.trace[i][1], what=f"beyond[{o.trace[i][0]}]")
        i += 1
    for k in range(hp["n_a"]):
        ai, s, b = st.search_a(ac, wi, ai, want_scores=True, block=k)
        worst = max(worst, assert_cos_table(s.cpu().numpy()[:, :1], o.trace[i][1], what=f"beyond[{o.trace[i][0]}]"))
        flips += assert_cos_selection(b.cpu().numpy()[:1], o.trace[i][1], what=f"beyond[{o.trace[i][0]}]")
        i += 1
    torch.cuda.synchronize()
    assert i == len(o.trace)
    assert torch.equal(wi, w_f) and torch.equal(ai, a_f)
    print(f"[beyond] {i} tables within {worst:.1f} ulp of the oracle's, {flips} differing selections")
    if flips == 0:
        np.testing.assert_array_equal(w_f.cpu().numpy(), o.w_interval.reshape(-1))
        np.testing.assert_array_equal(a_f.cpu().numpy(), o.a_interval.reshape(-1))


# ---- 6 ---------------------------------------------------------------------------------------------------------------
def _counted(eng, run):
    eng.launch_counters(reset=True)
    eng.stats_reset()
    eng.stats_enable(True)
    try:
        run()
        torch.cuda.synchronize()
        recs = eng.stats_launches()
    finally:
        eng.stats_enable(False)
    return eng.launch_counters(reset=True), recs


def test_routes(eng):
    g = load_golden("linblk_cos_v2h2a3_w4a4")
    p, oc, _ = layer_params(g)
    steps = p["n_H"] + p["n_a"]
    S, K = g["x"].shape[0] * g["x"].shape[1], g["x"].shape[2]
    # (score tables requested: no pass memo, every step of every round runs)
    n2, r2 = _counted(eng, lambda: eng.linear_calibrate(want_scores=True, **_tensors(g), **p))
    n1, r1 = _counted(eng, lambda: eng.linear_calibrate(want_scores=True, **_tensors(g), **dict(p, search_round=1)))
    assert [r["kernel"] for r in r2] == ["k_sweep_seg"] * (2 * steps) and len(r1) == steps      # no k_sweep<float>, one sweep per step
    # the launch records carry the reference's GEMM of the step: samples x features x K MACs (two operations each) per candidate
    assert all(r["alg_ops"] == 2.0 * S * oc * K * p["eq_n"] and r["alg_bytes"] > 0 for r in r2), r2[0]
    # ... and a step is five launches: k_pack_seg of the fixed operand and of the candidate planes, the sweep, k_finish_cos, k_select
    assert n2["asked"] - n1["asked"] == 5 * steps, (n1, n2)
    # n_H = n_a = 1: no segment kernel
    g1 = load_golden("linear_cosine_w8a8")
    p1 = dict(g1["params"])
    p1.pop("kind"); p1.pop("oc")
    assert p1.get("n_H", 1) == 1 and p1.get("n_a", 1) == 1 and p1["metric"] == "cosine"
    _, recs = _counted(eng, lambda: eng.linear_calibrate(weight=_t(g1["weight"]), bias=_t(g1.get("bias")), x=_t(g1["x"]), out=_t(g1["out"]),
                                                         grad=None, **dict(p1, n_H=1, n_a=1)))
    assert recs and "k_sweep_seg" not in {r["kernel"] for r in recs}


# ---- 7 ---------------------------------------------------------------------------------------------------------------
def test_postgelu_twin_with_cosine_and_blocks_is_refused(eng):
    g = load_golden("linblk_cos_v2h2a3_w4a4")
    p, _, _ = layer_params(g)
    eng.launch_counters(reset=True)
    with pytest.raises(NotImplementedError, match="twin"):
        eng.linear_calibrate(postgelu=True, **_tensors(g), **p)
    assert eng.launch_counters()["asked"] == 0


def test_k_16384_is_refused(eng):
    K = 16384
    x = torch.zeros(1, 2, K, device="cuda")
    w = torch.zeros(4, K, device="cuda")
    eng.launch_counters(reset=True)
    with pytest.raises(NotImplementedError, match="K < 16384"):
        eng.linear_calibrate(weight=w, bias=None, x=x, out=torch.zeros(1, 2, 4, device="cuda"), grad=None, w_bit=4, a_bit=4,
                             metric="cosine", eq_alpha=0.5, eq_beta=1.2, eq_n=10, search_round=1, n_V=1, n_H=2, n_a=1)
    assert eng.launch_counters()["asked"] == 0


# ---- 8 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [True, False], ids=["hessian-calibrator-grouped", "quant-calibrator-per-module"])
def test_calibrators_with_blocked_cosine_linears(eng, monkeypatch, grouped):
    from ptq4vit_amd.configs import BasePTQ
    from ptq4vit_amd.quant_layers.linear import PTQSLBatchingQuantLinear
    from ptq4vit_amd.utils import models, net_wrap
    from ptq4vit_amd.utils.quant_calib import HessianQuantCalibrator, QuantCalibrator
    g = np.load("tests/golden/minivit_ptq4vit.npz", allow_pickle=False)
    kw = json.loads(str(g["model_kwargs"]))
    images = torch.from_numpy(g["images"]).cuda()
    monkeypatch.setitem(BasePTQ.ptqsl_linear_kwargs, "n_H", 2)
    monkeypatch.setitem(BasePTQ.ptqsl_linear_kwargs, "n_a", 2)
    monkeypatch.setenv("P4V_GROUPED", "1" if grouped else "0")
    net = models.get_net("vit_tiny_patch16_224", seed=0, device="cuda", **kw)
    wrapped = net_wrap.wrap_modules_in_net(net, BasePTQ)
    linears = {n: m for n, m in wrapped.items() if isinstance(m, PTQSLBatchingQuantLinear)}
    assert len(linears) >= 5 and all(m.metric == "cosine" and m.n_H == 2 and m.n_a == 2 for m in linears.values())
    fresh = {n: copy.deepcopy(m) for n, m in linears.items()}
    caps = {}
    for n, m in linears.items():
        def rec(_o=m.calibration_job, _m=m, _n=n):
            caps[_n] = (_m.raw_input.clone(), _m.raw_out.clone())
            return _o()
        m.calibration_job = rec

    class Loader:
        batch_size = images.shape[0]

        def __iter__(self):
            yield images, torch.zeros(images.shape[0], dtype=torch.long)

    eng.launch_counters(reset=True)
    if grouped:
        HessianQuantCalibrator(net, wrapped, Loader(), sequential=False, batch_size=4).batching_quant_calib()
    else:
        QuantCalibrator(net, wrapped, Loader(), sequential=False).batching_quant_calib()
    torch.cuda.synchronize()
    cnt = eng.launch_counters(reset=True)
    assert (cnt["groups"] >= 1) == grouped, cnt
    assert set(caps) == set(linears)
    for n, m in linears.items():
        assert m.calibrated and tuple(m.w_interval.shape) == (m.n_V, 1, 2, 1) and tuple(m.a_interval.shape) == (2, 1), n
        alone = fresh[n]
        alone.raw_input, alone.raw_out = caps[n]
        alone.raw_grad = None
        alone.calibration_step2()
        assert torch.equal(alone.w_interval, m.w_interval) and torch.equal(alone.a_interval, m.a_interval), n
    with torch.no_grad():
        assert torch.isfinite(net(images)).all()      # every module now runs in quant_forward mode
