"""GPU: blocks whose initial min-max interval is 0 or negative, on the Linear and MatMul searches and their int8 forward.

SURVEY.md App. A-10: a block that is all zero has interval 0, fake-quantises as 0 / 0, and the reference's score column of it is
NaN in every table -- argmax takes candidate 0, and every search that multiplies through the block is NaN too.  An int8 plane
cannot hold a NaN and `0 * dot + bias` is finite, so the engine has to put the NaN back where the scales are formed (DESIGN.md
s1, "Zero and negative intervals on the int8 paths").  A negative interval (the post-GELU twin's signed maximum of an input
that is negative throughout) is legal arithmetic and gives finite tables.

  a  the reference's own degenerate runs (tests/golden/degen_*.npz; tests/test_oracle_degenerate.py asserts what each of them
     is) through every entry point: fused with tables (Linear on int8 and on fp32 planes), granular == fused bit for bit, the
     module classes, quant_forward
  b  every sweep route of tests/test_hip_mixbit.py (LINEAR_ROUTES / MATMUL_ROUTES: the smallest shape of each kernel) with one
     zero block against the numpy oracle, the route's kernel asserted; the twin routes and sweep6-plain once more on a strictly
     negative input
  c  exact pruning with a NaN column, the passes asserted to be staged: pruned == unpruned == the engine's cross-check, bit for
     bit, and the oracle's selections
  d  one group call of a zero-block Linear, a zero-head MatMul and two healthy members: every member as its single call, the
     healthy ones still staged
  e  the edges of the fix: two non-zero intervals whose product underflows stay finite, as in the reference; an interval of 0
     handed in over data that is not zero is NaN here and finite in the reference (the documented limit, pinned)

Bars: SCORE_RTOL, TIE_RTOL, GRID_TOL, MAX_GRID_STEPS of tests/helpers.py as they stand; finiteness entry by entry
(assert_scores_close); a selection on an all-NaN column is exactly 0; an interval whose reference is +-0 is compared by its bits.
"""
import numpy as np
import pytest
import torch

from tests.degen_cases import (LINEAR, MATMUL, MMBLK, NAMES, assert_fixture_premise, assert_intervals, check_tables, expected_nan,
                               linear_params, matmul_params, same_bits)
from tests.helpers import SCORE_RTOL, candidate_grid, load_golden, record_margin
from tests.test_hip_mixbit import (HP, LINEAR_ROUTES, MATMUL_ROUTES, PRUNE_LINEAR, PRUNE_MATMUL, _cands, _kinds, _np, _same, _t,
                                   _three_ways)
from tests.test_hip_parity import _mk_attention, _mk_linear

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    return engine


def _grid(p):
    return candidate_grid(p["eq_alpha"], p["eq_beta"], p["eq_n"])


def _check_intervals(flips, got, ref, mult, what, ref_scores=None):
    """No differing selection: bit for bit (the sign of a zero included).  Otherwise a near-tie moved an interval to the
    neighbouring entry of its candidate table; zero references stay exact.  Returns the number of entries that differ."""
    if flips == 0:
        same_bits(got, ref, what)
        record_margin(None, None, {"intervals": int(np.asarray(ref).size), "differing_intervals": 0})
        return 0
    return assert_intervals(got, ref, mult, what, ref_scores=ref_scores)


def _forward_close(got, ref, K, what):
    """The NaN pattern of the reference's quantised output; elsewhere tests/test_hip_planes.py's bar for the int8 forward: 2e-6
    sqrt(K) of the largest (finite) output."""
    got, ref = np.asarray(_np(got) if torch.is_tensor(got) else got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=what + ": NaN pattern of the quantised output")
    m = ~np.isnan(ref)
    if m.any():
        err, bar = np.abs(got[m] - ref[m]).max() / np.abs(ref[m]).max(), 2e-6 * K ** 0.5
        record_margin("quant_forward_rel_err_over_bar", err / bar)
        assert err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


# ======================================================================================================================
# a. the reference's fixtures through every entry point
# ======================================================================================================================
def _linear_args(g):
    p = linear_params(g)
    return dict(weight=_t(g["weight"]), bias=_t(g["bias"]) if "bias" in g else None, x=_t(g["x"]), out=_t(g["out"]),
                grad=_t(g["grad"]), n_H=p.pop("n_H", 1), n_a=p.pop("n_a", 1), **p)


def _matmul_args(g):
    p = matmul_params(g)
    blocks = (1 if p["sos"] else p.pop("n_V_A", 1), 1 if p["sos"] else p.pop("n_H_A", 1), p.pop("n_V_B", 1), p.pop("n_H_B", 1))
    for k in ("n_V_A", "n_H_A"):
        p.pop(k, None)
    return dict(A=_t(g["A"]), B=_t(g["B"]), out=_t(g["out"]), grad=_t(g["grad"]), blocks=blocks, **p)


def _linear_tables(g, r):
    """The reference's tables of round r: [column block h], [activation block a]."""
    p = g["params"]
    n_H, n_a = p.get("n_H", 1), p.get("n_a", 1)
    tabs = g["scores"][r * (n_H + n_a):(r + 1) * (n_H + n_a)]
    return tabs[:n_H], tabs[n_H:]


@pytest.mark.parametrize("force_f32", [False, True], ids=["i8", "f32"])
@pytest.mark.parametrize("name", LINEAR)
def test_linear_fixture_fused_call(eng, name, force_f32):
    """Tables of the first weight column block and the first activation block of every round (what the fused call returns), the
    final intervals of every block, and the default call (no tables: pass memo, pruning) bit-identical to it."""
    g = load_golden(name)
    assert_fixture_premise(g, name)
    p = g["params"]
    R, n_H, n_a = p["search_round"], p.get("n_H", 1), p.get("n_a", 1)
    args = _linear_args(g)
    w_iv, a_iv, scores, best = eng.linear_calibrate(want_scores=True, force_f32=force_f32, **args)
    w2, a2 = eng.linear_calibrate(force_f32=force_f32, **args)[:2]
    torch.cuda.synchronize()
    scores, best = _np(scores), _np(best)
    want, pairs, keep = expected_nan(g), [], []
    for r in range(R):
        wt, at = _linear_tables(g, r)
        pairs.append((scores[r, 0], best[r, 0], wt[0])); keep.append(r * (n_H + n_a))
        pairs.append((scores[r, 1][:, :1], best[r, 1][:1], at[0])); keep.append(r * (n_H + n_a) + n_H)
    flips = check_tables(pairs, [want[i] for i in keep], name)
    mult = _grid(p)
    wt, at = _linear_tables(g, R - 1)
    _check_intervals(flips if (n_H, n_a) == (1, 1) else 1, _np(w_iv), g["w_interval"], mult, name + " w_interval",
                     np.stack([np.asarray(t).reshape(p["eq_n"], -1) for t in wt], axis=-1).reshape(p["eq_n"], -1))
    _check_intervals(flips if (n_H, n_a) == (1, 1) else 1, _np(a_iv), g["a_interval"], mult, name + " a_interval",
                     np.concatenate([np.asarray(t).reshape(p["eq_n"], -1) for t in at], axis=1))
    _same(w2, w_iv, name + ": call without tables, w_interval"); _same(a2, a_iv, name + ": call without tables, a_interval")


@pytest.mark.parametrize("name", MATMUL + MMBLK)
def test_matmul_fixture_fused_call(eng, name):
    """Head-wise (k_sweep9 / k_sos_split) and with 2 x 2 sub-blocks (k_pack_seg / k_sweep_seg): every table of every step."""
    g = load_golden(name)
    assert_fixture_premise(g, name)
    args = _matmul_args(g)
    sos = args["sos"]
    A_iv, B_iv, split, scores, best = eng.matmul_calibrate(want_scores=True, **args)
    A2, B2, split2 = eng.matmul_calibrate(**args)[:3]
    torch.cuda.synchronize()
    scores, best = _np(scores), _np(best)
    R, steps = scores.shape[:2]
    assert R * steps == len(g["scores"]), (scores.shape, len(g["scores"]))
    pairs = []
    for r in range(R):
        for s in range(steps):
            ref = g["scores"][r * steps + s]
            if sos and s == 0:                       # the split table: 20 rows, one column
                pairs.append((scores[r, 0][:20, :1], best[r, 0][:1], ref.reshape(-1, 1)))
            else:
                pairs.append((scores[r, s], best[r, s], ref))
    flips = check_tables(pairs, expected_nan(g), name)
    mult = _grid(g["params"])
    if sos:
        assert float(split.cpu()) == float(g["split"])
        same_bits(_np(A_iv), np.asarray(g["A_interval"], np.float32), name + " A_interval")
        _same(split2, split, name + ": call without tables, split")
    else:
        _check_intervals(flips, _np(A_iv), g["A_interval"], mult, name + " A_interval")
    _check_intervals(flips, _np(B_iv), g["B_interval"], mult, name + " B_interval")
    _same(A2, A_iv, name + ": call without tables, A_interval"); _same(B2, B_iv, name + ": call without tables, B_interval")


@pytest.mark.parametrize("name", LINEAR)
def test_linear_fixture_granular_steps_equal_the_fused_call(eng, name):
    """p4v_amax_init, then search_round x (every weight column block, every activation block): the table of EVERY block step
    against the reference's, the first block's tables and the final intervals bit-identical to the fused call's."""
    g = load_golden(name)
    p = g["params"]
    R, n_H, n_a = p["search_round"], p.get("n_H", 1), p.get("n_a", 1)
    args = _linear_args(g)
    w_f, a_f, sc_f, be_f = eng.linear_calibrate(want_scores=True, **args)
    st = eng.LinearStepper(**{k: v for k, v in args.items() if k not in ("eq_alpha", "eq_beta", "search_round")})
    w, a = st.init_intervals()
    wc, ac = _cands(eng, p, w), _cands(eng, p, a)
    pairs, blocked = [], (n_H, n_a) != (1, 1)
    for r in range(R):
        wt, at = _linear_tables(g, r)
        for h in range(n_H):
            w, sw, bw = st.search_w(wc, w, a, want_scores=True, block=h if blocked else None)
            pairs.append((_np(sw), _np(bw), wt[h]))
            if h == 0:
                _same(sw, sc_f[r, 0], f"{name} round {r} w scores"); _same(bw, be_f[r, 0], f"{name} round {r} w argmax")
        for k in range(n_a):
            a, sa, ba = st.search_a(ac, w, a, want_scores=True, block=k if blocked else None)
            pairs.append((_np(sa)[:, :1], _np(ba)[:1], at[k]))
            if k == 0:
                _same(sa[:, :1], sc_f[r, 1][:, :1], f"{name} round {r} a scores"); _same(ba[:1], be_f[r, 1][:1], f"{name} round {r} a argmax")
    _same(w, w_f, f"{name} w_interval"); _same(a, a_f, f"{name} a_interval")
    flips = check_tables(pairs, expected_nan(g), name)
    _check_intervals(flips, _np(w), g["w_interval"], _grid(p), name + " w_interval")
    _check_intervals(flips, _np(a), g["a_interval"], _grid(p), name + " a_interval")


@pytest.mark.parametrize("name", MATMUL + MMBLK)
def test_matmul_fixture_granular_steps_equal_the_fused_call(eng, name):
    """init, then search_round x (every A block -- the split search for the split-of-softmax class --, every B block) in the
    reference's order: tables, selections and intervals of every step bit-identical to the fused call's."""
    g = load_golden(name)
    p = g["params"]
    R, H = p["search_round"], g["A"].shape[1]
    args = _matmul_args(g)
    sos, (nVA, nHA, nVB, nHB) = args["sos"], args["blocks"]
    A_f, B_f, split_f, sc_f, be_f = eng.matmul_calibrate(want_scores=True, **args)
    drop = ("eq_alpha", "eq_beta", "search_round") + (() if name in MMBLK else ("blocks",))
    st = eng.MatMulStepper(**{k: v for k, v in args.items() if k not in drop})
    A_iv, B_iv = st.init_intervals()
    mult = eng.candidate_multipliers(p["eq_alpha"], p["eq_beta"], p["eq_n"], B_iv.device)
    Bc = mult.view(-1, 1, 1, 1) * B_iv.view(1, H, nVB, nHB)
    Ac = None if sos else mult.view(-1, 1, 1, 1) * A_iv.view(1, H, nVA, nHA)
    split = None
    for r in range(R):
        step = 0
        if sos:
            split, A_iv, s1, b1 = st.search_split(want_scores=True)
            _same(s1, sc_f[r, 0][:20, :1], f"{name} round {r} split scores"); _same(b1, be_f[r, 0][:1], f"{name} round {r} split argmax")
            step = 1
        elif name in MMBLK:
            for v in range(nVA):
                for h in range(nHA):
                    A_iv, s1, b1 = st.search_block("A", v, h, Ac[:, :, v, h], A_iv, B_iv, want_scores=True)
                    _same(s1, sc_f[r, step], f"{name} round {r} A block ({v}, {h}) scores")
                    _same(b1, be_f[r, step], f"{name} round {r} A block ({v}, {h}) argmax")
                    step += 1
        else:
            A_iv, s1, b1 = st.search_A(Ac.reshape(-1, H), A_iv, B_iv, want_scores=True)
            _same(s1, sc_f[r, 0], f"{name} round {r} A scores"); _same(b1, be_f[r, 0], f"{name} round {r} A argmax")
            step = 1
        if name in MMBLK:
            for v in range(nVB):
                for h in range(nHB):
                    B_iv, s2, b2 = st.search_block("B", v, h, Bc[:, :, v, h], A_iv, B_iv, split=split, want_scores=True)
                    _same(s2, sc_f[r, step], f"{name} round {r} B block ({v}, {h}) scores")
                    _same(b2, be_f[r, step], f"{name} round {r} B block ({v}, {h}) argmax")
                    step += 1
        else:
            B_iv, s2, b2 = st.search_B(Bc.reshape(-1, H), A_iv, B_iv, split=split, want_scores=True)
            _same(s2, sc_f[r, 1], f"{name} round {r} B scores"); _same(b2, be_f[r, 1], f"{name} round {r} B argmax")
            step += 1
        assert step == sc_f.shape[1]
    _same(A_iv, A_f, f"{name} A_interval"); _same(B_iv, B_f, f"{name} B_interval")
    if sos:
        _same(split, split_f, f"{name} split")


def _linear_module(g, batching):
    from ptq4vit_amd.quant_layers import linear as L
    p = linear_params(g)
    cls = {(True, False): L.PTQSLBatchingQuantLinear, (True, True): L.PostGeluPTQSLBatchingQuantLinear,
           (False, False): L.PTQSLQuantLinear, (False, True): L.PostGeluPTQSLQuantLinear}[(batching, p.pop("postgelu"))]
    m = cls(g["weight"].shape[1], g["weight"].shape[0], bias="bias" in g, **p).cuda()
    m.weight.data.copy_(_t(g["weight"]))
    if "bias" in g:
        m.bias.data.copy_(_t(g["bias"]))
    m.raw_input, m.raw_out, m.raw_grad = _t(g["x"]), _t(g["out"]), _t(g["grad"])
    return m


def _matmul_module(g, batching):
    from ptq4vit_amd.quant_layers import matmul as M
    p = matmul_params(g)
    sos = p.pop("sos")
    cls = {(True, False): M.PTQSLBatchingQuantMatMul, (True, True): M.SoSPTQSLBatchingQuantMatMul,
           (False, False): M.PTQSLQuantMatMul, (False, True): M.SoSPTQSLQuantMatMul}[(batching, sos)]
    if not batching:                                     # one group per head: the search of the batching classes
        p["n_G_A"] = p["n_G_B"] = g["A"].shape[1]
    m = cls(**p)
    m.raw_input, m.raw_out, m.raw_grad = [_t(g["A"]), _t(g["B"])], _t(g["out"]), _t(g["grad"])
    return m


def _last_tables_decided(g):
    """True if no column of the reference's tables is decided by less than SCORE_RTOL -- then the default call, which returns
    no tables, has to install the reference's intervals bit for bit (dead columns: candidate 0, nothing to decide)."""
    for t in g["scores"]:
        t = np.asarray(t, np.float64).reshape(t.shape[0], -1)
        t = t[:, ~np.isnan(t).all(axis=0)]
        if t.shape[1]:
            top = np.sort(t, axis=0)[-2:]
            if ((top[1] - top[0]) / np.maximum(np.abs(top[1]), 1e-300)).min() < SCORE_RTOL:
                return False
    return True


@pytest.mark.parametrize("name", NAMES)
def test_fixture_batching_module_class(eng, name):
    """PTQSLBatching* / PostGeluPTQSLBatching* / SoSPTQSLBatching*.calibration_step2(): the default engine call (no tables: pass
    memo, exact pruning) installs the reference's intervals in the reference's shapes -- bit for bit where every selection of
    the reference's run is decided by more than SCORE_RTOL, on the candidate grid otherwise; zero intervals always by their
    bits.  The calibrated module's quant_forward has the NaN pattern of the reference's output and, whenever the installed
    intervals ARE the reference's, its values to the int8 forward's bar."""
    g = load_golden(name)
    p = g["params"]
    flips = 0 if _last_tables_decided(g) else 1
    mult = _grid(p)
    if name in LINEAR:
        m = _linear_module(g, True)
        x = m.raw_input
        m.calibration_step2()
        assert tuple(m.w_interval.shape) == g["w_interval"].shape and tuple(m.a_interval.shape) == g["a_interval"].shape
        moved = _check_intervals(flips, _np(m.w_interval), g["w_interval"], mult, name + " w_interval")
        moved += _check_intervals(flips, _np(m.a_interval), g["a_interval"], mult, name + " a_interval")
        m.mode = "quant_forward"
        with torch.no_grad():
            qf = m(x)
        K = g["weight"].shape[1]
    else:
        m = _matmul_module(g, True)
        A, B = m.raw_input
        m.calibration_step2()
        assert tuple(m.B_interval.shape) == g["B_interval"].shape
        moved = _check_intervals(flips, _np(m.B_interval), g["B_interval"], mult, name + " B_interval")
        if p["sos"]:
            assert float(m.split) == float(g["split"])
            same_bits(_np(torch.as_tensor(m.A_interval)), np.asarray(g["A_interval"], np.float32), name + " A_interval")
        else:
            moved += _check_intervals(flips, _np(torch.as_tensor(m.A_interval)), g["A_interval"], mult, name + " A_interval")
        m.mode = "quant_forward"
        with torch.no_grad():
            qf = m(A, B)
        K = g["A"].shape[-1]
    assert m.calibrated
    got = _np(qf)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(g["quant_forward"]), err_msg=name + ": NaN pattern of the module's output")
    record_margin(None, None, {"modules": 1, "modules_on_the_reference_intervals": int(moved == 0)})
    if moved == 0:
        _forward_close(got, g["quant_forward"], K, name + " quant_forward of the calibrated module")


@pytest.mark.parametrize("name", LINEAR + MATMUL)
def test_fixture_nonbatching_module_class(eng, name):
    """PTQSLQuant* / PostGeluPTQSLQuant* / SoSPTQSLQuant*.calibration_step2(x): scores are means where the batching classes sum,
    so the reference is the oracle with batching=False on the fixture's tensors (MatMul: one group per head)."""
    from oracle.ptq4vit_oracle import LinearOracle, MatMulOracle
    g = load_golden(name)
    p = g["params"]
    mult = _grid(p)
    with np.errstate(invalid="ignore", divide="ignore"):
        if name in LINEAR:
            o = LinearOracle(g["weight"], g.get("bias"), batching=False, **linear_params(g))
            res = o.calibration_step2(g["x"], g["out"], g["grad"])
            ref_qf, K = o.quant_forward(g["x"]), g["weight"].shape[1]
        else:
            H = g["A"].shape[1]
            o = MatMulOracle(batching=False, n_G_A=1 if p["sos"] else H, n_G_B=H, **matmul_params(g))
            res = o.calibration_step2(g["A"], g["B"], g["out"], g["grad"])
            ref_qf, K = o.quant_forward(g["A"], g["B"]), g["A"].shape[-1]
    if name in LINEAR:
        m = _linear_module(g, False)
        with torch.no_grad():
            qf = m.calibration_step2(m.raw_input)
        a_iv = m.a_interval[0] if p["postgelu"] else m.a_interval
        moved = (assert_intervals(_np(m.w_interval), res["w_interval"], mult, name + " w_interval")
                 + assert_intervals(_np(a_iv), res["a_interval"], mult, name + " a_interval"))
    else:
        m = _matmul_module(g, False)
        with torch.no_grad():
            qf = m.calibration_step2(*m.raw_input)
        moved = assert_intervals(_np(m.B_interval), res["B_interval"], mult, name + " B_interval", ref_scores=o.trace[-1][1])
        if p["sos"]:
            assert float(m.split) == float(res["split"])
            same_bits(_np(torch.as_tensor(m.A_interval)), np.asarray(res["A_interval"], np.float32), name + " A_interval")
        else:
            moved += assert_intervals(_np(m.A_interval), res["A_interval"], mult, name + " A_interval", ref_scores=o.trace[-2][1])
    got = _np(qf)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref_qf), err_msg=name + ": NaN pattern of the module's output")
    if moved == 0:
        _forward_close(got, ref_qf, K, name + " quant_forward of the calibrated module")


@pytest.mark.parametrize("name", NAMES)
def test_fixture_quant_forward_on_the_reference_intervals(eng, name):
    """p4v_linear_quant_forward / p4v_matmul_quant_forward / p4v_matmul_blocks_quant_forward with the reference's intervals."""
    g = load_golden(name)
    p = g["params"]
    if name in LINEAR:
        out = eng.linear_quant_forward(weight=_t(g["weight"]), bias=_t(g["bias"]) if "bias" in g else None, x=_t(g["x"]),
                                       w_interval=_t(g["w_interval"]), a_interval=_t(g["a_interval"]), w_bit=p["w_bit"],
                                       a_bit=p["a_bit"], n_V=p["n_V"], n_H=p.get("n_H", 1), n_a=p.get("n_a", 1), postgelu=p["postgelu"])
        K = g["weight"].shape[1]
    else:
        args = _matmul_args(g)
        kw = dict(A=args["A"], B=args["B"], A_interval=_t(np.asarray(g["A_interval"], np.float32)), B_interval=_t(g["B_interval"]),
                  split=_t(np.asarray(g["split"], np.float32)) if p["sos"] else None, A_bit=p["A_bit"], B_bit=p["B_bit"], sos=p["sos"])
        out = eng.matmul_blocks_quant_forward(blocks=args["blocks"], **kw) if name in MMBLK else eng.matmul_quant_forward(**kw)
        K = g["A"].shape[-1]
    torch.cuda.synchronize()
    _forward_close(out, g["quant_forward"], K, name)


# ======================================================================================================================
# b. every sweep route with one zero block, against the numpy oracle
# ======================================================================================================================
def _run_linear(eng, inputs, *, metric, n_V, postgelu, n_H=1, n_a=1, force_generic=False):
    from oracle.ptq4vit_oracle import LinearOracle
    w, bias, x, out, grad = inputs
    hp = dict(HP, w_bit=8, a_bit=8, metric=metric, n_V=n_V, n_H=n_H, n_a=n_a)
    o = LinearOracle(w, bias, postgelu=postgelu, **hp)
    with np.errstate(invalid="ignore", divide="ignore"):
        o.calibration_step2(x, out, grad)
    try:
        eng.debug_variant(0, force_generic=force_generic)
        (w_iv, a_iv, scores, best), kinds = _kinds(eng, lambda: eng.linear_calibrate(
            weight=_t(w), bias=_t(bias), x=_t(x), out=_t(out), grad=_t(grad), postgelu=postgelu, want_scores=True, **hp))
    finally:
        eng.debug_variant(0)
    scores, best = _np(scores), _np(best)
    per_round, pairs = n_H + n_a, []
    for r in range(HP["search_round"]):
        pairs.append((scores[r, 0], best[r, 0], o.trace[r * per_round][1]))
        pairs.append((scores[r, 1][:, :1], best[r, 1][:1], o.trace[r * per_round + n_H][1]))
    flips = check_tables(pairs, None, "linear route")
    mult = candidate_grid(HP["eq_alpha"], HP["eq_beta"], HP["eq_n"])
    blocked = not (n_H == 1 and n_a == 1)             # (the fused call returns the first block's tables only)
    _check_intervals(1 if blocked else flips, _np(w_iv), o.w_interval, mult, "w_interval", o.trace[-1 - n_a][1] if n_H == 1 else None)
    _check_intervals(1 if blocked else flips, _np(a_iv), o.a_interval, mult, "a_interval", o.trace[-1][1] if n_a == 1 else None)
    return o, kinds


def _route_inputs(cfg, mutate):
    b, T, K, N = (cfg[k] for k in ("b", "T", "K", "N"))
    w, bias, x, out, grad = _mk_linear(7, b, T, K, N, cfg["postgelu"])
    w, x = w.copy(), x.copy()
    mutate(w, x)
    out = (x.reshape(-1, K) @ w.T + bias).reshape(b, T, N).astype(np.float32)
    return w, bias, x, out, grad


# (route, zero row block): block 1 everywhere; where there are three, the LAST one as well -- the block that the padding features
# of a ragged N (390 in 3 x 130 under 128-wide tiles) are counted to
ZERO_BLOCK_CASES = [(r, 1) for r in LINEAR_ROUTES] + [(r, c["n_V"] - 1) for r, (c, _) in LINEAR_ROUTES.items() if c["n_V"] > 2]


@pytest.mark.parametrize("route,block", ZERO_BLOCK_CASES, ids=[f"{r}-block{b}" for r, b in ZERO_BLOCK_CASES])
def test_linear_route_with_a_zero_block_vs_oracle(eng, route, block):
    """A zero row block where n_V > 1, the whole weight zero otherwise: the NaN columns and the finite ones, the selections
    (candidate 0 on a NaN column) and the intervals as the oracle has them."""
    cfg, kernel = LINEAR_ROUTES[route]
    cfg = dict(cfg)
    n_V, N = cfg["n_V"], cfg["N"]

    def zero(w, x):
        if n_V > 1:
            w[block * (N // n_V):(block + 1) * (N // n_V)] = 0.0
        else:
            w[:] = 0.0
    inputs = _route_inputs(cfg, zero)
    for k in ("b", "T", "K", "N"):
        cfg.pop(k)
    o, kinds = _run_linear(eng, inputs, **cfg)
    assert any(np.isnan(t).any() for _, t in o.trace), "test data: the oracle's run has no NaN"
    if n_V > 1:
        assert not np.isnan(np.delete(o.trace[0][1], block, axis=1)).any(), "test data: the other row blocks are healthy"
    print(f"[route] {route}, zero block {block}: {sorted(set(kinds))}")
    assert kernel in kinds, f"{route}: {kernel} did not run: {sorted(set(kinds))}"


NEGATIVE_ROUTES = [r for r, (c, _) in LINEAR_ROUTES.items() if c["postgelu"]] + ["sweep6-plain"]


@pytest.mark.parametrize("route", NEGATIVE_ROUTES)
def test_linear_route_on_a_strictly_negative_input_vs_oracle(eng, route):
    """Twin routes: the signed maximum, the interval and every candidate are negative -- finite tables, a negative a_interval.
    sweep6-plain: the abs-max interval stays positive, every activation sits on the negative half of the grid."""
    cfg, kernel = LINEAR_ROUTES[route]
    cfg = dict(cfg)

    def negative(w, x):
        x[:] = -np.abs(x) - np.float32(0.0025)
    inputs = _route_inputs(cfg, negative)
    for k in ("b", "T", "K", "N"):
        cfg.pop(k)
    o, kinds = _run_linear(eng, inputs, **cfg)
    assert not any(np.isnan(t).any() for _, t in o.trace) and (np.asarray(o.a_interval) < 0).all() == cfg["postgelu"]
    print(f"[route] {route} (negative input): {sorted(set(kinds))}")
    assert kernel in kinds, f"{route}: {kernel} did not run: {sorted(set(kinds))}"


def _run_matmul(eng, inputs, kind, *, metric="hessian", variant=0):
    from oracle.ptq4vit_oracle import MatMulOracle
    A, B, out, grad = inputs
    sos = kind == "sv"
    hp = dict(HP, A_bit=8, B_bit=8, metric=metric)
    o = MatMulOracle(sos=sos, **hp)
    with np.errstate(invalid="ignore", divide="ignore"):
        res = o.calibration_step2(A, B, out, grad)
    Bt = _t(np.ascontiguousarray(B.transpose(0, 1, 3, 2))).transpose(-2, -1) if kind == "qk" else _t(B)   # k.transpose VIEW
    try:
        eng.debug_variant(variant)
        (A_iv, B_iv, split, scores, best), kinds = _kinds(eng, lambda: eng.matmul_calibrate(
            A=_t(A), B=Bt, out=_t(out), grad=_t(grad), sos=sos, want_scores=True, **hp))
    finally:
        eng.debug_variant(0)
    scores, best = _np(scores), _np(best)
    pairs = []
    for r in range(HP["search_round"]):
        ta, tb = o.trace[2 * r][1], o.trace[2 * r + 1][1]
        pairs.append((scores[r, 0][:20, :1], best[r, 0][:1], ta) if sos else (scores[r, 0], best[r, 0], ta))
        pairs.append((scores[r, 1], best[r, 1], tb))
    flips = check_tables(pairs, None, f"matmul {kind}")
    mult = candidate_grid(HP["eq_alpha"], HP["eq_beta"], HP["eq_n"])
    _check_intervals(flips, _np(B_iv), res["B_interval"], mult, "B_interval", o.trace[-1][1])
    if sos:
        if flips == 0:
            assert float(split.cpu()) == float(res["split"])
            same_bits(_np(A_iv), np.asarray(res["A_interval"], np.float32), "A_interval")
    else:
        _check_intervals(flips, _np(A_iv), res["A_interval"], mult, "A_interval", o.trace[-2][1])
    return o, kinds


@pytest.mark.parametrize("operand", ["A", "B"])
@pytest.mark.parametrize("route", list(MATMUL_ROUTES))
def test_matmul_route_with_a_zero_head_vs_oracle(eng, route, operand):
    """Head 1 of A, and separately of B, all zero.  (A zero A head of the split-of-softmax class has no interval of its own:
    the oracle's tables stay finite there, and so must the engine's.)"""
    cfg, variant, kernel = MATMUL_ROUTES[route]
    A, B, out, grad = _mk_attention(5, cfg["b"], cfg["H"], cfg["S"], cfg["D"], cfg["kind"])
    A, B = A.copy(), np.ascontiguousarray(B).copy()
    (A if operand == "A" else B)[:, 1] = 0.0
    out = (A @ B).astype(np.float32)
    o, kinds = _run_matmul(eng, (A, B, out, grad), cfg["kind"], metric=cfg.get("metric", "hessian"), variant=variant)
    assert any(np.isnan(t).any() for _, t in o.trace) == (not (cfg["kind"] == "sv" and operand == "A")), "test data"
    print(f"[route] {route} zero {operand} head: {sorted(set(kinds))}")
    assert kernel in kinds, f"{route}: {kernel} did not run: {sorted(set(kinds))}"


# ======================================================================================================================
# c. exact pruning with a NaN column
# ======================================================================================================================
def test_candidate_pruning_is_exact_on_a_linear_with_a_zero_row_block(eng):
    """qkv (n_V = 3) at the size of PRUNE_LINEAR["K768"], row block 1 zero: the hull's "NaN anywhere: sweep everything"."""
    from oracle.ptq4vit_oracle import LinearOracle
    cfg = PRUNE_LINEAR["K768"]
    w, bias, x, out, grad = _mk_linear(31, cfg["b"], cfg["T"], cfg["K"], cfg["N"], False)
    w = w.copy()
    w[64:128] = 0.0
    out = (x.reshape(-1, cfg["K"]) @ w.T + bias).reshape(out.shape).astype(np.float32)
    heavy = grad.copy().reshape(-1, cfg["N"])
    heavy[np.random.default_rng(5).choice(heavy.shape[0], size=heavy.shape[0] // 40, replace=False)] *= 300.0
    grad = heavy.reshape(grad.shape)
    hp = dict(w_bit=8, a_bit=8, metric="hessian", eq_alpha=0.01, eq_beta=1.2, eq_n=100, search_round=2, n_V=3, n_H=1, n_a=1, postgelu=False)
    args = dict(weight=_t(w), bias=_t(bias), x=_t(x), out=_t(out), grad=_t(grad))
    pruned, full, checked, cnt, kinds = _three_ways(eng, lambda **k: eng.linear_calibrate(**args, **hp, **k))
    own = eng.linear_calibrate(**args, **hp)
    torch.cuda.synchronize()
    print(f"[prune] linear qkv, zero row block: {cnt}, {sorted(set(kinds))}")
    # the passes of the forced call ARE staged (three row blocks of 64 features at 788 samples), through stage B1's k_bound: what
    # is compared below is the hull's "NaN anywhere: sweep everything", not three times the full sweep
    assert cnt["staged"] > 0 and cnt["kept_full_sweep"] == 0 and cnt["not_eligible"] == 0, cnt
    assert "k_bound" in kinds, sorted(set(kinds))
    for k, what in ((0, "w_interval"), (1, "a_interval")):
        _same(pruned[k], full[k], f"pruned vs unpruned {what}"); _same(checked[k], full[k], f"cross-checked vs unpruned {what}")
        _same(own[k], full[k], f"the engine's own choice vs unpruned {what}")
    o = LinearOracle(w, bias, **hp)
    with np.errstate(invalid="ignore", divide="ignore"):
        o.calibration_step2(x, out, grad)
    assert np.isnan(o.trace[-2][1][:, 1]).all() and np.isnan(o.trace[-1][1]).all(), "test data"
    mult = candidate_grid(0.01, 1.2, 100)
    assert_intervals(_np(full[0]), o.w_interval, mult, "w_interval vs oracle", ref_scores=o.trace[-2][1])
    same_bits(_np(full[1]), o.a_interval, "a_interval vs oracle (all-NaN table: candidate 0)")


def test_candidate_pruning_is_exact_on_a_matmul_with_a_zero_head(eng):
    """q.k^T at the size of PRUNE_MATMUL["qk"], head 1 of A zero: that head's column NaN in both tables, the others pruned as ever."""
    from oracle.ptq4vit_oracle import MatMulOracle
    cfg = PRUNE_MATMUL["qk"]
    A, B, out, grad = _mk_attention(41, cfg["b"], cfg["H"], cfg["S"], cfg["D"], "qk")
    A = A.copy()
    A[:, 1] = 0.0
    out = (A @ B).astype(np.float32)
    grad = grad.copy()
    grad[:, :, 0, :] *= 300.0
    hp = dict(A_bit=8, B_bit=8, metric="hessian", eq_alpha=0.01, eq_beta=1.2, eq_n=100, search_round=2, sos=False)
    args = dict(A=_t(A), B=_t(np.ascontiguousarray(B.transpose(0, 1, 3, 2))).transpose(-2, -1), out=_t(out), grad=_t(grad))
    pruned, full, checked, cnt, kinds = _three_ways(eng, lambda **k: eng.matmul_calibrate(**args, **hp, **k))
    own = eng.matmul_calibrate(**args, **hp)
    torch.cuda.synchronize()
    print(f"[prune] matmul qk, zero A head: {cnt}, {sorted(set(kinds))}")
    assert cnt["staged"] > 0 and cnt["kept_full_sweep"] == 0 and cnt["not_eligible"] == 0, cnt      # staged, with the sliced stages
    assert {"k_slice_a", "k_slice_b"} <= set(kinds), sorted(set(kinds))
    for k, what in ((0, "A_interval"), (1, "B_interval")):
        _same(pruned[k], full[k], f"pruned vs unpruned {what}"); _same(checked[k], full[k], f"cross-checked vs unpruned {what}")
        _same(own[k], full[k], f"the engine's own choice vs unpruned {what}")
    o = MatMulOracle(**hp)
    with np.errstate(invalid="ignore", divide="ignore"):
        res = o.calibration_step2(A, B, out, grad)
    assert np.isnan(o.trace[-1][1][:, 1]).all() and not np.isnan(np.delete(o.trace[-1][1], 1, axis=1)).any(), "test data"
    mult = candidate_grid(0.01, 1.2, 100)
    assert_intervals(_np(full[0]), res["A_interval"], mult, "A_interval vs oracle", ref_scores=o.trace[-2][1])
    assert_intervals(_np(full[1]), res["B_interval"], mult, "B_interval vs oracle", ref_scores=o.trace[-1][1])
    assert _np(full[0])[1] == 0.0 and _np(full[1])[1] == np.asarray(res["B_interval"]).reshape(-1)[1]      # candidate 0, exactly


# ======================================================================================================================
# d. one group call: NaN members beside healthy ones
# ======================================================================================================================
def test_degenerate_members_in_one_group_call_equal_the_single_calls(eng):
    """The zero-row-block Linear and the zero-A-head MatMul fixtures with the qkv Linear and a q.k^T of tests/test_hip_group.py's
    mixture: every member bit-identical to its single call (NaN tables of one member leave its neighbours alone), and the
    healthy members' passes are staged as in their single calls."""
    from tests.test_hip_group import _mixture
    specs = _mixture(eng)
    healthy = [specs[3], specs[8]]
    assert healthy[0][0] == "linear" and healthy[0][1]["n_V"] == 3 and healthy[1][0] == "matmul" and not healthy[1][1]["sos"]

    def jobs(which):
        js = []
        if "degen" in which:
            js.append(eng.linear_job(**_linear_args(load_golden("degen_linear_v3_hessian_zero_rows"))))
            js.append(eng.matmul_job(**_matmul_args(load_golden("degen_matmul_qk_hessian_zero_A_head"))))
        if "healthy" in which:
            js += [getattr(eng, kind + "_job")(**kw) for kind, kw in healthy]
        return js
    eng.prune_counters(reset=True)
    single_h = [eng.run_job(j) for j in jobs(("healthy",))]
    torch.cuda.synchronize()
    cnt_single = eng.prune_counters(reset=True)
    single_d = [eng.run_job(j) for j in jobs(("degen",))]
    torch.cuda.synchronize()
    cnt_degen = eng.prune_counters(reset=True)
    eng.launch_counters(reset=True)
    grouped = eng.calibrate_group(jobs(("degen", "healthy")))
    torch.cuda.synchronize()
    cnt, lc = eng.prune_counters(reset=True), eng.launch_counters(reset=True)
    print(f"[group] healthy members alone: {cnt_single}; degenerate members alone: {cnt_degen}; the group of four: {cnt}")
    assert lc["groups"] == 1 and len(grouped) == 4
    for what, a, b in zip(("zero-block linear", "zero-head matmul", "healthy qkv", "healthy q.k^T"), single_d + single_h, grouped):
        for x, y in zip(a.outputs, b.outputs):
            assert (x is None) == (y is None)
            if x is not None:
                _same(y, x, f"{what}: grouped vs single")
    # every pass takes in the group the outcome it took alone: the group's counters are the sums over the four single calls
    assert cnt_single["staged"] > 0, cnt_single
    assert cnt == {k: cnt_single[k] + cnt_degen[k] for k in cnt}, (cnt_single, cnt_degen, cnt)
    g = load_golden("degen_linear_v3_hessian_zero_rows")
    flips = 0 if _last_tables_decided(g) else 1
    _check_intervals(flips, _np(grouped[0].outputs[0]), g["w_interval"], _grid(g["params"]), "grouped zero-block linear w_interval vs the reference")
    _check_intervals(flips, _np(grouped[0].outputs[1]), g["a_interval"], _grid(g["params"]), "grouped zero-block linear a_interval vs the reference")


# ======================================================================================================================
# e. the edges of "a factor that is +-0 makes the scale NaN" 
# ======================================================================================================================
def _forward_with(eng, w, bias, x, w_iv, a_iv, postgelu):
    from oracle.ptq4vit_oracle import LinearOracle
    o = LinearOracle(w, bias, w_bit=8, a_bit=8, n_V=1, postgelu=postgelu)
    o.w_interval, o.a_interval = np.full((1, 1, 1, 1), w_iv, np.float32), np.full((1, 1), a_iv, np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        ref = o.quant_forward(x)
    got = eng.linear_quant_forward(weight=_t(w), bias=_t(bias), x=_t(x), w_interval=_t(o.w_interval), a_interval=_t(o.a_interval),
                                   w_bit=8, a_bit=8, n_V=1, n_H=1, n_a=1, postgelu=postgelu)
    torch.cuda.synchronize()
    return _np(got), ref


def _edge_layer(scale):
    rng = np.random.default_rng(3)
    w = (rng.standard_normal((32, 64)) * scale).astype(np.float32)
    x = (rng.standard_normal((2, 9, 64)) * scale).astype(np.float32)
    bias = (rng.standard_normal(32) * 0.1).astype(np.float32)
    assert (w != 0).all() and (x != 0).all()
    return w, bias, x


def test_intervals_whose_product_underflows_give_a_finite_forward(eng):
    """Two intervals of 8e-31 are not zero, their product is (fp32 underflow).  The reference's products of fake-quantised values
    underflow the same way and its output is the bias: the scale must stay 0, not become NaN -- the NaN is keyed on a FACTOR
    being +-0, not on the table entry."""
    w, bias, x = _edge_layer(1e-28)
    w_iv, a_iv = np.float32(np.abs(w).max() / 127.5), np.float32(np.abs(x).max() / 127.5)
    assert w_iv != 0 and a_iv != 0 and np.float32(w_iv * a_iv) == 0
    got, ref = _forward_with(eng, w, bias, x, w_iv, a_iv, False)
    assert np.isfinite(ref).all() and np.array_equal(ref, np.broadcast_to(bias, ref.shape)), "test data: the reference's output is the bias"
    _forward_close(got, ref, 64, "underflowing scale product")


@pytest.mark.parametrize("case", ["weight", "twin"])
def test_a_zero_interval_handed_in_over_nonzero_data_is_nan_here_and_finite_in_the_reference(eng, case):
    """The documented limit of the fix, pinned so that it cannot drift unnoticed: an interval of +-0 that does NOT come from the
    min-max initialisation -- the data under it is not zero.  The reference divides x / 0 = +-inf, clamps and multiplies by 0:
    finite.  The engine's scale is NaN and so is every output the block touches.  No search can reach this (an initial interval
    of 0 means the block IS zero, and every candidate is a multiple of it); only quant_forward with intervals from outside can.
      weight: w_interval = 0 over a weight without a zero entry
      twin:   a_interval = -0.0 over a strictly negative post-GELU input (no row holds the exact zero that is 0 / 0)"""
    w, bias, x = _edge_layer(0.05)
    if case == "weight":
        got, ref = _forward_with(eng, w, bias, x, 0.0, np.abs(x).max() / 127.5, False)
    else:
        got, ref = _forward_with(eng, w, bias, -np.abs(x), np.abs(w).max() / 127.5, -0.0, True)
    assert np.isfinite(ref).all(), "test data: the reference's output is finite"
    assert np.isnan(got).all(), "the engine's output under a zero interval is NaN throughout (DESIGN.md s1)"
