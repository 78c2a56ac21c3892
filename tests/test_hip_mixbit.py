"""GPU: the two operands of a layer on DIFFERENT bit widths (w_bit != a_bit, A_bit != B_bit) and widths below 4.

The C ABI takes the two widths independently; every other GPU test hands both operands the same one, so a site of
csrc/p4v_api.hip that used wq for aq (Aq for Bq) -- a pack clamp, an initial interval, the post-GELU negative range, the
split-of-softmax divisors -- would pass them all, and no pass ever had one operand on the 8-bit quantiser (quant16_sat8) and the
other on the sub-8-bit one (quant_fast1 / quant16_any).

  a  fixtures the reference produced at mixed widths (tests/golden/mixbit_*.npz; tests/test_oracle_mixbit.py shows that every
     selection in them is decided by more than SCORE_RTOL and that exchanging the widths changes tables and intervals) through
     every entry point: fused with / without tables, granular, module classes, quant_forward, one group call.  NO differing
     selection is tolerated on them.
  b  every sweep route against the numpy oracle on seeded inputs, each with an 8-bit and a sub-8-bit operand both ways round;
     the kernel family that is meant to run is asserted from stats_launches().  The records name families, not template
     instances: "k_sweep6" does not tell EPI_COS / EPI_COS_T from the plain epilogue, "k_sweep2" not the swapped cosine launch
     from a plain one, "k_sweep7 (twin)" not the merged from the two-plane twin -- there the route follows from the metric,
     the shape and the variant bit handed over, and the check of the route itself is the comparison with the oracle.
  c  exact candidate pruning at mixed widths: pruned == unpruned == the engine's cross-check, bit for bit
  d  the integer planes at every width 2..8 against oracle.quant_int
  e  widths outside 2..8 are refused before any launch

Bars: SCORE_RTOL, TIE_RTOL, GRID_TOL, MAX_GRID_STEPS of tests/helpers.py as they stand (the helpers' defaults).
"""
import numpy as np
import pytest
import torch

from tests.helpers import (assert_argmax_tie_aware, assert_on_candidate_grid, assert_scores_close, candidate_grid, golden_names,
                           load_golden, record_margin)
from tests.test_hip_parity import _mk_attention, _mk_linear

pytestmark = pytest.mark.gpu

NAMES = golden_names("mixbit_")
LINEAR = [n for n in NAMES if n.startswith(("mixbit_linear_", "mixbit_postgelu_"))]
MATMUL = [n for n in NAMES if n.startswith("mixbit_matmul_")]
MMBLK = [n for n in NAMES if n.startswith("mixbit_mmblk_")]
CONV = [n for n in NAMES if n.startswith("mixbit_conv_")]

HP = dict(eq_alpha=0.01, eq_beta=1.2, eq_n=100, search_round=2)
PAIRS = [(8, 4), (4, 8), (8, 6), (6, 8)]          # an 8-bit operand (quant16_sat8) with a sub-8-bit one, both ways round
EXTRA = [(2, 8), (8, 3), (5, 7)]                  # widths that never ran: on one route per layer class
FORCE_PRUNE, CROSS_CHECK = 8388608, 134217728     # debug_variant bits (tests/test_hip_parity.py, tests/test_hip_production_path.py)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    return engine


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b, what):
    np.testing.assert_array_equal(_np(a), _np(b), err_msg=what)


def _kinds(eng, fn):
    """fn() with launch records on: (result, kernel names in launch order)."""
    eng.stats_reset()
    eng.stats_enable(True)
    try:
        res = fn()
        torch.cuda.synchronize()
        return res, [r["kernel"] for r in eng.stats_launches()]
    finally:
        eng.stats_enable(False)


def _cmp_tables(pairs, name):
    """pairs: (got_scores [C, nblk], got_best [nblk], ref_table).  Returns the number of differing selections (near-ties only)."""
    flips = 0
    for i, (got, best, ref) in enumerate(pairs):
        ref2 = np.asarray(ref).reshape(ref.shape[0], -1)
        got = got[: ref2.shape[0], : ref2.shape[1]]
        assert_scores_close(got, ref2, what=f"{name}[{i}]")
        flips += assert_argmax_tie_aware(best[: ref2.shape[1]], ref2, what=f"{name}[{i}]")
        np.testing.assert_array_equal(best[: ref2.shape[1]], np.argmax(got, axis=0), err_msg=f"{name}[{i}] select")
    return flips


# ======================================================================================================================
# a. the reference's fixtures through every entry point
# ======================================================================================================================
def _linear_args(g):
    p = dict(g["params"])
    p.pop("kind"); p.pop("oc")
    return dict(weight=_t(g["weight"]), bias=_t(g["bias"]) if "bias" in g else None, x=_t(g["x"]), out=_t(g["out"]),
                grad=_t(g["grad"]), n_H=p.pop("n_H", 1), n_a=p.pop("n_a", 1), **p)


def _matmul_args(g):
    p = dict(g["params"])
    p.pop("kind")
    blocks = (1 if p["sos"] else p.pop("n_V_A", 1), 1 if p["sos"] else p.pop("n_H_A", 1), p.pop("n_V_B", 1), p.pop("n_H_B", 1))
    for k in ("n_V_A", "n_H_A"):
        p.pop(k, None)
    return dict(A=_t(g["A"]), B=_t(g["B"]), out=_t(g["out"]), grad=_t(g["grad"]), blocks=blocks, **p)


def _conv_args(g):
    p = dict(g["params"])
    p.pop("kind")
    st = p.pop("stride")
    return dict(weight=_t(g["weight"]), bias=_t(g["bias"]), x=_t(g["x"]), out=_t(g["out"]), grad=_t(g["grad"]),
                stride=(st, st), padding=(0, 0), dilation=(1, 1), **p)


def _no_flip(flips, name):
    assert flips == 0, f"{name}: {flips} differing selections on a fixture whose every selection is decided by > SCORE_RTOL"


@pytest.mark.parametrize("force_f32", [False, True], ids=["i8", "f32"])
@pytest.mark.parametrize("name", LINEAR)
def test_linear_fixture_fused_call(eng, name, force_f32):
    g = load_golden(name)
    p = g["params"]
    R = p["search_round"]
    args = _linear_args(g)
    w_iv, a_iv, scores, best = eng.linear_calibrate(want_scores=True, force_f32=force_f32, **args)
    w2, a2 = eng.linear_calibrate(force_f32=force_f32, **args)[:2]              # memo / pruned default: no tables
    torch.cuda.synchronize()
    scores, best = _np(scores), _np(best)
    pairs = []
    for r in range(R):
        pairs.append((scores[r, 0], best[r, 0], g["scores"][2 * r]))
        pairs.append((scores[r, 1][:, :1], best[r, 1][:1], g["scores"][2 * r + 1]))
    _no_flip(_cmp_tables(pairs, name), name)
    np.testing.assert_array_equal(_np(w_iv), g["w_interval"].reshape(-1))
    np.testing.assert_array_equal(_np(a_iv), g["a_interval"].reshape(-1))
    record_margin(None, None, {"intervals": int(w_iv.numel() + a_iv.numel()), "differing_intervals": 0})
    _same(w2, w_iv, name + ": call without tables, w_interval"); _same(a2, a_iv, name + ": call without tables, a_interval")


@pytest.mark.parametrize("name", MATMUL + MMBLK)
def test_matmul_fixture_fused_call(eng, name):
    """Head-wise (k_sweep9 / k_sos_split) and with 2 x 2 sub-blocks (k_pack_seg / k_sweep_seg)."""
    g = load_golden(name)
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
    _no_flip(_cmp_tables(pairs, name), name)
    np.testing.assert_array_equal(_np(A_iv).reshape(-1), np.asarray(g["A_interval"]).reshape(-1))
    np.testing.assert_array_equal(_np(B_iv).reshape(-1), g["B_interval"].reshape(-1))
    record_margin(None, None, {"intervals": int(A_iv.numel() + B_iv.numel()), "differing_intervals": 0})
    _same(A2, A_iv, name + ": call without tables, A_interval"); _same(B2, B_iv, name + ": call without tables, B_interval")
    if sos:
        assert float(split.cpu()) == float(g["split"])
        _same(split2, split, name + ": call without tables, split")


@pytest.mark.parametrize("name", CONV)
def test_conv_fixture_fused_call(eng, name):
    g = load_golden(name)
    args = _conv_args(g)
    R = args["search_round"]
    w_iv, a_iv, scores, best = eng.conv_calibrate(want_scores=True, **args)
    w2, a2 = eng.conv_calibrate(**args)[:2]
    torch.cuda.synchronize()
    scores, best = _np(scores), _np(best)
    pairs = []
    for r in range(R):
        pairs.append((scores[r, 0], best[r, 0], g["scores"][2 * r]))
        pairs.append((scores[r, 1][:, :1], best[r, 1][:1], g["scores"][2 * r + 1]))
    _no_flip(_cmp_tables(pairs, name), name)
    np.testing.assert_array_equal(_np(w_iv), np.asarray(g["w_interval"]).reshape(-1))
    np.testing.assert_array_equal(_np(a_iv), np.asarray(g["a_interval"]).reshape(-1))
    record_margin(None, None, {"intervals": int(w_iv.numel() + a_iv.numel()), "differing_intervals": 0})
    _same(w2, w_iv, name + ": call without tables, w_interval"); _same(a2, a_iv, name + ": call without tables, a_interval")


def _cands(eng, p, iv):
    """Reference linear.py:544-545: fp32 multipliers x the INITIAL interval, computed once before the round loop."""
    mult = eng.candidate_multipliers(p["eq_alpha"], p["eq_beta"], p["eq_n"], iv.device)
    return mult.view(-1, 1) * iv.reshape(1, -1)


@pytest.mark.parametrize("name", LINEAR + MATMUL + CONV)
def test_fixture_granular_steps_equal_the_fused_call(eng, name):
    """init, then search_round x (first operand, second operand) as the reference chains its methods: tables, selections and
    intervals of every step bit-identical to the fused call's."""
    g = load_golden(name)
    p = g["params"]
    R = p["search_round"]
    drop = ("eq_alpha", "eq_beta", "search_round", "blocks")
    if name in MATMUL:
        args = _matmul_args(g)
        sos = args["sos"]
        A_f, B_f, split_f, sc_f, be_f = eng.matmul_calibrate(want_scores=True, **args)
        st = eng.MatMulStepper(**{k: v for k, v in args.items() if k not in drop})
        A_iv, B_iv = st.init_intervals()
        Bc = _cands(eng, p, B_iv)
        Ac = None if sos else _cands(eng, p, A_iv)
        split = None
        for r in range(R):
            if sos:
                split, A_iv, s1, b1 = st.search_split(want_scores=True)
                _same(s1, sc_f[r, 0][:20, :1], f"{name} round {r} split scores"); _same(b1, be_f[r, 0][:1], f"{name} round {r} split argmax")
            else:
                A_iv, s1, b1 = st.search_A(Ac, A_iv, B_iv, want_scores=True)
                _same(s1, sc_f[r, 0], f"{name} round {r} A scores"); _same(b1, be_f[r, 0], f"{name} round {r} A argmax")
            B_iv, s2, b2 = st.search_B(Bc, A_iv, B_iv, split=split, want_scores=True)
            _same(s2, sc_f[r, 1], f"{name} round {r} B scores"); _same(b2, be_f[r, 1], f"{name} round {r} B argmax")
        _same(A_iv, A_f, f"{name} A_interval"); _same(B_iv, B_f, f"{name} B_interval")
        if sos:
            _same(split, split_f, f"{name} split")
        return
    args = _linear_args(g) if name in LINEAR else _conv_args(g)
    fused = eng.linear_calibrate if name in LINEAR else eng.conv_calibrate
    w_f, a_f, sc_f, be_f = fused(want_scores=True, **args)
    st = (eng.LinearStepper if name in LINEAR else eng.ConvStepper)(**{k: v for k, v in args.items() if k not in drop})
    w, a = st.init_intervals()
    wc, ac = _cands(eng, p, w), _cands(eng, p, a)
    for r in range(R):
        w, sw, bw = st.search_w(wc, w, a, want_scores=True)
        _same(sw, sc_f[r, 0], f"{name} round {r} w scores"); _same(bw, be_f[r, 0], f"{name} round {r} w argmax")
        a, sa, ba = st.search_a(ac, w, a, want_scores=True)
        _same(sa[:, :1], sc_f[r, 1][:, :1], f"{name} round {r} a scores"); _same(ba[:1], be_f[r, 1][:1], f"{name} round {r} a argmax")
    _same(w, w_f, f"{name} w_interval"); _same(a, a_f, f"{name} a_interval")


@pytest.mark.parametrize("name", MMBLK)
def test_sub_block_fixture_granular_steps_equal_the_fused_call(eng, name):
    """p4v_amax_init_matmul_blocks, then search_round x (every A block -- the split search for the split-of-softmax class --, every
    B block) through p4v_matmul_blocks_search in the reference's product(range(n_V), range(n_H)) order: the table, the selection
    and the intervals of every block step bit-identical to the fused call's, the final intervals the reference's."""
    g = load_golden(name)
    p = g["params"]
    R, H = p["search_round"], g["A"].shape[1]
    args = _matmul_args(g)
    sos, (nVA, nHA, nVB, nHB) = args["sos"], args["blocks"]
    A_f, B_f, split_f, sc_f, be_f = eng.matmul_calibrate(want_scores=True, **args)
    st = eng.MatMulStepper(**{k: v for k, v in args.items() if k not in ("eq_alpha", "eq_beta", "search_round")})
    assert st.blocks == args["blocks"]
    A_iv, B_iv = st.init_intervals()
    assert (A_iv is None) == sos and B_iv.numel() == H * nVB * nHB
    mult = eng.candidate_multipliers(p["eq_alpha"], p["eq_beta"], p["eq_n"], B_iv.device).view(-1, 1)
    Bc = mult.view(-1, 1, 1, 1) * B_iv.view(1, H, nVB, nHB)                  # multipliers x the INITIAL intervals (matmul.py:571-572)
    Ac = None if sos else mult.view(-1, 1, 1, 1) * A_iv.view(1, H, nVA, nHA)
    split = None
    for r in range(R):
        step = 0
        if sos:
            split, A_iv, s1, b1 = st.search_split(want_scores=True)
            _same(s1, sc_f[r, 0][:20, :1], f"{name} round {r} split scores"); _same(b1, be_f[r, 0][:1], f"{name} round {r} split argmax")
            step = 1
        else:
            for v in range(nVA):
                for h in range(nHA):
                    A_iv, s1, b1 = st.search_block("A", v, h, Ac[:, :, v, h], A_iv, B_iv, want_scores=True)
                    _same(s1, sc_f[r, step], f"{name} round {r} A block ({v}, {h}) scores")
                    _same(b1, be_f[r, step], f"{name} round {r} A block ({v}, {h}) argmax")
                    step += 1
        for v in range(nVB):
            for h in range(nHB):
                B_iv, s2, b2 = st.search_block("B", v, h, Bc[:, :, v, h], A_iv, B_iv, split=split, want_scores=True)
                _same(s2, sc_f[r, step], f"{name} round {r} B block ({v}, {h}) scores")
                _same(b2, be_f[r, step], f"{name} round {r} B block ({v}, {h}) argmax")
                step += 1
        assert step == sc_f.shape[1]
    _same(A_iv, A_f, f"{name} A_interval"); _same(B_iv, B_f, f"{name} B_interval")
    np.testing.assert_array_equal(_np(B_iv), g["B_interval"].reshape(-1))
    np.testing.assert_array_equal(_np(A_iv), np.asarray(g["A_interval"], np.float32).reshape(-1))
    if sos:
        _same(split, split_f, f"{name} split")
        assert float(split.cpu()) == float(g["split"])


def _linear_module(g, batching):
    from ptq4vit_amd.quant_layers import linear as L
    p = g["params"]
    cls = {(True, False): L.PTQSLBatchingQuantLinear, (True, True): L.PostGeluPTQSLBatchingQuantLinear,
           (False, False): L.PTQSLQuantLinear, (False, True): L.PostGeluPTQSLQuantLinear}[(batching, p["postgelu"])]
    m = cls(g["weight"].shape[1], g["weight"].shape[0], bias="bias" in g, w_bit=p["w_bit"], a_bit=p["a_bit"], metric=p["metric"],
            search_round=p["search_round"], eq_alpha=p["eq_alpha"], eq_beta=p["eq_beta"], eq_n=p["eq_n"], n_V=p["n_V"]).cuda()
    m.weight.data.copy_(_t(g["weight"]))
    if "bias" in g:
        m.bias.data.copy_(_t(g["bias"]))
    m.raw_input, m.raw_out, m.raw_grad = _t(g["x"]), _t(g["out"]), _t(g["grad"])
    return m


def _matmul_module(g, batching):
    from ptq4vit_amd.quant_layers import matmul as M
    p = dict(g["params"])
    p.pop("kind")
    sos = p.pop("sos")
    cls = {(True, False): M.PTQSLBatchingQuantMatMul, (True, True): M.SoSPTQSLBatchingQuantMatMul,
           (False, False): M.PTQSLQuantMatMul, (False, True): M.SoSPTQSLQuantMatMul}[(batching, sos)]
    if not batching:                                     # one group per head: the search of the batching classes
        p["n_G_A"] = p["n_G_B"] = g["A"].shape[1]
    m = cls(**p)
    m.raw_input, m.raw_out, m.raw_grad = [_t(g["A"]), _t(g["B"])], _t(g["out"]), _t(g["grad"])
    return m


def _conv_module(g):
    from ptq4vit_amd.quant_layers.conv import ChannelwiseBatchingQuantConv2d
    p = g["params"]
    oc, ic, k, _ = g["weight"].shape
    m = ChannelwiseBatchingQuantConv2d(ic, oc, k, stride=p["stride"], w_bit=p["w_bit"], a_bit=p["a_bit"], metric=p["metric"],
                                       search_round=p["search_round"], eq_alpha=p["eq_alpha"], eq_beta=p["eq_beta"],
                                       eq_n=p["eq_n"]).cuda()
    m.weight.data.copy_(_t(g["weight"])); m.bias.data.copy_(_t(g["bias"]))
    m.raw_input, m.raw_out, m.raw_grad = _t(g["x"]), _t(g["out"]), _t(g["grad"])
    return m


@pytest.mark.parametrize("name", NAMES)
def test_fixture_batching_module_class(eng, name):
    """PTQSLBatching* / PostGeluPTQSLBatching* / SoSPTQSLBatching* / ChannelwiseBatching*.calibration_step2(): the default engine
    call (no tables: pass memo, exact pruning) installs the reference's intervals, bit for bit, in the reference's shapes."""
    g = load_golden(name)
    if name in LINEAR:
        m = _linear_module(g, True)
        m.calibration_step2()
        np.testing.assert_array_equal(_np(m.w_interval), g["w_interval"]); np.testing.assert_array_equal(_np(m.a_interval), g["a_interval"])
        if g["params"]["postgelu"]:
            assert float(m.a_neg_interval) == 0.16997124254703522 / 2 ** (g["params"]["a_bit"] - 1)
    elif name in CONV:
        m = _conv_module(g)
        m.calibration_step2()
        np.testing.assert_array_equal(_np(m.w_interval).reshape(-1), np.asarray(g["w_interval"]).reshape(-1))
        np.testing.assert_array_equal(_np(m.a_interval).reshape(-1), np.asarray(g["a_interval"]).reshape(-1))
    else:
        m = _matmul_module(g, True)
        m.calibration_step2()
        np.testing.assert_array_equal(_np(m.B_interval), g["B_interval"])
        np.testing.assert_array_equal(_np(torch.as_tensor(m.A_interval)).reshape(-1), np.asarray(g["A_interval"]).reshape(-1))
        if g["params"]["sos"]:
            assert float(m.split) == float(g["split"])
    assert m.calibrated


@pytest.mark.parametrize("name", LINEAR + MATMUL)
def test_fixture_nonbatching_module_class(eng, name):
    """PTQSLQuant* / PostGeluPTQSLQuant* / SoSPTQSLQuant*.calibration_step2(x): scores are means where the batching classes sum,
    so the reference is the oracle with batching=False on the fixture's tensors (MatMul: one group per head).  Intervals equal
    the oracle's, or lie on the neighbouring entry of the candidate table (a tie of the oracle's own last table)."""
    from oracle.ptq4vit_oracle import LinearOracle, MatMulOracle
    g = load_golden(name)
    p = dict(g["params"])
    p.pop("kind")
    mult = candidate_grid(p["eq_alpha"], p["eq_beta"], p["eq_n"])
    if name in LINEAR:
        p.pop("oc")
        o = LinearOracle(g["weight"], g.get("bias"), batching=False, **p)
        res = o.calibration_step2(g["x"], g["out"], g["grad"])
        m = _linear_module(g, False)
        with torch.no_grad():
            qf = m.calibration_step2(m.raw_input)
        a_iv = m.a_interval[0] if p["postgelu"] else m.a_interval
        moved = (assert_on_candidate_grid(_np(m.w_interval), res["w_interval"], mult, name + " w_interval", ref_scores=o.trace[-2][1])
                 + assert_on_candidate_grid(_np(a_iv), res["a_interval"], mult, name + " a_interval", ref_scores=o.trace[-1][1]))
        ref_qf, K = o.quant_forward(g["x"]), g["weight"].shape[1]
    else:
        H = g["A"].shape[1]
        o = MatMulOracle(batching=False, n_G_A=1 if p["sos"] else H, n_G_B=H, **p)
        res = o.calibration_step2(g["A"], g["B"], g["out"], g["grad"])
        m = _matmul_module(g, False)
        with torch.no_grad():
            qf = m.calibration_step2(*m.raw_input)
        moved = assert_on_candidate_grid(_np(m.B_interval), res["B_interval"], mult, name + " B_interval", ref_scores=o.trace[-1][1])
        if p["sos"]:
            assert float(m.split) == float(res["split"])
            np.testing.assert_array_equal(_np(torch.as_tensor(m.A_interval)).reshape(-1), np.asarray(res["A_interval"], np.float32).reshape(-1))
        else:
            moved += assert_on_candidate_grid(_np(m.A_interval), res["A_interval"], mult, name + " A_interval", ref_scores=o.trace[-2][1])
        ref_qf, K = o.quant_forward(g["A"], g["B"]), g["A"].shape[-1]
    if moved == 0:
        _close(qf, ref_qf, K, name + " quant_forward of the calibrated module")


def _close(got, ref, K, what):
    """quant_forward: the engine multiplies grid indices exactly and rescales once, the reference multiplies fake-quantised fp32
    operands -- the same real number to fp32 GEMM noise: 2e-6 sqrt(K) of the largest output (tests/test_hip_planes.py's bar)."""
    got, ref = np.asarray(_np(got) if torch.is_tensor(got) else got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err, bar = np.abs(got - ref).max() / np.abs(ref).max(), 2e-6 * K ** 0.5
    record_margin("quant_forward_rel_err_over_bar", err / bar)
    assert err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


@pytest.mark.parametrize("name", NAMES)
def test_fixture_quant_forward_on_the_reference_intervals(eng, name):
    g = load_golden(name)
    p = g["params"]
    if name in LINEAR:
        out = eng.linear_quant_forward(weight=_t(g["weight"]), bias=_t(g["bias"]) if "bias" in g else None, x=_t(g["x"]),
                                       w_interval=_t(g["w_interval"]), a_interval=_t(g["a_interval"]), w_bit=p["w_bit"],
                                       a_bit=p["a_bit"], n_V=p["n_V"], n_H=1, n_a=1, postgelu=p["postgelu"])
        K = g["weight"].shape[1]
    elif name in CONV:                                # the Conv2d classes have no int8 forward: their torch formulation on the GPU
        m = _conv_module(g)
        m.w_interval, m.a_interval = _t(np.asarray(g["w_interval"])), _t(np.asarray(g["a_interval"]))
        m.calibrated, m.mode = True, "quant_forward"
        with torch.no_grad():
            out = m(m.raw_input)
        K = int(np.prod(g["weight"].shape[1:]))
    else:
        args = _matmul_args(g)
        kw = dict(A=args["A"], B=args["B"], A_interval=_t(np.asarray(g["A_interval"], np.float32)), B_interval=_t(g["B_interval"]),
                  split=_t(np.asarray(g["split"], np.float32)) if p["sos"] else None, A_bit=p["A_bit"], B_bit=p["B_bit"], sos=p["sos"])
        out = eng.matmul_blocks_quant_forward(blocks=args["blocks"], **kw) if name in MMBLK else eng.matmul_quant_forward(**kw)
        K = g["A"].shape[-1]
    torch.cuda.synchronize()
    _close(out, g["quant_forward"], K, name)


def test_fixtures_in_one_group_call_equal_the_single_calls(eng):
    def jobs():
        js = [eng.linear_job(**_linear_args(load_golden(n))) for n in LINEAR]
        js += [eng.matmul_job(**_matmul_args(load_golden(n))) for n in MATMUL + MMBLK]
        return js + [eng.conv_job(**_conv_args(load_golden(n))) for n in CONV]
    single = [eng.run_job(j) for j in jobs()]
    torch.cuda.synchronize()
    eng.launch_counters(reset=True)
    grouped = eng.calibrate_group(jobs())
    torch.cuda.synchronize()
    cnt = eng.launch_counters(reset=True)
    assert cnt["groups"] == 1 and len(grouped) == len(NAMES) == 12
    for n, a, b in zip(LINEAR + MATMUL + MMBLK + CONV, single, grouped):
        for x, y in zip(a.outputs, b.outputs):
            assert (x is None) == (y is None)
            if x is not None:
                _same(y, x, f"{n}: grouped vs single")
        g = load_golden(n)                            # ... and both are the reference's
        ref = (g["A_interval"], g["B_interval"]) if "A" in g else (g["w_interval"], g["a_interval"])
        for x, r in zip(b.outputs, ref):
            np.testing.assert_array_equal(_np(x).reshape(-1), np.asarray(r, np.float32).reshape(-1), err_msg=n)


# ======================================================================================================================
# b. every sweep route at mixed widths, against the numpy oracle
# ======================================================================================================================
def _run_linear(eng, inputs, bits, *, metric, n_V, postgelu, n_H=1, n_a=1, variant=0, force_generic=False):
    from oracle.ptq4vit_oracle import LinearOracle
    w, bias, x, out, grad = inputs
    hp = dict(HP, w_bit=bits[0], a_bit=bits[1], metric=metric, n_V=n_V, n_H=n_H, n_a=n_a)
    o = LinearOracle(w, bias, postgelu=postgelu, **hp)
    o.calibration_step2(x, out, grad)
    try:
        eng.debug_variant(variant, force_generic=force_generic)
        (w_iv, a_iv, scores, best), kinds = _kinds(eng, lambda: eng.linear_calibrate(
            weight=_t(w), bias=_t(bias), x=_t(x), out=_t(out), grad=_t(grad), postgelu=postgelu, want_scores=True, **hp))
    finally:
        eng.debug_variant(0)
    scores, best = _np(scores), _np(best)
    per_round, pairs = n_H + n_a, []
    for r in range(HP["search_round"]):
        pairs.append((scores[r, 0], best[r, 0], o.trace[r * per_round][1]))
        pairs.append((scores[r, 1][:, :1], best[r, 1][:1], o.trace[r * per_round + n_H][1]))
    what = f"linear w{bits[0]}a{bits[1]}"
    flips = _cmp_tables(pairs, what)
    mult = candidate_grid(HP["eq_alpha"], HP["eq_beta"], HP["eq_n"])
    moved = (assert_on_candidate_grid(_np(w_iv), o.w_interval, mult, what + " w_interval", ref_scores=o.trace[-1 - n_a][1] if n_H == 1 else None)
             + assert_on_candidate_grid(_np(a_iv), o.a_interval, mult, what + " a_interval", ref_scores=o.trace[-1][1] if n_a == 1 else None))
    if flips == 0 and n_H == 1 and n_a == 1:
        assert moved == 0, "same selections but different intervals"
    return (w_iv, a_iv, scores, best), kinds


# route -> (shape and search, the kernel that must run).  Shapes: the smallest the existing tests use for the route.  K = 100,
# N = 130 runs on k_sweep4/5 by itself: the generic int8 kernel is kept with the engine's force_generic switch, as in
# test_hip_parity.py::test_fast_sweep_matches_generic_sweep.
LINEAR_ROUTES = {
    "sweep6-plain": (dict(b=3, T=50, K=192, N=96, n_V=1, metric="hessian", postgelu=False), "k_sweep6"),
    "sweep6-twin": (dict(b=2, T=40, K=384, N=128, n_V=1, metric="hessian", postgelu=True), "k_sweep6"),
    "sweep45-K320": (dict(b=2, T=70, K=320, N=128, n_V=1, metric="hessian", postgelu=False), "k_sweep4/5"),
    "sweep45-K100": (dict(b=2, T=70, K=100, N=130, n_V=1, metric="hessian", postgelu=False), "k_sweep4/5"),
    "generic-int8": (dict(b=2, T=70, K=100, N=130, n_V=1, metric="hessian", postgelu=False, force_generic=True), "k_sweep<int8>"),
    "sweep7-plain": (dict(b=2, T=70, K=1024, N=192, n_V=3, metric="hessian", postgelu=False), "k_sweep7"),
    "sweep7-merged-twin": (dict(b=2, T=150, K=1024, N=64, n_V=1, metric="hessian", postgelu=True), "k_sweep7 (twin)"),
    "K1088-twin": (dict(b=2, T=70, K=1088, N=130, n_V=1, metric="hessian", postgelu=True), "k_sweep2g"),
    "cos-sweep6": (dict(b=3, T=50, K=192, N=192, n_V=3, metric="cosine", postgelu=False), "k_sweep6"),
    "cos-sweep7": (dict(b=2, T=70, K=1024, N=256, n_V=1, metric="cosine", postgelu=False), "k_sweep7"),
    "cos-swapped-sweep2": (dict(b=5, T=61, K=200, N=390, n_V=3, metric="cosine", postgelu=False), "k_sweep2"),
    "f32-general": (dict(b=3, T=50, K=96, N=160, n_V=2, n_H=2, n_a=2, metric="hessian", postgelu=False), "k_sweep<float>"),
    "f32-general-twin": (dict(b=3, T=50, K=96, N=160, n_V=2, n_H=2, n_a=2, metric="hessian", postgelu=True), "k_sweep<float>"),
}
LINEAR_CASES = [(r, bits) for r in LINEAR_ROUTES for bits in PAIRS] + [("sweep6-twin", bits) for bits in EXTRA]


@pytest.mark.parametrize("route,bits", LINEAR_CASES, ids=[f"{r}-w{b[0]}a{b[1]}" for r, b in LINEAR_CASES])
def test_linear_route_at_mixed_widths_vs_oracle(eng, route, bits):
    cfg, kernel = LINEAR_ROUTES[route]
    cfg = dict(cfg)
    b, T, K, N = (cfg.pop(k) for k in ("b", "T", "K", "N"))
    _, kinds = _run_linear(eng, _mk_linear(7, b, T, K, N, cfg["postgelu"]), bits, **cfg)
    print(f"[route] {route} w{bits[0]}a{bits[1]}: {sorted(set(kinds))}")
    assert kernel in kinds, f"{route}: {kernel} did not run: {sorted(set(kinds))}"


@pytest.mark.parametrize("bits", PAIRS, ids=lambda b: f"w{b[0]}a{b[1]}")
def test_two_plane_twin_equals_the_merged_twin_at_mixed_widths(eng, bits):
    """k_sweep7's post-GELU weight search: the merged k_pos + k_neg plane (default) against the two streamed planes (variant
    2097152; both are recorded as "k_sweep7 (twin)"): bit-identical tables, selections, intervals.  [0, aq - 1] / [-aq, 0] and
    a_neg follow a_bit alone."""
    cfg = dict(LINEAR_ROUTES["sweep7-merged-twin"][0])
    b, T, K, N = (cfg.pop(k) for k in ("b", "T", "K", "N"))
    inputs = _mk_linear(7, b, T, K, N, True)
    merged, k1 = _run_linear(eng, inputs, bits, **cfg)
    two, k2 = _run_linear(eng, inputs, bits, variant=2097152, **cfg)
    assert "k_sweep7 (twin)" in k1 and "k_sweep7 (twin)" in k2, (sorted(set(k1)), sorted(set(k2)))
    for a, c, what in zip(merged, two, ("w_interval", "a_interval", "score tables", "selections")):
        np.testing.assert_array_equal(_np(a) if torch.is_tensor(a) else a, _np(c) if torch.is_tensor(c) else c, err_msg=what)


def _run_matmul(eng, inputs, bits, kind, *, metric="hessian", variant=0):
    from oracle.ptq4vit_oracle import MatMulOracle
    A, B, out, grad = inputs
    sos = kind == "sv"
    hp = dict(HP, A_bit=bits[0], B_bit=bits[1], metric=metric)
    o = MatMulOracle(sos=sos, **hp)
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
    what = f"matmul {kind} A{bits[0]}B{bits[1]}"
    flips = _cmp_tables(pairs, what)
    mult = candidate_grid(HP["eq_alpha"], HP["eq_beta"], HP["eq_n"])
    moved = assert_on_candidate_grid(_np(B_iv), res["B_interval"], mult, what + " B_interval", ref_scores=o.trace[-1][1])
    if sos:
        if flips == 0:
            assert float(split.cpu()) == float(res["split"])
            np.testing.assert_array_equal(_np(A_iv), np.asarray(res["A_interval"], np.float32).reshape(-1))
    else:
        moved += assert_on_candidate_grid(_np(A_iv), res["A_interval"], mult, what + " A_interval", ref_scores=o.trace[-2][1])
    if flips == 0:
        assert moved == 0, "same selections but different intervals"
    return (A_iv, B_iv, split, scores, best), kinds


MATMUL_ROUTES = {
    "sweep9": (dict(kind="qk", b=24, H=3, S=49, D=32), 0, "k_sweep9"),
    "sweep8": (dict(kind="qk", b=24, H=3, S=49, D=32), 524288, "k_sweep8"),
    "streaming": (dict(kind="qk", b=1, H=3, S=129, D=96), 0, "k_sweep2"),
    "sos-split": (dict(kind="sv", b=2, H=2, S=144, D=32), 0, "k_sos_split"),
    "sos-f32-split": (dict(kind="sv", b=1, H=2, S=257, D=64), 0, "k_sweep<float>"),
    # cosine: matmul_impl hands the operands over the other way round (row = B, col = A) while the scale tables keep the A, B
    # order, and the split-of-softmax class takes the fp32 PACK_SOS_SIM planes
    "cos-qk": (dict(kind="qk", b=1, H=3, S=129, D=96, metric="cosine"), 0, "k_sweep2"),
    "cos-sos": (dict(kind="sv", b=2, H=2, S=144, D=32, metric="cosine"), 0, "k_sweep<float>"),
}
MATMUL_CASES = ([(r, bits) for r in MATMUL_ROUTES for bits in PAIRS] + [("sweep9", bits) for bits in EXTRA]
                + [("sos-split", bits) for bits in EXTRA] + [("cos-qk", (5, 7)), ("cos-sos", (2, 8))])


@pytest.mark.parametrize("route,bits", MATMUL_CASES, ids=[f"{r}-A{b[0]}B{b[1]}" for r, b in MATMUL_CASES])
def test_matmul_route_at_mixed_widths_vs_oracle(eng, route, bits):
    cfg, variant, kernel = MATMUL_ROUTES[route]
    inputs = _mk_attention(5, cfg["b"], cfg["H"], cfg["S"], cfg["D"], cfg["kind"])
    res, kinds = _run_matmul(eng, inputs, bits, cfg["kind"], metric=cfg.get("metric", "hessian"), variant=variant)
    print(f"[route] {route} A{bits[0]}B{bits[1]}: {sorted(set(kinds))}")
    assert kernel in kinds, f"{route}: {kernel} did not run: {sorted(set(kinds))}"
    if route == "sweep8":                             # the 128-tile sweep selects what the 16 x 16-block sweep selects
        ref, k9 = _run_matmul(eng, inputs, bits, cfg["kind"])
        assert "k_sweep9" in k9 and "k_sweep8" not in k9
        np.testing.assert_array_equal(res[4], ref[4], err_msg="k_sweep8 vs k_sweep9 selections")
        _same(res[0], ref[0], "A_interval"); _same(res[1], ref[1], "B_interval")


def _expand(s, rows, cols):
    """[H][nV][nH] block values -> [H][rows][cols] (blocks of ceil(dim / n), reference matmul.py:109-122)."""
    H, nV, nH = s.shape
    cr, cc = -(-rows // nV), -(-cols // nH)
    return s[:, np.arange(rows) // cr][:, :, np.arange(cols) // cc]


@pytest.mark.parametrize("bits", [(8, 4), (4, 8)], ids=lambda b: f"A{b[0]}B{b[1]}")
def test_segmented_forward_is_exact_on_integer_data_at_mixed_widths(eng, bits):
    """k_pack_seg / k_sweep_seg: the exact-integer case of tests/test_hip_mmblk.py with one operand on a 4-bit grid.  Grid indices
    are drawn to FILL each operand's own grid ([-8, 7] at 4 bits, [-100, 100] at 8), block scales are powers of two, so every
    partial sum is representable: the int8 forward equals the float64 product bit for bit -- and an operand clamped to the
    other's grid does not (100 does not fit 4 bits)."""
    b, H, M, K, N = 1, 2, 133, 70, 37
    blocks = nVA, nHA, nVB, nHB = 2, 2, 3, 2
    rng = np.random.default_rng(5)
    e = lambda off, nV, nH: (2.0 ** -(np.arange(nV * nH).reshape(nV, nH)[None] + np.arange(H)[:, None, None] + off)).astype(np.float32)
    sA, sB = e(0, nVA, nHA), e(1, nVB, nHB)
    rA, rB = ((100, 7) if bits == (8, 4) else (7, 100))
    kA = rng.integers(-rA, rA + 1, size=(b, H, M, K)).astype(np.float32)
    kB = rng.integers(-rB, rB + 1, size=(b, H, K, N)).astype(np.float32)
    kA[..., 0, :], kA[..., :, 0] = rA, -rA - (1 if rA == 7 else 0)          # both clamp ends of the narrow grid are used: 7 and -8
    kB[..., 0, :], kB[..., :, 0] = rB, -rB - (1 if rB == 7 else 0)
    A, B = kA * _expand(sA, M, K)[None], kB * _expand(sB, K, N)[None]
    want = A.astype(np.float64) @ B.astype(np.float64)
    assert np.array_equal(want, want.astype(np.float32).astype(np.float64)), "test data: every output must be an fp32 number"
    got, kinds = _kinds(eng, lambda: eng.matmul_blocks_quant_forward(A=_t(A), B=_t(B), A_interval=_t(sA), B_interval=_t(sB), split=None,
                                                                     A_bit=bits[0], B_bit=bits[1], blocks=blocks))
    got = _np(got)
    bad = np.argwhere(got.astype(np.float64) != want)
    assert bad.size == 0, f"{len(bad)} of {want.size} outputs differ, first at {bad[0]}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"
    assert "k_sweep_seg" in kinds, sorted(set(kinds))


def _mk_conv(seed, b, ic, H, W, oc, kh, kw, padding):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((oc, ic, kh, kw)) * 0.05 * np.linspace(0.3, 3.0, oc)[:, None, None, None]).astype(np.float32)
    bias = (rng.standard_normal(oc) * 0.1).astype(np.float32)
    x = rng.standard_normal((b, ic, H, W)).astype(np.float32)
    out = torch.nn.functional.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(bias), stride=(kh, kw), padding=padding).numpy()
    grad = (rng.standard_normal(out.shape) * 1e-3).astype(np.float32)
    return w, bias, x, out, grad


@pytest.mark.parametrize("bits", PAIRS + EXTRA + [(8, 16)], ids=lambda b: f"w{b[0]}a{b[1]}")
def test_channelwise_conv_at_mixed_widths_vs_oracle(eng, bits):
    """32 x 24 image, 4 x 3 kernel, padding (1, 0): weight and activation search of the channel-wise class on fp32 planes.
    W8A16: a_bit 9..31 keeps quantising the input (aq up to 2^30 on the fp32 planes path)."""
    from oracle.ptq4vit_oracle import ConvOracle
    w, bias, x, out, grad = _mk_conv(9, 3, 3, 32, 24, 16, 4, 3, (1, 0))
    hp = dict(HP, w_bit=bits[0], a_bit=bits[1], metric="hessian")
    o = ConvOracle(w, bias, stride=(4, 3), padding=(1, 0), dilation=(1, 1), channelwise=True, **hp)
    res = o.calibration_step2(x, out, grad)
    (w_iv, a_iv, scores, best), kinds = _kinds(eng, lambda: eng.conv_calibrate(
        weight=_t(w), bias=_t(bias), x=_t(x), out=_t(out), grad=_t(grad), stride=(4, 3), padding=(1, 0), dilation=(1, 1),
        channelwise=True, want_scores=True, **hp))
    scores, best = _np(scores), _np(best)
    pairs = []
    for r in range(HP["search_round"]):
        pairs.append((scores[r, 0], best[r, 0], o.trace[2 * r][1]))
        pairs.append((scores[r, 1][:, :1], best[r, 1][:1], o.trace[2 * r + 1][1]))
    what = f"conv w{bits[0]}a{bits[1]}"
    flips = _cmp_tables(pairs, what)
    mult = candidate_grid(HP["eq_alpha"], HP["eq_beta"], HP["eq_n"])
    moved = (assert_on_candidate_grid(_np(w_iv), np.asarray(res["w_interval"]), mult, what + " w_interval", ref_scores=o.trace[-2][1])
             + assert_on_candidate_grid(_np(a_iv), np.asarray(res["a_interval"]), mult, what + " a_interval", ref_scores=o.trace[-1][1]))
    print(f"[route] {what}: {sorted(set(kinds))}")
    assert "k_sweep<float>" in kinds, sorted(set(kinds))
    if flips == 0:
        assert moved == 0, "same selections but different intervals"


# ======================================================================================================================
# c. exact candidate pruning at mixed widths
# ======================================================================================================================
def _three_ways(eng, run):
    """(forced pruned, unpruned, cross-checked) results + the counters and kernels of the forced pruned call."""
    try:
        eng.debug_variant(FORCE_PRUNE)
        eng.prune_counters(reset=True)
        pruned, kinds = _kinds(eng, lambda: run())
        cnt = eng.prune_counters(reset=True)
        eng.debug_variant(FORCE_PRUNE | CROSS_CHECK)
        checked = run()
    finally:
        eng.debug_variant(0)
    full = run(prune=False)
    torch.cuda.synchronize()
    return pruned, full, checked, cnt, kinds


# the smallest batch at which a pass of the shape is staged under forced pruning, measured at both width orders: Linear 4 images
# (788 samples; 1-3: "kept_full_sweep"), the attention matmuls 1 image of 3 heads (197 query rows)
PRUNE_LINEAR = {"K768": dict(b=4, T=197, K=768, N=192, postgelu=False), "K3072-gelu": dict(b=4, T=197, K=3072, N=192, postgelu=True)}


@pytest.mark.parametrize("bits", [(8, 4), (4, 8)], ids=lambda b: f"w{b[0]}a{b[1]}")
@pytest.mark.parametrize("case", list(PRUNE_LINEAR))
def test_candidate_pruning_is_exact_linear_at_mixed_widths(eng, case, bits):
    cfg = PRUNE_LINEAR[case]
    w, bias, x, out, grad = _mk_linear(31, cfg["b"], cfg["T"], cfg["K"], cfg["N"], cfg["postgelu"])
    rng = np.random.default_rng(5)
    heavy = grad.copy().reshape(-1, cfg["N"])
    heavy[rng.choice(heavy.shape[0], size=max(1, heavy.shape[0] // 40), replace=False)] *= 300.0     # a few samples carry the weight
    hp = dict(w_bit=bits[0], a_bit=bits[1], metric="hessian", eq_alpha=0.01, eq_beta=1.2, eq_n=100, search_round=3, n_V=1, n_H=1,
              n_a=1, postgelu=cfg["postgelu"])
    args = dict(weight=_t(w), bias=_t(bias), x=_t(x), out=_t(out), grad=_t(heavy.reshape(grad.shape)))
    pruned, full, checked, cnt, kinds = _three_ways(eng, lambda **k: eng.linear_calibrate(**args, **hp, **k))
    print(f"[prune] linear {case} w{bits[0]}a{bits[1]}: {cnt}, {sorted(set(kinds))}")
    assert cnt["staged"] > 0, cnt
    for k, what in ((0, "w_interval"), (1, "a_interval")):
        _same(pruned[k], full[k], f"pruned vs unpruned {what}"); _same(checked[k], full[k], f"cross-checked vs unpruned {what}")
    assert "k_bound" in kinds, sorted(set(kinds))               # stage B1 of a Linear: both operands quantised in registers


PRUNE_MATMUL = {"qk": dict(kind="qk", b=1, H=3, S=197, D=64), "sos": dict(kind="sv", b=1, H=3, S=197, D=64)}


@pytest.mark.parametrize("bits", [(8, 4), (4, 8)], ids=lambda b: f"A{b[0]}B{b[1]}")
@pytest.mark.parametrize("case", list(PRUNE_MATMUL))
def test_candidate_pruning_is_exact_matmul_at_mixed_widths(eng, case, bits):
    cfg = PRUNE_MATMUL[case]
    A, B, out, grad = _mk_attention(41, cfg["b"], cfg["H"], cfg["S"], cfg["D"], cfg["kind"])
    grad = grad.copy()
    grad[:, :, 0, :] *= 300.0                                     # the class-token query row carries the weight, as in a ViT
    hp = dict(A_bit=bits[0], B_bit=bits[1], metric="hessian", eq_alpha=0.01, eq_beta=1.2, eq_n=100, search_round=3, sos=cfg["kind"] == "sv")
    Bt = _t(np.ascontiguousarray(B.transpose(0, 1, 3, 2))).transpose(-2, -1) if cfg["kind"] == "qk" else _t(B)
    args = dict(A=_t(A), B=Bt, out=_t(out), grad=_t(grad))
    pruned, full, checked, cnt, kinds = _three_ways(eng, lambda **k: eng.matmul_calibrate(**args, **hp, **k))
    print(f"[prune] matmul {case} A{bits[0]}B{bits[1]}: {cnt}, {sorted(set(kinds))}")
    assert cnt["staged"] > 0, cnt
    for k, what in ((0, "A_interval"), (1, "B_interval"), (2, "split")):
        if pruned[k] is not None:
            _same(pruned[k], full[k], f"pruned vs unpruned {what}"); _same(checked[k], full[k], f"cross-checked vs unpruned {what}")
    # stage A / B2 of an attention matmul: the sliced operands are quantised in registers, each with its own quantiser choice
    want = {"k_slice_a", "k_slice_b"} if cfg["kind"] == "qk" else {"k_slice_b"}
    assert want <= set(kinds), sorted(set(kinds))


# ======================================================================================================================
# d. integer planes at every width 2..8
# ======================================================================================================================
def _plane_input(bit, s, seed):
    """257 x 199: random values, the exact half-way values (k + 0.5) s of the whole grid and beyond both clamp ends, the clamp ends
    themselves and far beyond, +0 / -0, and a column of NaN."""
    q = 2 ** (bit - 1)
    x = (np.random.default_rng(seed).standard_normal((257, 199)) * q * s / 2).astype(np.float32)
    k = np.arange(-q - 3, q + 3, dtype=np.float32)
    half = ((k + np.float32(0.5)) * np.float32(s)).astype(np.float32)[:199]
    x[0, :len(half)] = half
    x[1, :len(half)] = np.nextafter(half, np.float32(np.inf))
    x[2, :len(half)] = np.nextafter(half, np.float32(-np.inf))
    x[3, :8] = np.array([0.0, -0.0, (q - 1) * s, q * s, -q * s, (-q - 1) * s, 1e30, -1e30], np.float32)
    x[256, :len(half)] = half                                     # ... and in the last row (a partial row tile)
    x[:, 198] = np.nan
    return x


def _check_plane(got, x, ref, lo, hi, what):
    """Bit-equal to the oracle wherever the input is a number; a NaN input has no grid index (the reference's round / clamp keep
    NaN): it must stay inside the grid and leave its neighbours alone."""
    got, nan = _np(got).astype(np.int32), np.isnan(x)
    np.testing.assert_array_equal(got[~nan], np.asarray(ref)[~nan], err_msg=what)
    assert nan.any() and (got[nan] >= lo).all() and (got[nan] <= hi).all(), what


@pytest.mark.parametrize("bit", range(2, 9))
def test_integer_planes_at_every_width(eng, bit):
    """quantize_i8 and pack_plane_i8 (sym: one scale per 100 rows; twin: the merged post-GELU plane) on lo = -2^(b-1),
    hi = 2^(b-1) - 1: width 8 takes quant16_sat8, every other width quant_fast1 / quant16_any."""
    from oracle.ptq4vit_oracle import POSTGELU_NEG_RANGE, quant_int, twin_planes
    q = 2 ** (bit - 1)
    lo, hi = -q, q - 1
    s = np.array([0.0371, 0.011, 0.5], dtype=np.float32)
    x = _plane_input(bit, s[0], bit)
    rows_s = np.repeat(s, 100)[:257, None]
    with np.errstate(invalid="ignore", over="ignore"):
        ref = quant_int(x, rows_s, lo, hi)
        s_neg = np.float32(POSTGELU_NEG_RANGE / q)
        pos, neg = twin_planes(x, s[0], s_neg, q)
    _check_plane(eng.quantize_i8(_t(x), _t(s), 100, lo, hi), x, ref, lo, hi, f"quantize_i8 {bit} bit")
    plane, padded = eng.pack_plane_i8(_t(x), mode="sym", scales=torch.from_numpy(s), rows_per_scale=100, lo=lo, hi=hi, qmax=q)
    _check_plane(plane, x, ref, lo, hi, f"pack_plane_i8 sym {bit} bit")
    assert not padded[:, 199:].any()
    both, padded = eng.pack_plane_i8(_t(x), mode="twin", scales=torch.tensor([s[0]]), const_scale=float(s_neg), lo=lo, hi=hi, qmax=q)
    _check_plane(both, x, pos + neg, lo, hi, f"pack_plane_i8 twin {bit} bit")
    assert not padded[:, 199:].any()
    ok = ~np.isnan(x)
    assert ref[ok].min() == lo and ref[ok].max() == hi and pos[ok].max() == hi and neg[ok].min() == lo      # both clamps are reached


@pytest.mark.parametrize("bit", range(2, 9))
def test_dual_planes_at_every_width(eng, bit):
    """k_pack_dual: the post-GELU pair ([0, q-1] on the searched scale, [-q, 0] on 0.16997 / q) and the split-of-softmax pair
    (high range x (q-1), low range / (split / (q-1))); at 2 bits q - 1 = 1."""
    from oracle.ptq4vit_oracle import POSTGELU_NEG_RANGE, sos_planes, twin_planes
    q = 2 ** (bit - 1)
    s = np.float32(0.0371)
    x = _plane_input(bit, s, 100 + bit)
    s_neg = np.float32(POSTGELU_NEG_RANGE / q)
    with np.errstate(invalid="ignore", over="ignore"):
        pos, neg = twin_planes(x, s, s_neg, q)
    p1, p2, q1, q2 = eng.debug_pack_dual(_t(x), sos=False, scale=float(s), lo=-q, hi=q - 1, qmax=q, const_scale=float(s_neg))
    _check_plane(p1, x, pos, 0, q - 1, f"dual post-GELU positive plane {bit} bit")
    _check_plane(p2, x, neg, -q, 0, f"dual post-GELU negative plane {bit} bit")
    assert not q1[:, 199:].any() and not q2[:, 199:].any()
    split = np.float32(0.125)
    a_int = split / np.float32(q - 1)
    A = np.abs(x) * np.float32(0.02)                                # softmax-like: mostly far below 1
    k = np.arange(-1, q + 1, dtype=np.float32)
    A[0, :len(k)] = np.clip((k + np.float32(0.5)) * a_int, 0, 1)    # half-way values of the low grid
    A[1, :len(k)] = np.clip((k + np.float32(0.5)) / np.float32(q - 1), 0, 1)     # ... of the high grid
    A[2, :6] = [split, np.nextafter(split, np.float32(0)), np.nextafter(split, np.float32(1)), 0.0, 1.0, split / 2]
    with np.errstate(invalid="ignore"):
        ref_hi, ref_lo = sos_planes(A, split, q)
    p1, p2, q1, q2 = eng.debug_pack_dual(_t(A), sos=True, scale=float(split), lo=0, hi=q - 1, qmax=q)
    _check_plane(p1, A, ref_hi, 0, q - 1, f"dual split-of-softmax high plane {bit} bit")
    _check_plane(p2, A, ref_lo, 0, q - 1, f"dual split-of-softmax low plane {bit} bit")
    if bit == 2:
        assert set(np.unique(ref_hi[~np.isnan(A)])) == {0, 1} and set(np.unique(ref_lo[~np.isnan(A)])) == {0, 1}


# ======================================================================================================================
# e. refused widths
# ======================================================================================================================
BAD = [0, 1, 9]


def _refused(eng, fn, what):
    before = eng.launch_counters()
    with pytest.raises(NotImplementedError, match="bit"):
        fn()
    torch.cuda.synchronize()
    assert eng.launch_counters() == before, f"{what}: launches before the refusal"


@pytest.mark.parametrize("bad", BAD)
@pytest.mark.parametrize("operand", [0, 1])
def test_linear_entry_points_refuse_widths_outside_2_to_8(eng, bad, operand):
    g = load_golden("mixbit_linear_w4a8_hessian_v3")
    args = _linear_args(g)
    args["w_bit" if operand == 0 else "a_bit"] = bad
    what = f"linear {'w_bit' if operand == 0 else 'a_bit'}={bad}"
    _refused(eng, lambda: eng.linear_calibrate(**args), what + " calibrate / workspace")
    step = {k: v for k, v in args.items() if k not in ("eq_alpha", "eq_beta", "search_round")}
    _refused(eng, lambda: eng.LinearStepper(**step), what + " granular")
    _refused(eng, lambda: eng.linear_quant_forward(weight=args["weight"], bias=args["bias"], x=args["x"], w_interval=_t(g["w_interval"]),
                                                   a_interval=_t(g["a_interval"]), w_bit=args["w_bit"], a_bit=args["a_bit"], n_V=3,
                                                   n_H=1, n_a=1), what + " quant_forward")


@pytest.mark.parametrize("bad", BAD)
@pytest.mark.parametrize("operand", [0, 1])
@pytest.mark.parametrize("name", ["mixbit_matmul_qk_a8b4_hessian", "mixbit_matmul_sos_a4b8_hessian", "mixbit_mmblk_qk_a8b4_vA2hA2_vB2hB2"])
def test_matmul_entry_points_refuse_widths_outside_2_to_8(eng, name, bad, operand):
    g = load_golden(name)
    args = _matmul_args(g)
    args["A_bit" if operand == 0 else "B_bit"] = bad
    what = f"{name} {'A_bit' if operand == 0 else 'B_bit'}={bad}"
    _refused(eng, lambda: eng.matmul_calibrate(**args), what + " calibrate / workspace")
    step = {k: v for k, v in args.items() if k not in ("eq_alpha", "eq_beta", "search_round")}
    _refused(eng, lambda: eng.MatMulStepper(**step), what + " granular")
    kw = dict(A=args["A"], B=args["B"], A_interval=_t(np.asarray(g["A_interval"], np.float32)), B_interval=_t(g["B_interval"]),
              split=_t(np.asarray(g["split"], np.float32)) if args["sos"] else None, A_bit=args["A_bit"], B_bit=args["B_bit"], sos=args["sos"])
    if name in MMBLK:
        _refused(eng, lambda: eng.matmul_blocks_quant_forward(blocks=args["blocks"], **kw), what + " quant_forward")
    else:
        _refused(eng, lambda: eng.matmul_quant_forward(**kw), what + " quant_forward")


@pytest.mark.parametrize("field,bad", [("w_bit", 0), ("w_bit", 1), ("w_bit", 9), ("a_bit", 0), ("a_bit", 1)])
def test_conv_entry_points_refuse_widths_outside_their_range(eng, field, bad):
    g = load_golden("mixbit_conv_cw_w4a8_hessian")
    args = _conv_args(g)
    args[field] = bad
    _refused(eng, lambda: eng.conv_calibrate(**args), f"conv {field}={bad} calibrate / workspace")
    step = {k: v for k, v in args.items() if k not in ("eq_alpha", "eq_beta", "search_round")}
    _refused(eng, lambda: eng.ConvStepper(**step), f"conv {field}={bad} granular")


def test_refusals_come_from_the_calibrate_calls_themselves(eng):
    """The Python wrappers above stop at the workspace query.  The C calibrate entry points, alone and as a group member, refuse
    by themselves too: a job prepared at valid widths (real tensors, real workspace) whose descriptor is then changed."""
    from ptq4vit_amd import _lib

    def job(kind, args, **fields):
        j = getattr(eng, kind + "_job")(**args)
        d = j.desc.mm if hasattr(j.desc, "mm") else j.desc
        for k, v in fields.items():
            setattr(d, k, v)
        return j
    lin = _linear_args(load_golden("mixbit_linear_w4a8_hessian_v3"))
    mm = _matmul_args(load_golden("mixbit_matmul_qk_a8b4_hessian"))
    blk = _matmul_args(load_golden("mixbit_mmblk_qk_a8b4_vA2hA2_vB2hB2"))
    cv = _conv_args(load_golden("mixbit_conv_cw_w4a8_hessian"))
    for kind, args, fields in (("linear", lin, dict(a_bit=1)), ("linear", lin, dict(w_bit=9)), ("matmul", mm, dict(A_bit=1)),
                               ("matmul", mm, dict(B_bit=0)), ("matmul", blk, dict(B_bit=1)), ("matmul", blk, dict(A_bit=9)),
                               ("conv", cv, dict(w_bit=1)), ("conv", cv, dict(a_bit=1)), ("conv", cv, dict(w_bit=9))):
        _refused(eng, lambda: eng.run_job(job(kind, args, **fields)), f"{kind} {fields} single call")
        assert _lib.load().p4v_last_error()
    before = eng.launch_counters()
    with pytest.raises((NotImplementedError, RuntimeError), match="bit"):
        eng.calibrate_group([job("matmul", mm, A_bit=1)])
    torch.cuda.synchronize()
    after = eng.launch_counters()
    assert (after["asked"], after["issued"]) == (before["asked"], before["issued"]), (before, after)


def test_granular_entry_points_refuse_by_themselves(eng):
    """The steppers' constructors stop at the workspace query too.  A stepper built at valid widths (real tensors, real
    workspace) whose descriptor is then changed: p4v_amax_init_* and every p4v_*_search_* entry point refuse, nothing launched."""
    drop = ("eq_alpha", "eq_beta", "search_round", "blocks")
    g = load_golden("mixbit_linear_w4a8_hessian_v3")
    args = _linear_args(g)
    st = eng.LinearStepper(**{k: v for k, v in args.items() if k not in drop})
    w, a = st.init_intervals()
    wc, ac = _cands(eng, g["params"], w), _cands(eng, g["params"], a)
    st.d.a_bit = 1
    _refused(eng, st.init_intervals, "p4v_amax_init_linear")
    _refused(eng, lambda: st.search_w(wc, w, a), "p4v_linear_search_w")
    _refused(eng, lambda: st.search_a(ac, w, a), "p4v_linear_search_a")
    g = load_golden("mixbit_conv_cw_w4a8_hessian")
    args = _conv_args(g)
    st = eng.ConvStepper(**{k: v for k, v in args.items() if k not in drop})
    w, a = st.init_intervals()
    wc, ac = _cands(eng, g["params"], w), _cands(eng, g["params"], a)
    st.d.w_bit = 1
    _refused(eng, st.init_intervals, "p4v_amax_init_conv")
    _refused(eng, lambda: st.search_w(wc, w, a), "p4v_conv_search_w_channelwise")
    _refused(eng, lambda: st.search_a(ac, w, a), "p4v_conv_search_a")
    for name in ("mixbit_matmul_qk_a8b4_hessian", "mixbit_matmul_sos_a4b8_hessian"):
        g = load_golden(name)
        args = _matmul_args(g)
        st = eng.MatMulStepper(**{k: v for k, v in args.items() if k not in drop})
        A_iv, B_iv = st.init_intervals()
        Bc = _cands(eng, g["params"], B_iv)
        st.d.B_bit = 9
        _refused(eng, st.init_intervals, "p4v_amax_init_matmul")
        if args["sos"]:
            _refused(eng, st.search_split, "p4v_sos_search_split")
            one = torch.ones(1, device=B_iv.device)
            _refused(eng, lambda: st.search_B(Bc, one, B_iv, split=one), "p4v_matmul_search_B (sos)")
        else:
            _refused(eng, lambda: st.search_A(_cands(eng, g["params"], A_iv), A_iv, B_iv), "p4v_matmul_search_A")
            _refused(eng, lambda: st.search_B(Bc, A_iv, B_iv), "p4v_matmul_search_B")
    g = load_golden("mixbit_mmblk_qk_a8b4_vA2hA2_vB2hB2")
    args = _matmul_args(g)
    st = eng.MatMulStepper(**{k: v for k, v in args.items() if k not in ("eq_alpha", "eq_beta", "search_round")})
    A_iv, B_iv = st.init_intervals()
    H = g["A"].shape[1]
    mult = eng.candidate_multipliers(g["params"]["eq_alpha"], g["params"]["eq_beta"], g["params"]["eq_n"], B_iv.device)
    cands = mult.view(-1, 1) * B_iv.view(H, 2, 2)[:, 0, 0].view(1, H)
    st.bd.mm.A_bit = 1
    _refused(eng, st.init_intervals, "p4v_amax_init_matmul_blocks")
    _refused(eng, lambda: st.search_block("B", 0, 0, cands, A_iv, B_iv), "p4v_matmul_blocks_search B")
    _refused(eng, lambda: st.search_block("A", 1, 1, cands, A_iv, B_iv), "p4v_matmul_blocks_search A")


def test_conv_a_bit_32_and_above_stays_unquantised(eng):
    g = load_golden("mixbit_conv_cw_w4a8_hessian")
    res = {}
    for a_bit in (32, 40):
        args = dict(_conv_args(g), a_bit=a_bit)
        res[a_bit] = eng.conv_calibrate(**args)
    torch.cuda.synchronize()
    _same(res[32][0], res[40][0], "w_interval with a_bit 32 vs 40")
    with pytest.raises(RuntimeError, match="a_bit >= 32"):
        args = dict(_conv_args(g), a_bit=32)
        st = eng.ConvStepper(**{k: v for k, v in args.items() if k not in ("eq_alpha", "eq_beta", "search_round")})
        w, a = st.init_intervals()
        st.search_a(_cands(eng, g["params"], a), w, a)


@pytest.mark.parametrize("bits", [(9, 8), (8, 1), (12, 12)], ids=lambda b: f"{b[0]}-{b[1]}")
def test_module_classes_fall_back_to_their_torch_formulation_outside_2_to_8(eng, bits, monkeypatch):
    """quant_forward of the module classes outside the int8 entry points' widths: the fake-quant fp32 formulation, not an engine
    call -- and its output is the oracle's quant_forward."""
    from oracle.ptq4vit_oracle import LinearOracle, MatMulOracle
    from ptq4vit_amd.quant_layers.linear import PTQSLBatchingQuantLinear
    from ptq4vit_amd.quant_layers.matmul import PTQSLBatchingQuantMatMul
    for fn in ("linear_quant_forward", "matmul_quant_forward", "matmul_blocks_quant_forward"):
        monkeypatch.setattr(eng, fn, lambda **k: pytest.fail("engine call outside 2..8 bits"))
    den = [max(2 ** (b - 1) - 0.5, 1.0) for b in bits]         # (one bit: the grid is {-1, 0}; max / 0.5 would round everything to 0)
    g = load_golden("mixbit_linear_w4a8_hessian_v3")
    w_iv = (np.abs(g["weight"]).reshape(3, -1).max(1) / den[0]).astype(np.float32).reshape(3, 1, 1, 1)
    a_iv = np.full((1, 1), np.abs(g["x"]).max() / den[1], np.float32)
    m = PTQSLBatchingQuantLinear(g["weight"].shape[1], g["weight"].shape[0], w_bit=bits[0], a_bit=bits[1], n_V=3).cuda()
    m.weight.data.copy_(_t(g["weight"])); m.bias.data.copy_(_t(g["bias"]))
    m.w_interval, m.a_interval, m.calibrated, m.mode = _t(w_iv), _t(a_iv), True, "quant_forward"
    o = LinearOracle(g["weight"], g["bias"], w_bit=bits[0], a_bit=bits[1], n_V=3)
    o.w_interval, o.a_interval = w_iv, a_iv
    with torch.no_grad():
        _close(m(_t(g["x"])), o.quant_forward(g["x"]), g["weight"].shape[1], f"linear fallback {bits}")
    g = load_golden("mixbit_matmul_qk_a8b4_hessian")
    H = g["A"].shape[1]
    A_iv = (np.abs(g["A"]).max(axis=(0, 2, 3)) / den[0]).astype(np.float32).reshape(1, H, 1, 1, 1, 1, 1)
    B_iv = (np.abs(g["B"]).max(axis=(0, 2, 3)) / den[1]).astype(np.float32).reshape(1, H, 1, 1, 1, 1, 1)
    mm = PTQSLBatchingQuantMatMul(A_bit=bits[0], B_bit=bits[1])
    mm.n_G_A = mm.n_G_B = H
    mm.A_interval, mm.B_interval, mm.calibrated, mm.mode = _t(A_iv), _t(B_iv), True, "quant_forward"
    o = MatMulOracle(A_bit=bits[0], B_bit=bits[1])
    o._padding(g["A"], g["B"])
    o.A_interval, o.B_interval = A_iv, B_iv
    ref = o.quant_forward(g["A"], g["B"])
    assert np.abs(ref).max() > 0
    with torch.no_grad():
        _close(mm(_t(g["A"]), _t(g["B"])), ref, g["A"].shape[-1], f"matmul fallback {bits}")
