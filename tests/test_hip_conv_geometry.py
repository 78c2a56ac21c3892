"""GPU: the Conv2d search beyond unpadded square patch embeddings -- rectangular images / kernels / strides, asymmetric
padding, dilation on one axis, ResNet-style stems, patches that are entirely padding, a filter that is all zero.

The engine's conv view (csrc/p4v_kernels.h::pack_load: y = oy * sh - ph + ki * dh, 0 outside the image; k_gather_im2col for the
slice rows of the pruned passes) is symmetric in h and w on every shipped patch embedding, so a swapped ph / pw, a dilation on the
wrong axis or fw used for fh passes every other test.  Here:
  a. the reference's own runs on such geometries (tests/golden/convgeo_*.npz): score tables, selections, intervals;
  b. the same fixtures through the granular entry points and the module classes;
  c. seeded random geometries against the numpy oracle (tests/conv_cases.py; the oracle's im2col is pinned to F.unfold on the CPU);
  d. the exact pruning on padded convs, with a zero filter (NaN score column: the k_prune_hull fallback);
  e. a group call of differently shaped convs;
  f. the im2col gather itself against F.unfold, element for element;
  g. a geometry whose dilated kernel exceeds the padded input is refused.
Tolerances are those of tests/helpers.py (SCORE_RTOL, TIE_RTOL, the candidate grid); nothing is read from the reference tree."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conv_cases import case_id, conv_geometry_cases, dims, make_tensors
from tests.helpers import assert_argmax_tie_aware, candidate_grid, golden_names, load_golden
from tests.test_hip_parity import _cmp_tables, _t

pytestmark = pytest.mark.gpu

PTQ4VIT = dict(metric="hessian", eq_alpha=0.01, eq_beta=1.2, eq_n=100, search_round=3)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    return engine


def _split(g):
    """(geometry keywords, channelwise, the remaining hyper-parameters) of a convgeo fixture."""
    p = dict(g["params"])
    p.pop("kind")
    geo = {k: tuple(p.pop(k)) for k in ("stride", "padding", "dilation")}
    return geo, p.pop("channelwise"), p


def _tensors(g):
    return dict(weight=_t(g["weight"]), bias=_t(g["bias"]), x=_t(g["x"]), out=_t(g["out"]), grad=_t(g["grad"]))


def _pairs(scores, best, tables, R, aq):
    per_round = 2 if aq else 1
    pairs = []
    for r in range(R):
        pairs.append((scores[r, 0], best[r, 0], tables[r * per_round]))
        if aq:
            pairs.append((scores[r, 1][:, :1], best[r, 1][:1], tables[r * per_round + 1]))
    return pairs


def _same(a, b, what):
    np.testing.assert_array_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy(), err_msg=what)


# ---- a. the reference's runs, fused call with score tables ----------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names("convgeo_"))
def test_conv_geometry_vs_reference_golden(eng, name):
    """Same bar as test_hip_parity.py::test_conv_vs_reference_golden.  The zero-filter fixtures (g, h) add: that channel's score
    column is NaN in every table exactly where the reference's is (with a_bit = 8 the whole activation table), the first NaN wins
    the argmax (candidate 0), the channel's interval is exactly 0."""
    g = load_golden(name)
    geo, cw, p = _split(g)
    R, aq = p["search_round"], p["a_bit"] < 32
    w_iv, a_iv, scores, best = eng.conv_calibrate(**_tensors(g), **geo, channelwise=cw, want_scores=True, **p)
    torch.cuda.synchronize()
    scores, best = scores.cpu().numpy(), best.cpu().numpy()
    pairs = _pairs(scores, best, g["scores"], R, aq)
    for i, (got, _, ref) in enumerate(pairs):
        ref2 = ref.reshape(ref.shape[0], -1)
        np.testing.assert_array_equal(np.isnan(got[: ref2.shape[0], : ref2.shape[1]]), np.isnan(ref2), err_msg=f"{name}[{i}] NaN pattern")
    flips = _cmp_tables(pairs, name)
    w_iv, a_iv = w_iv.cpu().numpy(), a_iv.cpu().numpy()
    for c in g.get("zero_filters", []):
        assert w_iv[int(c)] == 0.0, f"{name}: interval of the zero filter {int(c)} is {w_iv[int(c)]!r}"
    print(f"[parity] {name}: {flips} near-tie flips in {len(pairs)} tables")
    if flips == 0:
        np.testing.assert_array_equal(w_iv, np.asarray(g["w_interval"]).reshape(-1))
        if aq:
            np.testing.assert_array_equal(a_iv, np.asarray(g["a_interval"]).reshape(-1))


# ---- b. the same fixtures through the other entry points ------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names("convgeo_"))
def test_conv_geometry_granular_sequence_is_bit_identical_to_the_fused_call(eng, name):
    """p4v_amax_init_conv, p4v_conv_search_w_*, p4v_conv_search_a one by one: every table, index and interval of the fused call."""
    g = load_golden(name)
    geo, cw, p = _split(g)
    R, aq = p["search_round"], p["a_bit"] < 32
    common = dict(**_tensors(g), **geo, w_bit=p["w_bit"], a_bit=p["a_bit"], metric=p["metric"], eq_n=p["eq_n"], channelwise=cw)
    w_f, a_f, sc_f, be_f = eng.conv_calibrate(eq_alpha=p["eq_alpha"], eq_beta=p["eq_beta"], search_round=R, want_scores=True, **common)
    st = eng.ConvStepper(**common)
    w, a = st.init_intervals()
    mult = eng.candidate_multipliers(p["eq_alpha"], p["eq_beta"], p["eq_n"], w.device)
    wc, ac = mult.view(-1, 1) * w.reshape(1, -1), mult.view(-1, 1) * a.reshape(1, -1)
    for r in range(R):
        w, sw, bw = st.search_w(wc, w, a, want_scores=True)
        _same(sw, sc_f[r, 0], f"{name} round {r} w scores"); _same(bw, be_f[r, 0], f"{name} round {r} w argmax")
        if aq:
            a, sa, ba = st.search_a(ac, w, a, want_scores=True)
            _same(sa[:, :1], sc_f[r, 1][:, :1], f"{name} round {r} a scores"); _same(ba[:1], be_f[r, 1][:1], f"{name} round {r} a argmax")
    _same(w, w_f, f"{name} w_interval"); _same(a, a_f, f"{name} a_interval")


def _module(g, geo, cw, p):
    from ptq4vit_amd.quant_layers.conv import BatchingEasyQuantConv2d, ChannelwiseBatchingQuantConv2d
    oc, ic, kh, kw = g["weight"].shape
    m = (ChannelwiseBatchingQuantConv2d if cw else BatchingEasyQuantConv2d)(ic, oc, (kh, kw), **geo, **p).cuda()
    m.weight.data.copy_(_t(g["weight"])); m.bias.data.copy_(_t(g["bias"]))
    m.raw_input, m.raw_out, m.raw_grad = _t(g["x"]), _t(g["out"]), _t(g["grad"])
    return m


@pytest.mark.parametrize("name", golden_names("convgeo_"))
def test_conv_geometry_module_classes_reproduce_the_fused_call_and_the_reference_output(eng, name):
    """ChannelwiseBatchingQuantConv2d / BatchingEasyQuantConv2d built with the fixture's stride, padding and dilation:
    calibration_step2() and the per-pass methods give the fused call's intervals bit for bit; quant_forward with the REFERENCE's
    intervals gives the reference's output -- rtol 1e-4 / atol 1e-5, the bar of the Conv2d module quant_forward check in
    test_hip_planes.py (test_ptqsl_conv_own_search_vs_reference) and of the oracle's on the CPU; a zero filter's channel is NaN in
    both."""
    g = load_golden(name)
    geo, cw, p = _split(g)
    w_f, a_f, _, _ = eng.conv_calibrate(**_tensors(g), **geo, channelwise=cw, **p)
    fused = _module(g, geo, cw, p)
    fused.calibration_step2()
    m = _module(g, geo, cw, p)
    m._initialize_calib_parameters()
    m._initialize_intervals()
    mult = eng.candidate_multipliers(m.eq_alpha, m.eq_beta, m.eq_n, m.weight.device)
    wc = mult.view(-1, 1, 1, 1, 1) * m.w_interval.unsqueeze(0)                     # reference conv.py:594
    ac = mult * m.a_interval.reshape(-1)[0]
    for _ in range(m.search_round):
        m._search_best_w_interval(wc)
        if m.a_bit < 32:
            m._search_best_a_interval(ac)                                           # reference conv.py:600
    for mod, what in ((fused, "calibration_step2"), (m, "per-pass methods")):
        _same(mod.w_interval.reshape(-1), w_f, f"{name} {what} w_interval")
        _same(mod.a_interval.reshape(-1), a_f, f"{name} {what} a_interval")
        assert tuple(mod.w_interval.shape) == ((g["weight"].shape[0], 1, 1, 1) if cw else (1, 1, 1, 1))
    # quant_forward on the reference's intervals (independent of where a near-tie fell in the search)
    fused.w_interval = _t(np.asarray(g["w_interval"], dtype=np.float32)).reshape(fused.w_interval.shape)
    if p["a_bit"] < 32:
        fused.a_interval = _t(np.asarray(g["a_interval"], dtype=np.float32)).reshape(())
    fused.mode = "quant_forward"
    with torch.no_grad():
        got = fused(_t(g["x"])).cpu().numpy()
    ref = g["quant_forward"]
    assert got.shape == ref.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=f"{name} quant_forward NaN pattern")
    keep = [c for c in range(ref.shape[1]) if c not in {int(z) for z in g.get("zero_filters", [])}]
    assert not np.isnan(ref[:, keep]).any()
    print(f"[quant_forward] {name}: max |diff| / max |ref| = {np.abs(got[:, keep] - ref[:, keep]).max() / np.abs(ref[:, keep]).max():.2e}")
    np.testing.assert_allclose(got[:, keep], ref[:, keep], rtol=1e-4, atol=1e-5)


# ---- c. seeded random geometries against the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", conv_geometry_cases(), ids=case_id)
def test_random_conv_geometries_vs_oracle(eng, cfg):
    """Whole score tables and tie-aware selection of both searches, two rounds, as test_random_linear_geometries_vs_oracle."""
    from oracle.ptq4vit_oracle import ConvOracle
    w, bias, x, out, grad = make_tensors(cfg)
    geo = dict(stride=cfg["stride"], padding=cfg["padding"], dilation=cfg["dilation"])
    hp = dict(w_bit=cfg["w_bit"], a_bit=cfg["a_bit"], metric=cfg["metric"], eq_alpha=0.01, eq_beta=1.2, eq_n=cfg["eq_n"], search_round=2)
    o = ConvOracle(w, bias, channelwise=cfg["channelwise"], **geo, **hp)
    res = o.calibration_step2(x, out, grad)
    w_iv, a_iv, scores, best = eng.conv_calibrate(weight=_t(w), bias=_t(bias), x=_t(x), out=_t(out), grad=_t(grad),
                                                  channelwise=cfg["channelwise"], want_scores=True, **geo, **hp)
    torch.cuda.synchronize()
    aq = cfg["a_bit"] < 32
    pairs = _pairs(scores.cpu().numpy(), best.cpu().numpy(), [t for _, t in o.trace], 2, aq)
    flips = _cmp_tables(pairs, "random-conv")
    fh, fw, L, K, M = dims(cfg)
    print(f"[parity] conv {case_id(cfg)}: L {L} K {K} M {M}: {flips} near-tie flips")
    if flips == 0:
        np.testing.assert_array_equal(w_iv.cpu().numpy(), np.asarray(res["w_interval"]).reshape(-1))
        if aq:
            np.testing.assert_array_equal(a_iv.cpu().numpy(), np.asarray(res["a_interval"]).reshape(-1))


# ---- d. exact pruning on padded convs -------------------------------------------------------------------------------------------
PRUNE_CASES = [
    dict(b=4, ic=8, H=24, W=20, oc=64, k=(3, 3), stride=(1, 1), padding=(1, 1), dilation=(1, 1), channelwise=True, w_bit=8, metric="hessian"),
    dict(b=8, ic=3, H=224, W=224, oc=64, k=(7, 7), stride=(2, 2), padding=(3, 3), dilation=(1, 1), channelwise=True, w_bit=8, metric="hessian"),
    dict(b=6, ic=5, H=40, W=36, oc=48, k=(3, 5), stride=(1, 2), padding=(2, 1), dilation=(2, 1), channelwise=False, w_bit=6, metric="L2_norm"),
]


def _prune_tensors(cfg, seed=13, zero_filters=()):
    c = dict(cfg, seed=seed)
    w, bias, x, out, grad = make_tensors(c)
    if zero_filters:
        w[list(zero_filters)] = 0.0
        out = F.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(bias), c["stride"], c["padding"], c["dilation"]).numpy()
    rng = np.random.default_rng(seed + 1)
    mask = rng.random((c["b"], 1) + out.shape[2:]) < 0.03                 # a few pixels carry the weight
    heavy = np.where(mask, grad * 300.0, grad).astype(np.float32)
    return w, bias, x, out, grad, heavy


@pytest.mark.parametrize("cfg", PRUNE_CASES, ids=lambda c: f"{'cw' if c['channelwise'] else 'lw'}-{c['metric'][:4]}-b{c['b']}ic{c['ic']}-{c['H']}x{c['W']}-oc{c['oc']}-k{c['k'][0]}x{c['k'][1]}")
def test_candidate_pruning_is_exact_on_padded_convs(eng, cfg):
    """The slice rows of a padded / strided / dilated conv are gathered by k_gather_im2col: forced pruning (variant 8388608), the
    engine's own choice, prune=False and the engine's cross-check (variant 134217728) select the same intervals, bit for bit, on a
    flat and a concentrated gradient profile; the forced call really ran in stages.  The 224 x 224 stem's default call is also
    followed against the torch-CPU port of the reference."""
    from tests.follow import follow_conv
    fh, fw, L, K, M = dims(cfg)
    slice_rows = min(-(-max(1, M // 16) // 256) * 256, -(-M // 256) * 256)
    assert M >= 640 and slice_rows * 5 <= M * 2, "not a pruning-eligible size"
    w, bias, x, out, grad, heavy = _prune_tensors(cfg)
    hp = dict(w_bit=cfg["w_bit"], a_bit=32, metric=cfg["metric"], eq_alpha=0.01, eq_beta=1.2, eq_n=100, search_round=3,
              stride=cfg["stride"], padding=cfg["padding"], dilation=cfg["dilation"], channelwise=cfg["channelwise"])
    for g_, prof in ((grad, "flat"), (heavy, "concentrated")):
        args = dict(weight=_t(w), bias=_t(bias), x=_t(x), out=_t(out), grad=_t(g_))
        try:
            eng.debug_variant(8388608)
            eng.prune_counters(reset=True)
            pruned = eng.conv_calibrate(**args, **hp)
            torch.cuda.synchronize()
            cnt = eng.prune_counters(reset=True)
            eng.debug_variant(134217728)
            checked = eng.conv_calibrate(**args, **hp)
        finally:
            eng.debug_variant(0)
        auto = eng.conv_calibrate(**args, **hp)
        full = eng.conv_calibrate(prune=False, **args, **hp)
        torch.cuda.synchronize()
        assert cnt["staged"] > 0, f"{prof}: the forced call did not run in stages: {cnt}"
        for got, what in ((pruned, "forced"), (auto, "engine's own choice"), (checked, "cross-check")):
            assert torch.equal(got[0], full[0]), f"{prof}: {what} selected other intervals at {(got[0] != full[0]).sum().item()} blocks"
            assert torch.equal(got[1], full[1])
    if cfg["H"] == 224:
        t = torch.from_numpy
        fhp = {k: hp[k] for k in ("w_bit", "a_bit", "metric", "eq_alpha", "eq_beta", "eq_n")}
        flips, _ = follow_conv(eng, weight=t(w), bias=t(bias), x=t(x), out=t(out), grad=t(heavy), stride=cfg["stride"], padding=cfg["padding"],
                               dilation=cfg["dilation"], hp=fhp, channelwise=cfg["channelwise"], what="7x7 stride-2 stem", expect_pruned=False)
        print(f"[follow] 7x7 stride-2 stem, default call: {flips} near-tie flips of {cfg['oc']} channels")


def test_zero_filter_at_a_pruning_eligible_size(eng):
    """A filter that is all zero (a pruned channel under channel-wise quantisation) has interval 0 and a NaN score for every
    candidate: k_prune_hull's "NaN anywhere disables the pruning".  Pruned == unpruned bit for bit, that channel's interval is 0,
    the others follow the oracle (tie-aware)."""
    from oracle.ptq4vit_oracle import ConvOracle
    from tests.follow import _lookup
    cfg, zero = PRUNE_CASES[0], 5
    w, bias, x, out, grad, heavy = _prune_tensors(cfg, seed=17, zero_filters=(zero,))
    geo = dict(stride=cfg["stride"], padding=cfg["padding"], dilation=cfg["dilation"])
    hp = dict(w_bit=8, a_bit=32, metric="hessian", eq_alpha=0.01, eq_beta=1.2, eq_n=100)
    args = dict(weight=_t(w), bias=_t(bias), x=_t(x), out=_t(out), grad=_t(heavy))
    try:
        eng.debug_variant(8388608)
        eng.prune_counters(reset=True)
        pruned = eng.conv_calibrate(**args, **geo, **hp, search_round=3, channelwise=True)
        torch.cuda.synchronize()
        cnt = eng.prune_counters(reset=True)
        eng.debug_variant(134217728)
        checked = eng.conv_calibrate(**args, **geo, **hp, search_round=3, channelwise=True)
    finally:
        eng.debug_variant(0)
    auto = eng.conv_calibrate(**args, **geo, **hp, search_round=3, channelwise=True)
    full = eng.conv_calibrate(prune=False, **args, **geo, **hp, search_round=3, channelwise=True)
    tabs = eng.conv_calibrate(want_scores=True, **args, **geo, **hp, search_round=1, channelwise=True)
    torch.cuda.synchronize()
    print(f"[prune] zero filter, forced: {cnt}")
    assert cnt["staged"] > 0, cnt
    for got, what in ((pruned, "forced"), (auto, "engine's own choice"), (checked, "cross-check")):
        assert torch.equal(got[0], full[0]), f"{what}: other intervals at {(got[0] != full[0]).sum().item()} channels"
    w_iv = full[0].cpu().numpy()
    assert w_iv[zero] == 0.0 and (np.delete(w_iv, zero) > 0).all()
    sc = tabs[2][0, 0].cpu().numpy()
    assert np.isnan(sc[:, zero]).all() and not np.isnan(np.delete(sc, zero, axis=1)).any() and int(tabs[3][0, 0, zero]) == 0
    o = ConvOracle(w, bias, channelwise=True, search_round=1, **geo, **hp)
    with np.errstate(invalid="ignore", divide="ignore"):
        o.calibration_step2(x, out, heavy)
    table = o.trace[0][1]
    assert np.isnan(table[:, zero]).all()
    mult = candidate_grid(0.01, 1.2, 100)
    w0 = (np.abs(w).max(axis=(1, 2, 3)) / np.float32(127.5)).astype(np.float32)
    cands = mult[:, None] * w0[None, :]
    keep = np.array([c for c in range(cfg["oc"]) if c != zero])
    idx = _lookup(cands[:, keep], w_iv[keep], "zero-filter conv")
    flips = assert_argmax_tie_aware(idx, table[:, keep], what="zero-filter conv, pruned weight search")
    print(f"[prune] zero filter: {flips} near-tie flips of {keep.size} channels")


# ---- e. group call --------------------------------------------------------------------------------------------------------------
def _conv_job_kw(cfg, seed, a_bit=32):
    w, bias, x, out, grad = make_tensors(dict(cfg, seed=seed))
    grad = grad * np.float32(1e-7)
    return dict(weight=_t(w), bias=_t(bias), x=_t(x), out=_t(out), grad=_t(grad), stride=cfg["stride"], padding=cfg["padding"],
                dilation=cfg["dilation"], w_bit=cfg["w_bit"], a_bit=a_bit, channelwise=cfg["channelwise"],
                **dict(PTQ4VIT, metric=cfg["metric"]))


def _group_specs():
    from tests.test_hip_group import _linear_kw
    g = torch.Generator().manual_seed(21)
    return [("conv", _conv_job_kw(PRUNE_CASES[0], 31, a_bit=8)),                              # 3x3 pad 1, a_bit = 8: both searches
            ("linear", _linear_kw(g, 4, 197, 192, 192, 1)),
            ("conv", _conv_job_kw(PRUNE_CASES[2], 32)),                                       # padded, dilated, rectangular, layer-wise
            ("conv", _conv_job_kw(dict(b=2, ic=3, H=64, W=48, oc=40, k=(7, 7), stride=(2, 2), padding=(3, 3), dilation=(1, 1),
                                       channelwise=True, w_bit=8, metric="hessian"), 33)),    # small 7x7 stride-2 stem
            ("conv", _conv_job_kw(dict(b=3, ic=4, H=15, W=19, oc=9, k=(3, 2), stride=(2, 2), padding=(2, 0), dilation=(1, 3),
                                       channelwise=True, w_bit=6, metric="cosine"), 34))]     # cosine: per-image view, never pruned


def test_group_of_differently_shaped_convs_equals_the_single_calls(eng):
    """p4v_calibrate_group over convs of different geometry (one padded and dilated, one with a_bit = 8) and a Linear: the single
    calls' intervals bit for bit; again under the engine's cross-check (variant 134217728)."""
    from tests.test_hip_group import _jobs
    specs = _group_specs()
    single = [eng.run_job(j) for j in _jobs(eng, specs)]
    torch.cuda.synchronize()
    grouped = eng.calibrate_group(_jobs(eng, specs))
    torch.cuda.synchronize()
    try:
        eng.debug_variant(134217728)
        checked = eng.calibrate_group(_jobs(eng, specs))
        torch.cuda.synchronize()
    finally:
        eng.debug_variant(0)
    n = 0
    for (kind, _), a, b, c in zip(specs, single, grouped, checked):
        for x, y, z in zip(a.outputs, b.outputs, c.outputs):
            assert torch.equal(x, y), f"{kind}: single {x.flatten()[:4].tolist()} vs grouped {y.flatten()[:4].tolist()}"
            assert torch.equal(x, z), f"{kind}: single {x.flatten()[:4].tolist()} vs grouped under the cross-check {z.flatten()[:4].tolist()}"
            n += x.numel()
    print(f"[group] {len(specs)} members, {n} interval scalars bit-identical")


# ---- f. the im2col view itself --------------------------------------------------------------------------------------------------
def _gather_geometries():
    out = [((c["b"], c["ic"], c["H"], c["W"]), c["k"], c["stride"], c["padding"], c["dilation"], case_id(c)) for c in conv_geometry_cases()]
    for n in golden_names("convgeo_"):
        g = load_golden(n)
        p = g["params"]
        out.append((g["x"].shape, tuple(g["weight"].shape[2:]), tuple(p["stride"]), tuple(p["padding"]), tuple(p["dilation"]), n))
    return out


@pytest.mark.parametrize("geo", _gather_geometries(), ids=lambda t: t[5])
def test_im2col_gather_equals_unfold(eng, geo):
    """k_gather_im2col (p4v_debug_gather_im2col) is a copy: the gathered rows are exactly those rows of
    F.unfold(x, ...).transpose(1, 2) -- the first and the last row, rows of the last image, unordered and repeated indices."""
    shape, k, s, pd, d, _ = geo
    rng = np.random.default_rng(sum(shape) + k[0] * 7 + k[1])
    x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()
    ref = F.unfold(x, k, dilation=d, padding=pd, stride=s).transpose(1, 2)                  # (b, L, K)
    b, L, K = ref.shape
    ref = ref.reshape(b * L, K)
    M = b * L
    last_image = np.arange((b - 1) * L, M)
    idx = np.concatenate([[0, M - 1], last_image[:: max(1, L // 7)], rng.integers(0, M, size=min(M, 200)), [M - 1, 0]]).astype(np.int32)
    got = eng.debug_gather_im2col(x, torch.from_numpy(idx).cuda(), kernel_size=k, stride=s, padding=pd, dilation=d)
    torch.cuda.synchronize()
    assert got.shape == (idx.size, K)
    assert torch.equal(got, ref[torch.from_numpy(idx).long().cuda()]), f"{(got != ref[torch.from_numpy(idx).long().cuda()]).sum().item()} elements differ"
    if M <= 4096:                                                                            # the whole matrix, in order
        allrows = eng.debug_gather_im2col(x, torch.arange(M, dtype=torch.int32, device="cuda"), kernel_size=k, stride=s, padding=pd, dilation=d)
        assert torch.equal(allrows, ref)


# ---- g. a dilated kernel larger than the padded input ---------------------------------------------------------------------------
def test_kernel_larger_than_the_padded_input_is_refused(eng):
    """H = 6, k = 7, pad 0, stride 2: (6 - 6 - 1) / 2 is -1 / 2 -- floor gives an output size of 0 (torch raises), truncation
    toward zero gave 1.  Both p4v_conv_workspace_bytes and p4v_conv_calibrate must answer P4V_ERR_INVALID.  (out / grad are
    [b, oc, 1, 1]: the size the truncating code derived, so nothing it did could read outside an allocation.)"""
    from ptq4vit_amd import _lib
    lib = _lib.load()
    b, ic, oc = 2, 3, 4
    with pytest.raises(RuntimeError):
        F.conv2d(torch.zeros(b, ic, 6, 6), torch.zeros(oc, ic, 7, 7), None, 2)
    g = torch.Generator().manual_seed(3)
    w, bias, x = torch.randn(oc, ic, 7, 7, generator=g).cuda(), torch.randn(oc, generator=g).cuda(), torch.randn(b, ic, 6, 6, generator=g).cuda()
    out, grad = torch.randn(b, oc, 1, 1, generator=g).cuda(), torch.randn(b, oc, 1, 1, generator=g).cuda()
    for (H, W, kh, kw) in ((6, 6, 7, 7), (6, 8, 7, 3), (8, 6, 3, 7)):          # both axes, then each axis alone
        d = _lib.ConvDesc(b, ic, H, W, oc, kh, kw, 2, 2, 0, 0, 1, 1, 8, 32, _lib.METRICS["hessian"], 100, 1, 1, 0, 1, 0)
        assert lib.p4v_conv_workspace_bytes(C.byref(d)) == 0
        assert b"bad geometry" in lib.p4v_last_error()
    d = _lib.ConvDesc(b, ic, 6, 6, oc, 7, 7, 2, 2, 0, 0, 1, 1, 8, 32, _lib.METRICS["hessian"], 100, 1, 1, 0, 1, 0)
    mult = eng.candidate_multipliers(0.01, 1.2, 100, x.device)
    w_iv, a_iv = torch.full((oc,), -1.0, device="cuda"), torch.full((1,), -1.0, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    p = eng.ptr
    rc = lib.p4v_conv_calibrate(C.byref(d), p(w), p(bias), p(x), p(out), p(grad), p(mult), p(w_iv), p(a_iv), None, None, p(ws), ws.numel(),
                                eng.stream_ptr(x.device))
    torch.cuda.synchronize()
    assert rc == -1 and b"bad geometry" in lib.p4v_last_error(), (rc, lib.p4v_last_error())
    assert bool((w_iv == -1.0).all()) and bool((a_iv == -1.0).all()), "a refused call wrote its outputs"
    with pytest.raises(RuntimeError, match="bad geometry"):
        eng.conv_calibrate(weight=w, bias=bias, x=x, out=out, grad=grad, stride=(2, 2), padding=(0, 0), dilation=(1, 1), w_bit=8, a_bit=32,
                           channelwise=True, **PTQ4VIT)
    # the smallest valid neighbour is still accepted: H = 7, k = 7 -> one output pixel
    d_ok = _lib.ConvDesc(b, ic, 7, 7, oc, 7, 7, 2, 2, 0, 0, 1, 1, 8, 32, _lib.METRICS["hessian"], 100, 1, 1, 0, 1, 0)
    assert lib.p4v_conv_workspace_bytes(C.byref(d_ok)) > 0
