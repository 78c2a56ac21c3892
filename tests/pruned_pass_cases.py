"""Shared by tests/test_hip_pruned_stages.py and tools/plan_dump.py: the smallest calibration per branch of the pruned drivers
(csrc/p4v_api.hip: plan_prune, run_pass_pruned, run_sos_split_pruned; DESIGN.md s5.1 "exact candidate pruning"), three search
rounds each, W8A8, hessian, 100 candidates, seeded inputs (the generators of tests/sweep_plan_cases.py).

The slice rules give the sizes: a Linear is staged from 640 samples (5 k <= 2 M with k >= 256), tries the quarter slice from
M = 4 112 (k_cap >= 512) and plans a second tier from M = 2 048 (k2 = rup(M / 4, 256) >= 2 k_cap); a MatMul from 64 query rows.
Which branch a Linear takes depends on the share of the metric weight (raw_grad^2 summed per sample) its slice holds: the cases
state the share they need as (slice rows, lower bound, upper bound) and `run` asserts it on the host before the call.

`run(eng, mode, prune=True)` makes ONE call and returns (intervals, tables):
  "default"  the pass memo is on, so the pruned passes may read their survivors back (host_sync_ok)
  "nomemo"   desc.reserved bit 1: the host does not read the survivors, stage B2 is always launched and the merge decides
  "xcheck"   the default call with variant bit 134217728: every pruned pass is followed by its full sweep, the engine compares
prune=False (desc.reserved bit 3) is the same call with full sweeps only: the reference of the intervals.

`run(..., want_scores=True)` asks for the score tables as well (no pass is eligible then: with prune=False the reference of the
TOTALS, tests/test_hip_prune_premises.py).

ZERO_REST_CASES (their own list: the EXPECTED literals of tests/test_hip_pruned_stages.py cover CASES): one case per pairing of
a stage-A kernel with the kernel of the totals, raw_grad EXACTLY zero outside the rows the slice takes (`zero_rest`: that many
heaviest samples of a Linear / output pixels of a Conv, query rows per (image, head) of a MatMul) -- the slice's sum and the
total are then the same sum of the same terms, and all that is left between them is the arithmetic of the two kernels.

METRIC_CASES: seven of the cases again (the forced ones: their staging does not depend on a share of raw_grad) under the four
difference metrics that read no raw_grad -- `metric_case(name, metric, grad_given)` makes the run; grad_given False: no tensor,
True: the case's own raw_grad, "adversarial": 1 / (|raw_out| + 1e-3) (sweep_plan_cases.grad_of).  `metric_oracle(name, metric)`
is the numpy reference of that call."""
import torch

from tests.search_round_cases import ROUNDS, _call, _cuda, run_case  # noqa: F401  (run_case: re-exported)
from tests.sweep_plan_cases import LOOSE, conv_inputs, grad_of, linear_inputs, matmul_inputs

MODES = ("default", "nomemo", "xcheck")
XCHECK = 134217728
XCHECKED = ("lin650_cls", "lin650_nV3", "qk65", "sos65")


def slice_share(grad, k):
    """share of the metric weight in the k heaviest samples of a Linear (what k_mass_fraction measures for a k-row slice)"""
    m = (grad.double() ** 2).sum(-1).flatten()
    return float(torch.topk(m, k).values.sum() / m.sum())


def _linear_grad(grad, shape, kind, spread, seed):
    """"cls": the class-token-heavy raw_grad of the generator; "flat": every sample alike; "spread": per-sample log-normal"""
    g = torch.Generator().manual_seed(seed + 1000)
    if kind == "flat":
        return torch.randn(shape, generator=g) * 1e-10
    if kind == "spread":
        return torch.randn(shape, generator=g) * 1e-10 * torch.exp(spread * torch.randn(shape[0], shape[1], 1, generator=g))
    return grad


def zero_rest_rows(grad, k, kind):
    """raw_grad with everything but the k heaviest rows (by raw_grad^2, the hessian weight) set to exactly 0 -- "linear": rows =
    samples [images][tokens] of [..., N]; "matmul": k query rows of every (image, head) of [b][H][M][N]; "conv": rows = output
    pixels (image, y, x) of [b][oc][fh][fw].  The share of the weight in those rows is asserted to be exactly 1."""
    g = grad.clone()
    if kind == "matmul":
        m = (g.double() ** 2).sum(-1)                                        # [b][H][M]
        keep = torch.zeros_like(m, dtype=torch.bool).scatter_(-1, torch.topk(m, k, dim=-1).indices, True)
        g[~keep] = 0.0
        m = (g.double() ** 2).sum(-1)
        outside = m.masked_fill(keep, 0.0).sum(-1)                            # the weight the slice does not hold: exactly none
        assert bool((1.0 - outside / m.sum(-1) == 1.0).all()) and bool((outside == 0).all()) and bool(((m > 0).sum(-1) <= k).all())
        return g
    m = (g.double() ** 2).sum(1 if kind == "conv" else -1)                   # conv: [b][fh][fw]; linear: [images][tokens]
    keep = torch.zeros(m.numel(), dtype=torch.bool)
    keep[torch.topk(m.flatten(), k).indices] = True
    keep = keep.reshape(m.shape)
    if kind == "conv":
        g = g * keep[:, None].to(g.dtype)
    else:
        g[~keep] = 0.0
    m = (g.double() ** 2).sum(1 if kind == "conv" else -1)
    outside = float(m[~keep].sum())
    assert 1.0 - outside / float(m.sum()) == 1.0 and outside == 0.0 and int((m > 0).sum()) <= k
    return g


def _given(grad_given, grad, out):
    return grad_of({False: "none", True: "seeded"}.get(grad_given, grad_given), grad, out)


def _linear(K, N, *, seed, images, tokens, grad="cls", spread=0.0, shares=(), n_V=1, postgelu=False, variant=0, tuning=(), scores=False,
            metric="hessian", grad_given=True, zero_rest=0):
    def run(eng, mode, prune=True, want_scores=False):
        w, b, x, out, gr = linear_inputs(K, N, seed=seed, images=images, tokens=tokens, postgelu=postgelu)
        gr = _linear_grad(gr, out.shape, grad, spread, seed)
        if zero_rest:
            gr = zero_rest_rows(gr, zero_rest, "linear")
        for k, lo, hi in shares if metric == "hessian" else ():     # (the shares are those of raw_grad^2: the hessian weight)
            assert lo <= slice_share(gr, k) < hi, (k, lo, slice_share(gr, k), hi)
        gr = _given(grad_given, gr, out)
        eng.debug_variant(variant | (XCHECK if mode == "xcheck" else 0))
        for key, value in tuning:
            eng.debug_tuning(key, value)
        try:
            job = eng.linear_job(weight=_cuda(w), bias=_cuda(b), x=_cuda(x), out=_cuda(out), grad=_cuda(gr), w_bit=8, a_bit=8,
                                 metric=metric, n_V=n_V, n_H=1, n_a=1, postgelu=postgelu, want_scores=scores or want_scores, prune=prune, **ROUNDS)
            return _call(eng, job, mode)
        finally:
            eng.debug_variant(0)
            for key, _ in tuning:
                eng.debug_tuning(key, 0)
    return run


def _matmul(M, K, N, *, seed, sos=False, metric="hessian", grad_given=True, zero_rest=0):
    def run(eng, mode, prune=True, want_scores=False):
        A, B, out, grad = matmul_inputs(M, K, N, seed=seed, sos=sos)
        if zero_rest:
            grad = zero_rest_rows(grad, zero_rest, "matmul")
        grad = _given(grad_given, grad, out)
        eng.debug_variant(LOOSE | (XCHECK if mode == "xcheck" else 0))
        try:
            job = eng.matmul_job(A=_cuda(A), B=_cuda(B), out=_cuda(out), grad=_cuda(grad), A_bit=8, B_bit=8, metric=metric, sos=sos,
                                 prune=prune, want_scores=want_scores, **ROUNDS)
            return _call(eng, job, mode)
        finally:
            eng.debug_variant(0)
    return run


def _conv(*, seed, a_bit, metric="hessian", grad_given=True, zero_rest=0):
    def run(eng, mode, prune=True, want_scores=False):
        w, b, x, out, grad = conv_inputs(seed=seed, images=10, size=64, patch=8)
        if zero_rest:
            grad = zero_rest_rows(grad, zero_rest, "conv")
        grad = _given(grad_given, grad, out)
        eng.debug_variant(LOOSE | (XCHECK if mode == "xcheck" else 0))
        try:
            job = eng.conv_job(weight=_cuda(w), bias=_cuda(b), x=_cuda(x), out=_cuda(out), grad=_cuda(grad), stride=(8, 8), padding=(0, 0),
                               dilation=(1, 1), w_bit=8, a_bit=a_bit, metric=metric, prune=prune, want_scores=want_scores, **ROUNDS)
            return _call(eng, job, mode)
        finally:
            eng.debug_variant(0)
    return run


L650 = dict(images=10, tokens=65)        # 650 samples: one 256-row slice
L4137 = dict(images=21, tokens=197)      # 4 137 samples: a 512-row slice, tried as 128 rows first
L2048 = dict(images=16, tokens=128)      # 2 048 samples: a 256-row slice and a 512-row second tier

# (name, run)
CASES = [
    # the 650-row Linear: the engine's own decision on a class-token profile and on a flat one (slice loose: full sweeps), the flat
    # one staged by force (many survivors), three score blocks (stage B1 on the synthetic candidate), the post-GELU twin
    ("lin650_cls", _linear(192, 96, seed=41, shares=[(256, 0.97, 1.0)], **L650)),
    ("lin650_flat", _linear(192, 96, seed=41, grad="flat", shares=[(256, 0.0, 0.5)], **L650)),
    ("lin650_flat_forced", _linear(192, 96, seed=41, grad="flat", shares=[(256, 0.0, 0.5)], variant=LOOSE, **L650)),
    ("lin650_nV3", _linear(192, 96, seed=42, n_V=3, variant=LOOSE, **L650)),
    ("postgelu650", _linear(192, 96, seed=45, postgelu=True, variant=LOOSE, **L650)),
    # the quarter slice kept (it holds >= 0.97 of the weight) and rejected (the full slice is ranked again and holds >= 0.5)
    ("lin4137_quarter", _linear(64, 64, seed=43, shares=[(128, 0.97, 1.0)], **L4137)),
    ("lin4137_spread", _linear(64, 64, seed=43, grad="spread", spread=1.1, shares=[(128, 0.0, 0.97), (512, 0.5, 1.0)], **L4137)),
    # the second tier: a first slice with 0.5 .. 0.9 of the weight and at least two survivors (tuning 13 = 2)
    ("lin2048_tier2", _linear(64, 96, seed=44, n_V=3, grad="spread", spread=0.8, shares=[(256, 0.5, 0.9)], tuning=[(13, 2)], **L2048)),
    # MatMul, 2 x 2 heads, 65 query rows: q.k^T with head_dim 64 (stage A in one kernel on both sides) and 128; the split search
    ("qk65", _matmul(65, 64, 65, seed=46)),
    ("qk65_d128", _matmul(65, 128, 65, seed=47)),
    ("sos65", _matmul(65, 65, 64, seed=48, sos=True)),
    # Conv: 10 x 3 x 64 x 64, 16 filters of 8 x 8, stride 8 -- 640 output pixels; fp32 planes (a_bit 32) and int8
    ("conv640_a32", _conv(seed=49, a_bit=32)),
    ("conv640_a8", _conv(seed=50, a_bit=8)),
    # score tables asked for: no pass is eligible
    ("lin650_scores", _linear(192, 96, seed=41, scores=True, **L650)),
]


# (name, run, the pairing the case is there for): raw_grad zero outside the slice's rows.  A Linear of 650 / 2 048 samples slices
# 256 rows, the 4 137-sample one tries 128 first and -- without the pass memo -- takes 512, which hold the same 128 rows and 384
# of weight zero; a MatMul slices 16 query rows per (image, head); the Conv's 640 output pixels slice 256.  The second tier runs
# only on a first slice with less than 0.9 of the weight, so its case keeps 512 rows -- the second slice -- and spreads the weight.
ZERO_REST_CASES = [
    ("lin650_zero_rest", _linear(192, 96, seed=41, zero_rest=256, **L650), "k_sweep6"),
    ("lin650_nV3_zero_rest", _linear(192, 96, seed=42, n_V=3, variant=LOOSE, zero_rest=256, **L650), "k_sweep6, three score blocks"),
    ("postgelu650_zero_rest", _linear(192, 96, seed=45, postgelu=True, variant=LOOSE, zero_rest=256, **L650), "twin k_sweep2"),
    ("lin4137_zero_rest", _linear(64, 64, seed=43, zero_rest=128, **L4137), "k_sweep4/5"),
    ("lin2048_zero_rest", _linear(64, 96, seed=44, n_V=3, zero_rest=256, **L2048), "k_sweep8"),
    ("lin2048_tier2_zero_rest", _linear(64, 96, seed=44, n_V=3, grad="spread", spread=0.8, shares=[(256, 0.5, 0.9)],
                                        tuning=[(13, 2)], zero_rest=512, **L2048), "k_sweep8, second tier"),
    ("qk65_zero_rest", _matmul(65, 64, 65, seed=46, zero_rest=16), "k_slice_a / k_slice_b with k_sweep9"),
    ("qk65_d128_zero_rest", _matmul(65, 128, 65, seed=47, zero_rest=16), "k_sweep2"),
    ("sos65_zero_rest", _matmul(65, 65, 64, seed=48, sos=True, zero_rest=16), "k_sos_split"),
    ("conv640_a32_zero_rest", _conv(seed=49, a_bit=32, zero_rest=256), "conv, fp32 planes"),
    ("conv640_a8_zero_rest", _conv(seed=50, a_bit=8, zero_rest=256), "conv, int8 planes"),
]


def modes_of(name):
    return tuple(m for m in MODES if m != "xcheck" or name in XCHECKED)


METRICS = ("L2_norm", "L1_norm", "linear_weighted_L2_norm", "square_weighted_L2_norm")
GRADS_GIVEN = (False, True, "adversarial")

# name -> (maker, arguments, keywords): the rows of CASES that prune by force, without their shares of raw_grad.  Under these
# metrics they reach what the single pruned Linear of the metric grid does not: the slice kernels (k_slice_a, k_slice_b), the
# pruned split search, the conv slice (k_gather_im2col), the synthetic candidate of three score blocks, the twin.
METRIC_SPECS = {
    "lin650_flat_forced": (_linear, (192, 96), dict(seed=41, grad="flat", variant=LOOSE, **L650)),
    "lin650_nV3": (_linear, (192, 96), dict(seed=42, n_V=3, variant=LOOSE, **L650)),
    "postgelu650": (_linear, (192, 96), dict(seed=45, postgelu=True, variant=LOOSE, **L650)),
    "qk65": (_matmul, (65, 64, 65), dict(seed=46)),
    "sos65": (_matmul, (65, 65, 64), dict(seed=48, sos=True)),
    "conv640_a32": (_conv, (), dict(seed=49, a_bit=32)),
    "conv640_a8": (_conv, (), dict(seed=50, a_bit=8)),
}
METRIC_CASES = [(name, metric) for name in METRIC_SPECS for metric in METRICS]


def metric_case(name, metric, grad_given):
    make, args, kw = METRIC_SPECS[name]
    return make(*args, metric=metric, grad_given=grad_given, **kw)


def metric_oracle(name, metric):
    """the numpy reference of metric_case(name, metric, .): (the intervals in the order the engine returns them; None: not searched, sos)"""
    from oracle.ptq4vit_oracle import ConvOracle, LinearOracle, MatMulOracle
    make, args, kw = METRIC_SPECS[name]
    np_ = lambda *ts: [t.numpy() for t in ts]
    if make is _linear:
        w, b, x, out, _ = np_(*linear_inputs(*args, seed=kw["seed"], images=kw["images"], tokens=kw["tokens"], postgelu=kw.get("postgelu", False)))
        o = LinearOracle(w, b, w_bit=8, a_bit=8, metric=metric, n_V=kw.get("n_V", 1), postgelu=kw.get("postgelu", False), **ROUNDS)
        o.calibration_step2(x, out, None)
        return [o.w_interval, o.a_interval], False
    if make is _conv:
        w, b, x, out, _ = np_(*conv_inputs(seed=kw["seed"], images=10, size=64, patch=8))
        o = ConvOracle(w, b, stride=8, w_bit=8, a_bit=kw["a_bit"], metric=metric, **ROUNDS)
        o.calibration_step2(x, out, None)
        return [o.w_interval, o.a_interval if kw["a_bit"] < 32 else None], False
    sos = kw.get("sos", False)
    A, B, out, _ = np_(*matmul_inputs(*args, seed=kw["seed"], sos=sos))
    o = MatMulOracle(A_bit=8, B_bit=8, metric=metric, sos=sos, **ROUNDS)
    res = o.calibration_step2(A, B, out, None)
    return [res["A_interval"], res["B_interval"]] + ([res["split"]] if sos else []), sos
