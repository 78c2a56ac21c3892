"""GPU: the weight-source rule through the entry points the metric grid does not call -- raw_grad is read if and only if the metric
is hessian (include/ptq4vit_hip.h, d_grad).  Under L2_norm, L1_norm, linear_weighted_L2_norm and square_weighted_L2_norm a call
with no raw_grad, with the generator's and with the adversarial one (tests/sweep_plan_cases.py, grad_of: 1 / (|raw_out| + 1e-3))
must return the same bits:

  * the granular calls p4v_linear_search_w / _a, p4v_matmul_search_A / _B, p4v_sos_search_split and p4v_conv_search_w_channelwise,
    with score tables (full sweeps) and without (the passes may be pruned: variant 8388608);
  * ONE p4v_calibrate_group call whose members mix the metrics, hessian among them, pruned by force.

Shapes: the 650-row Linear, the 65-row MatMuls and the 640-pixel conv of tests/pruned_pass_cases.py."""
import pytest
import torch

from tests.pruned_pass_cases import METRICS, ROUNDS
from tests.sweep_plan_cases import GRADS, LOOSE, conv_inputs, grad_of, linear_inputs, matmul_inputs

pytestmark = pytest.mark.gpu

KINDS = tuple(k for k in GRADS if k != "nan")          # "seeded", "none", "adversarial"


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    return engine


def _cuda(t):
    return None if t is None else t.cuda()


def _bits(ts):
    return [None if t is None else (tuple(t.shape), t.detach().cpu().numpy().tobytes()) for t in ts]


def _cands(eng, iv):
    return eng.candidate_multipliers(ROUNDS["eq_alpha"], ROUNDS["eq_beta"], ROUNDS["eq_n"], iv.device).view(-1, 1) * iv.reshape(1, -1)


def _linear_steps(eng, metric, kind, scores):
    w, b, x, out, grad = linear_inputs(192, 96, seed=41, images=10, tokens=65)
    st = eng.LinearStepper(weight=_cuda(w), bias=_cuda(b), x=_cuda(x), out=_cuda(out), grad=_cuda(grad_of(kind, grad, out)), w_bit=8, a_bit=8,
                           metric=metric, eq_n=ROUNDS["eq_n"], n_V=1, n_H=1, n_a=1)
    w_iv, a_iv = st.init_intervals()
    wc, ac = _cands(eng, w_iv), _cands(eng, a_iv)
    res = []
    for _ in range(2):
        w_iv, sw, bw = st.search_w(wc, w_iv, a_iv, want_scores=scores)
        a_iv, sa, ba = st.search_a(ac, w_iv, a_iv, want_scores=scores)
        res += [w_iv, sw, bw, a_iv, sa, ba]
    return res


def _matmul_steps(eng, metric, kind, scores, sos):
    A, B, out, grad = matmul_inputs(65, 65, 64, seed=48, sos=True) if sos else matmul_inputs(65, 64, 65, seed=46)
    st = eng.MatMulStepper(A=_cuda(A), B=_cuda(B), out=_cuda(out), grad=_cuda(grad_of(kind, grad, out)), A_bit=8, B_bit=8, metric=metric,
                           eq_n=ROUNDS["eq_n"], sos=sos)
    A_iv, B_iv = st.init_intervals()
    Bc = _cands(eng, B_iv)
    if sos:
        split, A_iv, ss, bs = st.search_split(want_scores=scores)
        B_iv, sb, bb = st.search_B(Bc, A_iv, B_iv, split=split, want_scores=scores)
        return [split, A_iv, ss, bs, B_iv, sb, bb]
    A_iv, sa, ba = st.search_A(_cands(eng, A_iv), A_iv, B_iv, want_scores=scores)
    B_iv, sb, bb = st.search_B(Bc, A_iv, B_iv, want_scores=scores)
    return [A_iv, sa, ba, B_iv, sb, bb]


def _conv_steps(eng, metric, kind, scores):
    w, b, x, out, grad = conv_inputs(seed=49, images=10, size=64, patch=8)
    st = eng.ConvStepper(weight=_cuda(w), bias=_cuda(b), x=_cuda(x), out=_cuda(out), grad=_cuda(grad_of(kind, grad, out)), stride=(8, 8),
                         padding=(0, 0), dilation=(1, 1), w_bit=8, a_bit=32, metric=metric, eq_n=ROUNDS["eq_n"])
    w_iv, a_iv = st.init_intervals()
    return list(st.search_w(_cands(eng, w_iv), w_iv, a_iv, want_scores=scores))


STEPS = {"linear": _linear_steps, "matmul_qk": lambda *a: _matmul_steps(*a, sos=False), "matmul_sos": lambda *a: _matmul_steps(*a, sos=True),
         "conv": _conv_steps}


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("module", sorted(STEPS))
def test_granular_calls_do_not_read_raw_grad(eng, module, metric):
    eng.debug_variant(LOOSE)
    try:
        for scores in (True, False):
            runs = {kind: _bits(STEPS[module](eng, metric, kind, scores)) for kind in KINDS}
            torch.cuda.synchronize()
            for kind in KINDS:
                assert runs[kind] == runs["none"], f"{module} {metric}, score tables {scores}: the {kind} raw_grad changes the result"
    finally:
        eng.debug_variant(0)
        eng.release_workspace()


def _group_jobs(eng, kind):
    """eight members: the 650-row Linear under the five difference metrics, q.k^T, the split-of-softmax p.v and the conv under one
    each; the hessian member keeps its own raw_grad, the others get `kind`"""
    jobs = []
    w, b, x, out, grad = linear_inputs(192, 96, seed=41, images=10, tokens=65)
    for metric in METRICS + ("hessian",):
        gr = grad if metric == "hessian" else grad_of(kind, grad, out)
        jobs.append(eng.linear_job(weight=_cuda(w), bias=_cuda(b), x=_cuda(x), out=_cuda(out), grad=_cuda(gr), w_bit=8, a_bit=8, metric=metric,
                                   n_V=1, n_H=1, n_a=1, **ROUNDS))
    for sos, metric, shape, seed in ((False, "L2_norm", (65, 64, 65), 46), (True, "linear_weighted_L2_norm", (65, 65, 64), 48)):
        A, B, out_m, grad_m = matmul_inputs(*shape, seed=seed, sos=sos)
        jobs.append(eng.matmul_job(A=_cuda(A), B=_cuda(B), out=_cuda(out_m), grad=_cuda(grad_of(kind, grad_m, out_m)), A_bit=8, B_bit=8,
                                   metric=metric, sos=sos, **ROUNDS))
    w, b, x, out_c, grad_c = conv_inputs(seed=49, images=10, size=64, patch=8)
    jobs.append(eng.conv_job(weight=_cuda(w), bias=_cuda(b), x=_cuda(x), out=_cuda(out_c), grad=_cuda(grad_of(kind, grad_c, out_c)), stride=(8, 8),
                             padding=(0, 0), dilation=(1, 1), w_bit=8, a_bit=32, metric="square_weighted_L2_norm", **ROUNDS))
    return jobs


def test_one_group_call_that_mixes_the_metrics_does_not_read_raw_grad(eng):
    eng.debug_variant(LOOSE)
    try:
        runs = {}
        for kind in KINDS:
            eng.launch_counters(reset=True)
            eng.prune_counters(reset=True)
            done = eng.calibrate_group(_group_jobs(eng, kind))
            torch.cuda.synchronize()
            assert eng.launch_counters()["groups"] == 1 and eng.prune_counters()["staged"] > 0
            runs[kind] = [_bits(j.outputs) for j in done]
        for kind in KINDS:
            for i, (a, b) in enumerate(zip(runs[kind], runs["none"])):
                assert a == b, f"group member {i}: the {kind} raw_grad changes the result"
    finally:
        eng.debug_variant(0)
        eng.release_workspace()
