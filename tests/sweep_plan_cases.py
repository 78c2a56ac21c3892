"""Shared by tests/test_hip_sweep_plan.py and tools/plan_dump.py: the smallest calibration per sweep kernel family
(csrc/p4v_api.hip, plan_sweep; DESIGN.md s5 "pass -> kernel"), with seeded inputs.

Linear layers: 2 images x 64 tokens, hessian, W8A8, 100 candidates, one round (weight search, then activation search).
`run(eng, prune)` makes the call and returns its result tensors (intervals; without pruning also the score tables and the
selections).  Every case but "bound" is meant for prune=False (desc.reserved bit 3); "bound" is the 650-row layer of
tests/test_hip_bound_kernels.py under variant 8388608, whose pruned passes run k_bound as stage B1."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

SEARCH = dict(eq_alpha=0.01, eq_beta=1.2, eq_n=100, search_round=1)
LOOSE = 8388608
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _cuda(t):
    return None if t is None else t.cuda()


def _grad(shape, g, token_dim):
    """raw_grad of the magnitude the reference's KL gradient has, the first token's rows heavy"""
    grad = torch.randn(shape, generator=g) * 1e-10
    idx = [slice(None)] * len(shape)
    idx[token_dim] = 0
    grad[tuple(idx)] *= 300.0
    return grad


GRADS = ("seeded", "none", "adversarial", "nan")


def grad_of(kind, grad, out):
    """the raw_grad a case hands to the engine: "seeded" the generator's own, "none" no tensor, "adversarial" 1 / (|raw_out| + 1e-3)
    -- finite, and it reverses the ranking of the elements by |raw_out|, so a kernel of a raw_out-weighted metric that read it would
    move its argmax by many entries --, "nan" all NaN.  A metric other than hessian must not read any of them
    (include/ptq4vit_hip.h, d_grad)."""
    assert kind in GRADS, kind
    if kind == "none":
        return None
    if kind == "adversarial":
        return 1.0 / (out.abs() + 1e-3)
    if kind == "nan":
        return torch.full_like(out, float("nan"))
    return grad


def linear_inputs(K, N, *, seed, images=2, tokens=64, postgelu=False):
    """(weight, bias, x, out, grad) of a seeded Linear layer, on the host"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(images, tokens, K, generator=g)
    if postgelu:
        x = F.gelu(1.5 * x)
    w = torch.randn(N, K, generator=g) * 0.05 * torch.linspace(0.6, 1.5, N)[:, None]
    b = torch.randn(N, generator=g) * 0.1
    out = F.linear(x, w, b)
    return w, b, x, out, _grad(out.shape, g, 1)


def _linear(K, N, *, seed, images=2, tokens=64, n_V=1, postgelu=False, variant=0, metric="hessian"):
    def run(eng, prune, grad="seeded"):
        w, b, x, out, gr = linear_inputs(K, N, seed=seed, images=images, tokens=tokens, postgelu=postgelu)
        eng.debug_variant(variant)
        try:
            res = eng.linear_calibrate(weight=_cuda(w), bias=_cuda(b), x=_cuda(x), out=_cuda(out), grad=_cuda(grad_of(grad, gr, out)), w_bit=8, a_bit=8,
                                       metric=metric, n_V=n_V, n_H=1, n_a=1, postgelu=postgelu, prune=prune, want_scores=not prune,
                                       **SEARCH)
        finally:
            eng.debug_variant(0)
        return [t for t in res if t is not None]
    return run


def matmul_inputs(M, K, N, *, seed, sos=False, batch=2, heads=2):
    """(A, B, out, grad) of a seeded MatMul, on the host: q.k^T with k transposed in memory, or softmax rows times v"""
    g = torch.Generator().manual_seed(seed)
    if sos:
        A = torch.softmax(torch.randn(batch, heads, M, K, generator=g) * 3.0, dim=-1)
        B = torch.randn(batch, heads, K, N, generator=g)
    else:
        A = torch.randn(batch, heads, M, K, generator=g)
        B = torch.randn(batch, heads, N, K, generator=g).transpose(-2, -1)
    out = A @ B
    return A, B, out, _grad(out.shape, g, 2)


def _matmul(M, K, N, *, seed, sos=False, batch=2, heads=2, metric="hessian"):
    def run(eng, prune, grad="seeded"):
        A, B, out, gr = matmul_inputs(M, K, N, seed=seed, sos=sos, batch=batch, heads=heads)
        res = eng.matmul_calibrate(A=_cuda(A), B=_cuda(B), out=_cuda(out), grad=_cuda(grad_of(grad, gr, out)), A_bit=8, B_bit=8, metric=metric,
                                   sos=sos, prune=prune, want_scores=not prune, **SEARCH)
        return [t for t in res if t is not None]
    return run


def _matmul_blocks(name, *, metric=None):
    """the fixture's inputs and blocks; `metric` replaces the fixture's own (a hessian fixture brings its raw_grad: by default it is
    passed under hessian only, a `grad` kind of GRADS passes that one under any metric)"""
    def run(eng, prune, grad=None):
        z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
        p = json.loads(str(z["params"]))
        p["metric"] = metric or p["metric"]
        t = lambda k: torch.from_numpy(np.ascontiguousarray(z[k])).cuda()
        blocks = (p.get("n_V_A", 1), p.get("n_H_A", 1), p.get("n_V_B", 1), p.get("n_H_B", 1))
        gr = t("grad") if p["metric"] == "hessian" else None
        if grad is not None:
            gr = _cuda(grad_of(grad, torch.from_numpy(np.ascontiguousarray(z["grad"])), torch.from_numpy(np.ascontiguousarray(z["out"]))))
        res = eng.matmul_calibrate(A=t("A"), B=t("B"), out=t("out"), grad=gr,
                                   A_bit=p["A_bit"], B_bit=p["B_bit"], metric=p["metric"], eq_alpha=p["eq_alpha"], eq_beta=p["eq_beta"],
                                   eq_n=p["eq_n"], search_round=p["search_round"], sos=p["sos"], blocks=blocks, want_scores=True)
        return [t for t in res if t is not None]
    return run


def conv_inputs(*, seed, images=2, size=32, patch=16):
    """(weight, bias, x, out, grad) of a seeded 16-filter patch embedding (by default 2 x 3 x 32 x 32, 16 x 16 patches), on the host"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(images, 3, size, size, generator=g)
    w = torch.randn(16, 3, patch, patch, generator=g) * 0.02 * torch.linspace(0.5, 2.0, 16).view(-1, 1, 1, 1)
    b = torch.randn(16, generator=g) * 0.02
    out = F.conv2d(x, w, b, stride=patch)
    return w, b, x, out, torch.randn(out.shape, generator=g) * 1e-10


def _conv(*, seed, metric="hessian"):
    def run(eng, prune, grad="seeded"):
        w, b, x, out, gr = conv_inputs(seed=seed)
        res = eng.conv_calibrate(weight=_cuda(w), bias=_cuda(b), x=_cuda(x), out=_cuda(out), grad=_cuda(grad_of(grad, gr, out)), stride=(16, 16),
                                 padding=(0, 0), dilation=(1, 1), w_bit=8, a_bit=32, metric=metric, prune=prune,
                                 want_scores=not prune, **SEARCH)
        return [t for t in res if t is not None]
    return run


# (name, maker, its arguments, pruned): the twelve shapes; every maker also takes `metric` (tests/metric_grid_cases.py)
SHAPES = [
    ("linear_k192_n128", _linear, ((192, 128), dict(seed=1)), False),
    ("linear_k128_n128", _linear, ((128, 128), dict(seed=2)), False),
    ("linear_k1024_n64", _linear, ((1024, 64), dict(seed=3)), False),
    ("postgelu_k1024_n64", _linear, ((1024, 64), dict(seed=4, postgelu=True)), False),
    ("linear_k1088_n64", _linear, ((1088, 64), dict(seed=5)), False),
    ("linear_k192_n120_nV3", _linear, ((192, 120), dict(seed=6, n_V=3)), False),
    ("matmul_qk_49", _matmul, ((49, 64, 49), dict(seed=7)), False),
    ("matmul_qk_120", _matmul, ((120, 64, 120), dict(seed=8)), False),
    ("matmul_sos_49", _matmul, ((49, 49, 64), dict(seed=9, sos=True)), False),
    ("conv_patch16_a32", _conv, ((), dict(seed=10)), False),
    ("bound_650x96_k192", _linear, ((192, 96), dict(seed=11, images=10, tokens=65, variant=LOOSE)), True),
    ("mmblk_qk_hessian_vA2hA2_vB2hB3", _matmul_blocks, (("mmblk_qk_hessian_vA2hA2_vB2hB3",), {}), False),
]

# (name, run, pruned): `pruned` cases run with the exact candidate pruning on, the others with desc.reserved bit 3
CASES = [(name, make(*args, **kw), pruned) for name, make, (args, kw), pruned in SHAPES]


def run_case(eng, run, prune, **kw):
    """One case with launch records: (result tensors, [(kernel, stage, grid_x, grid_z)], launch counters, prune counters); the
    launch counters also carry the pass memo's (hits, misses) as "memo".  `grad=` one of GRADS: the raw_grad handed to the engine."""
    eng.launch_counters(reset=True)
    eng.prune_counters(reset=True)
    eng.stats_reset()
    eng.stats_enable(True)
    try:
        res = run(eng, prune, **kw)
        torch.cuda.synchronize()
        st = eng.stats_get()
        recs = [(r["kernel"], r["stage"], r["grid_x"], r["grid_z"]) for r in eng.stats_launches()]
    finally:
        eng.stats_enable(False)
    return res, recs, dict(eng.launch_counters(), memo=(int(st["memo_hits"]), int(st["memo_misses"]))), eng.prune_counters()
