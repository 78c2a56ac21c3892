"""Shared by tests/test_hip_metric_grid.py and tools/plan_dump.py: the twelve shapes of tests/sweep_plan_cases.py (one per sweep
kernel family, each with its pruning setting) under the four difference metrics that the other bit-wise dumps do not run --
L2_norm, L1_norm, linear_weighted_L2_norm, square_weighted_L2_norm; the cases of sweep_plan_cases / search_round_cases run
hessian and cosine.  The metric decides the epilogue instance of every sweep kernel (EpiMode, csrc/p4v_kernels.h) and the
metric weight of its prologue: hessian shares EPI_SQ_W with square_weighted_L2_norm, the other three have instances of their own.

`run(eng, prune)` is the maker of sweep_plan_cases with `metric` set; `oracle(name, metric)` is the numpy reference of the same
call: (reference intervals ..., [score table per pass]) by kind of layer."""
import json
import os

import numpy as np

from tests.sweep_plan_cases import GOLDEN, SEARCH, SHAPES, _conv, _linear, _matmul, _matmul_blocks, conv_inputs, linear_inputs, matmul_inputs

METRICS = ("L2_norm", "L1_norm", "linear_weighted_L2_norm", "square_weighted_L2_norm")

# (name, metric, run, pruned)
CASES = [(name, metric, make(*args, metric=metric, **kw), pruned) for name, make, (args, kw), pruned in SHAPES for metric in METRICS]
IDS = [f"{name}-{metric}" for name, metric, _, _ in CASES]


def oracle(name, metric):
    """dict(kind, intervals = [reference interval arrays in the order the engine returns them; None: not searched], tables = [[candidates][blocks]
    score table of every pass, in order], sos)"""
    from oracle.ptq4vit_oracle import ConvOracle, LinearOracle, MatMulOracle
    make, (args, kw) = next((m, a) for n, m, a, _ in SHAPES if n == name)
    np_ = lambda *ts: [t.numpy() for t in ts]
    if make is _linear:
        gen = {k: v for k, v in kw.items() if k in ("seed", "images", "tokens", "postgelu")}
        w, b, x, out, _ = np_(*linear_inputs(*args, **gen))
        o = LinearOracle(w, b, w_bit=8, a_bit=8, metric=metric, n_V=kw.get("n_V", 1), postgelu=kw.get("postgelu", False), **SEARCH)
        o.calibration_step2(x, out, None)
        return dict(kind="linear", intervals=[o.w_interval, o.a_interval], tables=[t for _, t in o.trace], sos=False)
    if make is _conv:
        w, b, x, out, _ = np_(*conv_inputs(**kw))
        o = ConvOracle(w, b, stride=16, w_bit=8, a_bit=32, metric=metric, **SEARCH)
        o.calibration_step2(x, out, None)
        return dict(kind="conv", intervals=[o.w_interval, None], tables=[t for _, t in o.trace], sos=False)   # a_bit = 32: no a search
    if make is _matmul:
        sos = kw.get("sos", False)
        A, B, out, _ = np_(*matmul_inputs(*args, **kw))
        o = MatMulOracle(A_bit=8, B_bit=8, metric=metric, sos=sos, **SEARCH)
    else:
        assert make is _matmul_blocks
        z = np.load(os.path.join(GOLDEN, args[0] + ".npz"), allow_pickle=False)
        p = json.loads(str(z["params"]))
        sos = p["sos"]
        A, B, out = z["A"], z["B"], z["out"]
        o = MatMulOracle(A_bit=p["A_bit"], B_bit=p["B_bit"], metric=metric, sos=sos, eq_alpha=p["eq_alpha"], eq_beta=p["eq_beta"],
                         eq_n=p["eq_n"], search_round=p["search_round"],
                         **{k: p.get(k, 1) for k in ("n_V_A", "n_H_A", "n_V_B", "n_H_B")})
    res = o.calibration_step2(A, B, out, None)
    return dict(kind="matmul", intervals=[res["A_interval"], res["B_interval"]] + ([res["split"]] if sos else []),
                tables=[t for _, t in o.trace], sos=sos, search=dict(eq_alpha=o.eq_alpha, eq_beta=o.eq_beta, eq_n=o.eq_n))
