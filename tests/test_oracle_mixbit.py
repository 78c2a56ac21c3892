"""Mixed and low bit widths on the CPU: the numpy oracle and the torch port against fixtures the reference itself produced with
w_bit != a_bit / A_bit != B_bit (tests/golden/mixbit_*.npz: oracle/gen_golden.py::gen_mixed_bits, tools/gen_golden_mmblk.py mixbit).

Bar as in tests/test_oracle_golden.py: every score table the reference fed to argmax within SCORE_RTOL, selections equal or
near-ties by the reference's own scores, intervals bit-identical, the quantised output to fp32 GEMM noise.  On top of it:
  gap          every column of every table of a fixture is decided by >= 2.5e-4 relative (> SCORE_RTOL): a right implementation
               cannot flip a selection, so NO differing selection is tolerated on these fixtures (tests/test_hip_mixbit.py too)
  sensitivity  the oracle with the two widths EXCHANGED gives tables further than 10 x SCORE_RTOL from the fixture's and other
               intervals: an implementation that hands one operand the other's width fails, it does not merely risk failing
"""
import os

import numpy as np
import pytest

from oracle.ptq4vit_oracle import ConvOracle, LinearOracle, MatMulOracle
from tests.helpers import GOLDEN, SCORE_RTOL, assert_argmax_tie_aware, assert_scores_close, golden_names, load_golden

NAMES = golden_names("mixbit_")
LINEAR = [n for n in NAMES if n.startswith(("mixbit_linear_", "mixbit_postgelu_"))]
MATMUL = [n for n in NAMES if n.startswith("mixbit_matmul_")]
MMBLK = [n for n in NAMES if n.startswith("mixbit_mmblk_")]
CONV = [n for n in NAMES if n.startswith("mixbit_conv_")]
MIN_GAP = 2.5e-4


def bits_of(p):
    return (p["w_bit"], p["a_bit"]) if "w_bit" in p else (p["A_bit"], p["B_bit"])


def test_the_fixture_set():
    """Twelve fixtures (the two cosine cases of the plan cannot meet the gap condition: see gen_golden.MIXBIT_CASES), every one
    with two different widths, an 8-bit operand next to a sub-8-bit one in each, both orders for every layer kind, 2 bits once
    per Linear / MatMul."""
    assert len(NAMES) == 12 and sorted(LINEAR + MATMUL + MMBLK + CONV) == NAMES, NAMES
    seen = {}
    for n in NAMES:
        g = load_golden(n)
        p = g["params"]
        x, y = bits_of(p)
        assert x != y and 8 in (x, y) and min(x, y) >= 2, n
        kind = "postgelu" if p.get("postgelu") else "sos" if p.get("sos") else p["kind"]
        seen.setdefault(kind, set()).add(x < y)
        assert os.path.getsize(os.path.join(GOLDEN, n + ".npz")) <= 100 * 1024, n
    assert seen == {k: {True, False} for k in ("linear", "postgelu", "conv")} | {"matmul": {False}, "sos": {True}}, seen
    assert {bits_of(load_golden(n)["params"]) for n in LINEAR} >= {(4, 8), (8, 4), (2, 8)}
    assert {bits_of(load_golden(n)["params"]) for n in MATMUL} == {(8, 4), (4, 8), (2, 8)}
    for n in MMBLK:
        p = load_golden(n)["params"]
        assert p["n_V_B"] == p["n_H_B"] == 2 and (p["sos"] or p["n_V_A"] == p["n_H_A"] == 2)


def column_gaps(table):
    t = np.asarray(table, dtype=np.float64)
    t = t.reshape(t.shape[0], -1)
    top = np.sort(t, axis=0)[-2:]
    return (top[1] - top[0]) / np.maximum(np.abs(top[1]), 1e-300)


@pytest.mark.parametrize("name", NAMES)
def test_every_selection_of_the_fixture_is_decided_by_more_than_the_score_tolerance(name):
    g = load_golden(name)
    assert MIN_GAP > SCORE_RTOL
    for i, t in enumerate(g["scores"]):
        assert not np.isnan(t).any()
        gap = column_gaps(t).min()
        assert gap >= MIN_GAP, f"{name}[{i}]: a column is decided by {gap:.2e} < {MIN_GAP}"


def _check_trace(trace, g, name):
    assert len(trace) == len(g["scores"]), f"{name}: {len(trace)} searches vs {len(g['scores'])}"
    for i, ((tag, mine), ref) in enumerate(zip(trace, g["scores"])):
        assert_scores_close(mine, ref, what=f"{name}[{i}:{tag}]")
        flips = assert_argmax_tie_aware(np.argmax(np.asarray(mine).reshape(ref.shape[0], -1), axis=0), ref.reshape(ref.shape[0], -1),
                                        what=f"{name}[{i}:{tag}]")
        assert flips == 0, f"{name}[{i}:{tag}]: {flips} differing selections on a fixture without near-ties"


def run_oracle(g, swap=False, cls=None):
    """The oracle (or the torch port class `cls`) on the fixture's tensors; swap: the two widths exchanged."""
    p = dict(g["params"])
    kind = p.pop("kind")
    if swap:
        a, b = ("w_bit", "a_bit") if "w_bit" in p else ("A_bit", "B_bit")
        p[a], p[b] = p[b], p[a]
    if kind == "linear":
        p.pop("oc")
        o = (cls or LinearOracle)(g["weight"], g.get("bias"), **p)
        res = o.calibration_step2(g["x"], g["out"], g["grad"])
        iv = [res["w_interval"], res["a_interval"]]
    elif kind == "matmul":
        o = (cls or MatMulOracle)(**p)
        res = o.calibration_step2(g["A"], g["B"], g["out"], g["grad"])
        iv = [np.asarray(res["A_interval"]), res["B_interval"]] + ([np.asarray(res["split"])] if p["sos"] else [])
    else:
        o = (cls or ConvOracle)(g["weight"], g["bias"], **p)
        res = o.calibration_step2(g["x"], g["out"], g["grad"])
        iv = [np.asarray(res["w_interval"]), np.asarray(res["a_interval"])]
    return o, [np.asarray(v, dtype=np.float64).reshape(-1) for v in iv]


def fixture_intervals(g):
    keys = ("A_interval", "B_interval", "split") if "A" in g else ("w_interval", "a_interval")
    return [np.asarray(g[k], dtype=np.float64).reshape(-1) for k in keys if k in g]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_at_mixed_widths(name):
    g = load_golden(name)
    o, iv = run_oracle(g)
    _check_trace(o.trace, g, name)
    for mine, ref in zip(iv, fixture_intervals(g)):
        np.testing.assert_array_equal(mine, ref)
    qf = o.quant_forward(g["A"], g["B"]) if "A" in g else o.quant_forward(g["x"])
    np.testing.assert_allclose(qf, g["quant_forward"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("name", LINEAR + MATMUL)
def test_torch_port_matches_reference_at_mixed_widths(name):
    """oracle/torch_port.py has a Linear and a head-wise MatMul class (its Conv class is a_bit = 32 only, it has no sub-blocks)."""
    from oracle.torch_port import TorchLinear, TorchMatMul
    g = load_golden(name)
    o, iv = run_oracle(g, cls=TorchLinear if name in LINEAR else TorchMatMul)
    _check_trace(o.trace, g, name)
    for mine, ref in zip(iv, fixture_intervals(g)):
        np.testing.assert_array_equal(mine, ref)


@pytest.mark.parametrize("name", NAMES)
def test_exchanged_widths_are_visible_in_tables_and_intervals(name):
    g = load_golden(name)
    o, iv = run_oracle(g, swap=True)
    assert len(o.trace) == len(g["scores"])
    worst = 0.0
    for (tag, mine), ref in zip(o.trace, g["scores"]):
        ref = np.asarray(ref, dtype=np.float64)
        mine = np.asarray(mine, dtype=np.float64).reshape(ref.shape)
        worst = max(worst, float((np.abs(mine - ref) / np.maximum(np.abs(ref), np.abs(ref).max() * 1e-6)).max()))
    assert worst > 10 * SCORE_RTOL, f"{name}: exchanged widths move the tables by {worst:.2e} only"
    assert any(not np.array_equal(a, b) for a, b in zip(iv, fixture_intervals(g))), f"{name}: exchanged widths select the same intervals"
