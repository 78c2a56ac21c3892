"""Cosine Linear search with weight column blocks / activation blocks (n_H, n_a > 1) on the CPU: the numpy oracle against the
reference's own fixtures (tests/golden/linblk_*.npz, tools/gen_golden_linblk.py), and the discriminating power of those fixtures.

Intervals bit for bit; score tables within 8 ulp of the reference table's largest entry (measured: 2 .. 6 ulp); the smallest
cosine defect of every fixture at least 10 000 ulp, so that the 32 ulp bar of the GPU tests (tests/linblk_cases.py) still tells
a wrong block scale from a right one after a fixture is regenerated."""
import os

import numpy as np
import pytest

from oracle.ptq4vit_oracle import LinearOracle
from tests.helpers import GOLDEN, load_golden
from tests.linblk_cases import (BATCHING, BEYOND, MIN_DEFECT_ULP, NAMES, NONBATCHING, as_columns, assert_cos_table, beyond_tensors,
                                layer_params, smallest_defect_ulp)

ORACLE_BAR_ULP = 8


def test_the_five_fixtures_are_present_and_small():
    assert len(BATCHING) == 4 and NONBATCHING == ["linblk_ptqsl_cos_v2h2a2"], NAMES
    for n in NAMES:
        assert os.path.getsize(os.path.join(GOLDEN, n + ".npz")) <= 400 * 1024, n
        g = load_golden(n)
        p, oc, _ = layer_params(g)
        assert p["metric"] == "cosine" and (p["n_H"] > 1 or p["n_a"] > 1), n
        assert len(g["scores"]) == p["search_round"] * (p["n_H"] + p["n_a"]), n
        assert g["w_interval"].shape == (p["n_V"], 1, p["n_H"], 1) and g["a_interval"].shape == (p["n_a"], 1), n


@pytest.mark.parametrize("name", NAMES)
def test_linear_blocks_cosine_oracle_matches_reference(name):
    g = load_golden(name)
    p, oc, batching = layer_params(g)
    o = LinearOracle(g["weight"], g.get("bias"), batching=batching, **p)
    res = o.calibration_step2(g["x"], g["out"], None)
    assert len(o.trace) == len(g["scores"])
    worst = 0.0
    for i, ((tag, mine), ref) in enumerate(zip(o.trace, g["scores"])):
        worst = max(worst, assert_cos_table(mine, ref, what=f"{name}[{i}:{tag}]", bar=ORACLE_BAR_ULP))
        np.testing.assert_array_equal(np.argmax(as_columns(mine), axis=0), np.argmax(as_columns(ref), axis=0))
    print(f"[oracle] {name}: worst table error {worst:.1f} ulp")
    np.testing.assert_array_equal(res["w_interval"], g["w_interval"])
    np.testing.assert_array_equal(res["a_interval"], g["a_interval"])


@pytest.mark.parametrize("name", NAMES)
def test_fixture_defects_are_far_above_the_bar(name):
    g = load_golden(name)
    _, _, batching = layer_params(g)
    S = g["x"].shape[0] if batching else 1
    d = smallest_defect_ulp(g["scores"], S)
    print(f"[defect] {name}: smallest cosine defect {d:.0f} ulp")
    assert d >= MIN_DEFECT_ULP, f"{name}: smallest defect {d:.0f} ulp: the table bar would not tell a wrong scale from a right one"


def test_shape_beyond_the_fixtures_discriminates_too():
    """The oracle's own tables on the seeded layer the GPU test sweeps beyond the fixtures (K cuts on k-tile boundaries)."""
    w, bias, x, out = beyond_tensors()
    o = LinearOracle(w, bias, **BEYOND["hp"])
    o.calibration_step2(x, out, None)
    d = smallest_defect_ulp([t for _, t in o.trace], x.shape[0])
    print(f"[defect] beyond: smallest cosine defect {d:.0f} ulp")
    assert d >= MIN_DEFECT_ULP
