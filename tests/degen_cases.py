"""Shared by tests/test_oracle_degenerate.py and tests/test_hip_degenerate.py: blocks whose initial min-max interval is 0 or
negative on Linear and MatMul, fixtures tests/golden/degen_*.npz (oracle/gen_golden.py::gen_degenerate).

SURVEY.md App. A-10: a block with interval 0 fake-quantises as 0 / 0, so its score column is NaN in every table, argmax takes
candidate 0 (eq_alpha x the initial interval -- 0 again for the block itself) and every search that multiplies through the block
is NaN as well.  `params["zero_blocks"]` names the blocks: ["w", v, h] / ["a", group] for a Linear, ["A" | "B", head] or
["A" | "B", head, v, h] for a MatMul.  `expected_nan` turns that into the premise of every table of the run -- "all", "none" or
the list of NaN columns -- which the tests assert of the FIXTURE before they compare anything with it, so that a regenerated
fixture cannot silently become healthy."""
import numpy as np

from tests.helpers import assert_argmax_tie_aware, assert_scores_close, golden_names

NAMES = golden_names("degen_")
LINEAR = [n for n in NAMES if n.startswith(("degen_linear_", "degen_postgelu_"))]
MATMUL = [n for n in NAMES if n.startswith("degen_matmul_")]
MMBLK = [n for n in NAMES if n.startswith("degen_mmblk_")]
NEGATIVE = "degen_postgelu_hessian_negative"
NEG_ZERO = "degen_postgelu_hessian_nonpositive"


def as_columns(t):
    t = np.asarray(t)
    return t.reshape(t.shape[0], -1)


def expected_nan(g):
    """Per score table of the fixture, in the reference's order: "all", "none" or the sorted list of all-NaN columns."""
    p = g["params"]
    zb, R = p["zero_blocks"], p["search_round"]
    if p["kind"] == "linear":
        n_H, n_a = p.get("n_H", 1), p.get("n_a", 1)
        rows = sorted({b[1] for b in zb if b[0] == "w"})
        if not zb:
            w = a = "none"
        elif any(b[0] == "a" for b in zb) or len(rows) == p["n_V"]:
            w = a = "all"                             # a zero activation group poisons every product, a zero weight every row block
        else:
            w, a = rows, "all"                        # the activation search sums over every output feature
        return ([w] * n_H + [a] * n_a) * R
    heads = sorted({b[1] for b in zb})
    if p["sos"]:                                      # the split search runs against the UNQUANTISED B (matmul.py:600-631)
        assert all(b[0] == "B" for b in zb)
        return ["none", heads] * R
    steps = p.get("n_V_A", 1) * p.get("n_H_A", 1) + p.get("n_V_B", 1) * p.get("n_H_B", 1)
    return [heads] * (steps * R)


def nan_mask(ref, want):
    """The NaN mask the premise `want` describes for a table shaped like `ref` (as columns)."""
    m = np.zeros(as_columns(ref).shape, dtype=bool)
    if want == "all":
        m[:] = True
    elif want != "none":
        m[:, want] = True
    return m


def assert_fixture_premise(g, name):
    """The fixture is the degenerate case it is named for: NaN exactly where the zero blocks put it, no infinities, a zero
    interval on every zero block; the strictly negative case has no NaN and a negative interval."""
    p = g["params"]
    want = expected_nan(g)
    assert len(want) == len(g["scores"]), f"{name}: {len(g['scores'])} tables, premise for {len(want)}"
    for i, (ref, w) in enumerate(zip(g["scores"], want)):
        ref = as_columns(ref)
        np.testing.assert_array_equal(np.isnan(ref), nan_mask(ref, w), err_msg=f"{name}[{i}] fixture premise")
        assert not np.isinf(ref).any(), f"{name}[{i}] fixture premise"
    if p.get("negative_interval"):
        assert not p["zero_blocks"] and float(g["a_interval"].reshape(-1)[0]) < 0 and not np.isnan(g["quant_forward"]).any(), name
        assert float(g["x"].max()) < 0, name
        return
    assert p["zero_blocks"], name
    for b in p["zero_blocks"]:
        if b[0] == "w":
            iv = g["w_interval"][b[1], 0, b[2], 0]
        elif b[0] == "a":
            iv = g["a_interval"][b[1], 0]
        else:
            iv = g[b[0] + "_interval"][0, b[1], 0, b[2] if len(b) > 2 else 0, 0, b[3] if len(b) > 2 else 0, 0]
        assert iv == 0.0, f"{name}: block {b} has interval {iv!r}, not 0"
    assert np.isnan(g["quant_forward"]).any(), name
    if name == NEG_ZERO:
        assert np.signbit(g["a_interval"]).all() and float(g["x"].max()) == 0.0 and np.signbit(g["x"]).all(), name


def check_tables(pairs, premise, name):
    """pairs: (got table, got selection or None, reference table).  Finiteness equal to the reference's entry by entry
    (assert_scores_close), finite entries within SCORE_RTOL, selections tie-aware on the finite columns and exactly candidate 0
    on the all-NaN ones; a selection that is handed over is also the argmax of its own table.  `premise`: a fixture (every
    table of it, in its order), a list of premises as expected_nan gives them (one per pair: a call that returns some of the
    tables), or None -- the dead columns are then those the reference table itself has all NaN (an oracle run).  A table
    larger than the reference's (a buffer for more candidates or blocks) is cropped.  Returns the number of differing selections."""
    want = expected_nan(premise) if isinstance(premise, dict) else premise if premise is not None else [None] * len(pairs)
    assert len(pairs) == len(want), f"{name}: {len(pairs)} tables vs {len(want)}"
    flips = 0
    for i, ((got, best, ref), w) in enumerate(zip(pairs, want)):
        ref = as_columns(ref)
        got = np.asarray(got)
        got = got[: ref.shape[0], : ref.shape[1]] if got.ndim == 2 and got.size > ref.size else got.reshape(ref.shape)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=f"{name}[{i}] NaN pattern")
        assert_scores_close(got, ref, what=f"{name}[{i}]")
        own = np.argmax(got, axis=0)                  # NaN counts as the maximum: the first NaN, candidate 0 of a NaN column
        if best is None:
            best = own
        best = np.asarray(best).reshape(-1)[: ref.shape[1]]
        np.testing.assert_array_equal(best, own, err_msg=f"{name}[{i}] select")
        dead = (np.isnan(ref) if w is None else nan_mask(ref, w)).all(axis=0)
        assert not (np.isnan(ref).any(axis=0) & ~dead).any(), f"{name}[{i}]: a reference column is partly NaN"
        assert (best[dead] == 0).all(), f"{name}[{i}]: selection {best[dead]} on an all-NaN column, the reference takes candidate 0"
        if (~dead).any():
            flips += assert_argmax_tie_aware(best[~dead], ref[:, ~dead], what=f"{name}[{i}]")
    return flips


def assert_zero_intervals(got, ref, what):
    """The entries whose reference is +0.0 or -0.0, bit for bit: no near-tie can move them."""
    got, ref = np.asarray(got, dtype=np.float32).reshape(-1), np.asarray(ref, dtype=np.float32).reshape(-1)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    same_bits(got[ref == 0], ref[ref == 0], what + " (zero intervals)")


def assert_intervals(got, ref, mult, what, ref_scores=None):
    """Entries whose reference is +0.0 or -0.0: equal bit for bit (assert_on_candidate_grid divides by the reference).  The others:
    bit-identical or on the neighbouring entry of the same candidate table (assert_on_candidate_grid as it stands; `ref_scores`
    [candidates][blocks]: the reference's table of the pass that selected them).  Returns the number of differing entries."""
    from tests.helpers import assert_on_candidate_grid
    got = np.ascontiguousarray(np.asarray(got, dtype=np.float32).reshape(-1))
    ref = np.ascontiguousarray(np.asarray(ref, dtype=np.float32).reshape(-1))
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    z = ref == 0
    same_bits(got[z], ref[z], what + " (zero intervals)")
    if (~z).any():
        tab = None
        if ref_scores is not None:
            tab = as_columns(ref_scores)
            tab = tab[:, ~z] if tab.shape[1] == ref.size else None
        return assert_on_candidate_grid(got[~z], ref[~z], mult, what, ref_scores=tab)
    return 0


def same_bits(got, ref, what):
    """Bit-for-bit equality of two fp32 arrays: the sign of a zero counts, a NaN equals a NaN."""
    got = np.ascontiguousarray(np.asarray(got, dtype=np.float32).reshape(-1))
    ref = np.ascontiguousarray(np.asarray(ref, dtype=np.float32).reshape(-1))
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    bad = np.flatnonzero((got.view(np.uint32) != ref.view(np.uint32)) & ~(np.isnan(got) & np.isnan(ref)))
    assert bad.size == 0, f"{what}: entry {bad[0]}: {got[bad[0]]!r} vs {ref[bad[0]]!r} ({bad.size} of {got.size} differ)"


def linear_params(g):
    p = dict(g["params"])
    for k in ("kind", "oc", "zero_blocks", "negative_interval"):
        p.pop(k, None)
    return p


def matmul_params(g):
    p = dict(g["params"])
    for k in ("kind", "zero_blocks"):
        p.pop(k, None)
    return p
