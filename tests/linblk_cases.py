"""Shared by tests/test_oracle_linblk.py and tests/test_hip_linblk_cos.py: the cosine Linear search with weight column blocks /
activation blocks (n_H, n_a > 1), fixtures tests/golden/linblk_*.npz (tools/gen_golden_linblk.py).

The bar for a cosine score table: |got - ref| <= COS_BAR_ULP ulp of the reference table's LARGEST entry, one ulp being the fp32
spacing at that entry.  A cosine score is S - defect (S = images for the batching classes, 1 for the non-batching ones): the
fixtures use low bit widths so that the smallest defect is thousands of ulp -- 32 ulp is 5 x what an independent fp32
restatement on the CPU shows (6 ulp: sqrt, division, summation order) and more than 700 x below the smallest defect, so one
wrong block scale, segment boundary or slab index fails it."""
import numpy as np

from tests.helpers import golden_names, record_margin

NAMES = golden_names("linblk_")
BATCHING = [n for n in NAMES if not n.startswith("linblk_ptqsl_")]
NONBATCHING = [n for n in NAMES if n.startswith("linblk_ptqsl_")]
COS_BAR_ULP = 32
MIN_DEFECT_ULP = 10_000


def table_ulp(ref):
    """fp32 spacing at the largest entry of the reference table."""
    return float(np.spacing(np.float32(np.abs(np.asarray(ref, dtype=np.float32)).max())))


def as_columns(t):
    t = np.asarray(t)
    return t.reshape(t.shape[0], -1)


def assert_cos_table(got, ref, what="", bar=COS_BAR_ULP):
    """Every entry of `got` within `bar` ulp (of the reference table's largest entry) of `ref`; returns the worst, in ulp."""
    ref = as_columns(ref).astype(np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    assert np.isfinite(got).all() and np.isfinite(ref).all(), f"{what}: non-finite score"
    worst = float(np.abs(got - ref).max() / table_ulp(ref))
    record_margin("cos_table_ulp", worst)
    assert worst <= bar, f"{what}: cosine table off by {worst:.1f} ulp of its largest entry (bar {bar})"
    return worst


def assert_cos_selection(got_idx, ref, what="", bar=COS_BAR_ULP):
    """got_idx[j] is the reference's argmax of column j, or a candidate the REFERENCE's own table has within `bar` ulp of it."""
    ref = as_columns(ref).astype(np.float64)
    got_idx = np.asarray(got_idx).reshape(-1)[: ref.shape[1]]
    ref_idx = np.argmax(ref, axis=0)
    ulp = table_ulp(ref)
    for j, (gi, ri) in enumerate(zip(got_idx, ref_idx)):
        if gi != ri:
            gap = (ref[ri, j] - ref[gi, j]) / ulp
            record_margin("cos_tie_gap_ulp", gap)
            assert gap <= bar, f"{what}: block {j}: picked {gi}, reference {ri}, {gap:.0f} ulp apart in the reference's table (bar {bar})"
    differ = int((got_idx != ref_idx).sum())
    record_margin(None, None, {"selections": int(got_idx.size), "differing_selections": differ})
    return differ


def smallest_defect_ulp(tables, S):
    """min over the tables of (S - largest entry) in ulp of that entry: what a wrong scale has to move to go unnoticed."""
    return min((S - float(np.max(t))) / table_ulp(t) for t in tables)


def layer_params(g):
    """(constructor kwargs of the module / oracle, out_features, batching?) of a linblk fixture."""
    p = dict(g["params"])
    kind = p.pop("kind")
    oc = p.pop("oc")
    assert not p.pop("postgelu")
    return p, oc, kind == "linear"


# ---- the shape beyond the fixtures (tests/test_hip_linblk_cos.py, 5): against the numpy oracle -----------------------------
# features 200 = 2 V blocks of 100 (cross a 64-row slab), 266 samples (two 128-column tiles and a ragged third), K = 192 cut at
# 64 / 128 (n_H = 3: on k-tile boundaries) and 96 (n_a = 2)
BEYOND = dict(shape_x=(2, 133, 192), oc=200, seed=77,
              hp=dict(n_V=2, n_H=3, n_a=2, w_bit=4, a_bit=4, metric="cosine", eq_alpha=0.5, eq_beta=1.2, eq_n=100, search_round=1))


def beyond_tensors():
    c = BEYOND
    rng = np.random.default_rng(c["seed"])
    K = c["shape_x"][-1]
    w = (rng.standard_normal((c["oc"], K)) * 0.05 * np.linspace(0.5, 2.0, c["oc"])[:, None]).astype(np.float32)
    bias = (rng.standard_normal(c["oc"]) * 0.1).astype(np.float32)
    x = rng.standard_normal(c["shape_x"]).astype(np.float32)
    out = (x.reshape(-1, K) @ w.T + bias).reshape(*c["shape_x"][:-1], c["oc"]).astype(np.float32)
    return w, bias, x, out
