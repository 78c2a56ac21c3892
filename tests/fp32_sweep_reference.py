"""CPU references for the fp32 candidate sweep (k_sweep<float>: fp32 operands, fp32 MFMAs over K) of a channel-wise Conv2d weight
search with an unquantised input (tests/test_hip_metric_grid.py, tests/test_fp32_sweep_reference_cpu.py).  numpy only; the
quantiser and the candidate tables are the oracle's (fake_quant, candidate_multipliers, ConvOracle.initialize_intervals of
oracle/ptq4vit_oracle.py).  Nothing of the library under test is imported here.

Why the fp32 oracle is a poor judge of this sweep: d = raw_out - simulated cancels two to three digits, a channel-wise score of
the small patch embedding averages only eight rows, and the oracle's own fp32 GEMM is 4e-5 .. 8e-5 away from the exact tables
there -- a legitimate fp32 sum in another order is as far from the oracle as the helpers' SCORE_RTOL (sized for sums of 1e3 .. 1e7
terms).  So the sweep is held to the exact tables, with a bar taken from an emulation of one legitimate fp32 order:

  (a) `f64`    the score tables in float64: the oracle's fp32 fake_quant weights and the fp32 inputs, converted exactly; float64 GEMM,
               bias, difference, metric and reductions.  Its rounding (2^-53 sqrt K relative to the products) is nine digits below
               anything compared with it.
  (b) `seq32`  the tables of an fp32 emulation: every output element adds its K products strictly one after another (product
               rounded to fp32, sum rounded to fp32), then bias, difference and the metric's term in fp32 in the order of
               elementwise_similarity; the terms are reduced in float64, so that what (b) is away from (a) is the rounding of the
               GEMM chain and of the term, not of the last reduction.
  `oracle`     ConvOracle's own fp32 tables of the same pass.

bar(metric) = max(SCORE_RTOL, 2 x rel_err(seq32, f64)).  (b) is ONE legitimate order; the kernel's differs (several products per
MFMA step, several accumulator blocks).  The expected error of a chain grows like sqrt K whatever the order, so another order of the
same length stays within a small factor of (b): 2.  rel_err is the measure of helpers.assert_scores_close: max over the table of
|got - ref| / max(|ref|, 1e-6 max |ref|)."""
import numpy as np

from oracle.ptq4vit_oracle import ConvOracle, candidate_multipliers, elementwise_similarity, fake_quant, im2col
from tests.helpers import SCORE_RTOL

F32, F64 = np.float32, np.float64
BAR_FACTOR = 2.0


def rel_err(got, ref):
    got, ref = np.asarray(got, dtype=F64), np.asarray(ref, dtype=F64)
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), np.abs(ref).max() * 1e-6 + 1e-300)).max())


def _reduce(terms, b, L):
    """[p][b * L][oc] elementwise similarities -> [p][oc]: mean over the pixels of an image, summed over the images (conv.py:549-553)"""
    p, _, oc = terms.shape
    return terms.reshape(p, b, L, oc).mean(axis=2, dtype=F64).sum(axis=1, dtype=F64)


def conv_w_tables(weight, bias, x, out, grad, *, stride, metric, eq_alpha, eq_beta, eq_n, chunk=25, **_):
    """Weight search of ConvOracle(channelwise, a_bit = 32), first round: dict(f64, seq32, oracle: [eq_n][oc] score tables,
    w_cands [eq_n + 1][oc]).  `grad` is read under the hessian metric only."""
    weight, x, out = (np.ascontiguousarray(t, dtype=F32) for t in (weight, x, out))
    grad = np.ascontiguousarray(grad, dtype=F32) if metric == "hessian" else None
    o = ConvOracle(weight, bias, stride=stride, w_bit=8, a_bit=32, metric=metric, eq_alpha=eq_alpha, eq_beta=eq_beta, eq_n=eq_n, search_round=1)
    o.calibration_step2(x, out, grad)
    oracle_tab = np.asarray(o.trace[0][1], dtype=F32)
    oc = weight.shape[0]
    o.initialize_intervals(x)                                  # (the search moved w_interval: the candidates come from the initial one)
    w_cands = (candidate_multipliers(eq_alpha, eq_beta, eq_n).reshape(-1, 1, 1, 1, 1) * o.w_interval[None]).astype(F32)
    cols, fh, fw = im2col(x, o.ksize, o.stride, o.padding, o.dilation)
    b, L, K = cols.shape
    cols = cols.reshape(b * L, K)
    rows = lambda t: None if t is None else np.ascontiguousarray(t.reshape(b, oc, L).transpose(0, 2, 1).reshape(b * L, oc))
    raw, g = rows(out), rows(grad)
    bias32 = np.zeros(oc, dtype=F32) if bias is None else np.asarray(bias, dtype=F32)
    f64, seq32 = np.empty((eq_n, oc), dtype=F64), np.empty((eq_n, oc), dtype=F64)
    for p0 in range(0, eq_n, chunk):
        p1 = min(eq_n, p0 + chunk)
        w_sim = fake_quant(weight[None], w_cands[p0:p1], -o.w_qmax, o.w_qmax - 1).reshape(p1 - p0, oc, K)
        # (a) float64 throughout
        sim = np.einsum("mk,pnk->pmn", cols.astype(F64), w_sim.astype(F64)) + bias32.astype(F64)
        f64[p0:p1] = _reduce(elementwise_similarity(raw.astype(F64)[None], sim, metric, None if g is None else g.astype(F64)[None]), b, L)
        # (b) fp32, the K products of each output one after another
        acc = np.zeros((p1 - p0, b * L, oc), dtype=F32)
        wt = np.ascontiguousarray(w_sim.transpose(2, 0, 1))     # [K][p][oc]
        for k in range(K):
            acc += cols[None, :, k, None] * wt[k][:, None, :]   # (fp32 product, then fp32 sum: numpy does not contract them)
        sim32 = acc + bias32
        terms = elementwise_similarity(raw[None], sim32, metric, None if g is None else g[None])
        assert terms.dtype == F32
        seq32[p0:p1] = _reduce(terms, b, L)
    return dict(f64=f64, seq32=seq32, oracle=oracle_tab, w_cands=w_cands.reshape(eq_n + 1, oc))


def bar(tables):
    """(the bar of a k_sweep<float> table against tables["f64"], rel_err(seq32, f64))"""
    e = rel_err(tables["seq32"], tables["f64"])
    return max(SCORE_RTOL, BAR_FACTOR * e), e
