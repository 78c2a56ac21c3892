"""Shared by tests/test_hip_search_rounds.py and tools/plan_dump.py: the smallest calibration per path of the search rounds
(csrc/p4v_api.hip: search_rounds under linear_impl, matmul_impl and conv_impl, and the step loop of MatMulBlocksCall; DESIGN.md
s5.2 "pass memo", s5.6), three search rounds each, seeded inputs (the generators of tests/sweep_plan_cases.py) or a fixture of
tests/golden/.

`run(eng, mode)` makes ONE call and returns (intervals, tables):
  "default"  no score tables: the pass memo is on, pruning as the engine defaults it
  "scores"   want_scores=True: no memo, no pruning, every pass of every round runs and every table slot is written
  "nomemo"   the default call with desc.reserved bit 1: every pass runs, no tables
W8A8, 100 candidates unless the fixture says otherwise."""
import torch

from tests.helpers import load_golden
from tests.linblk_cases import layer_params
from tests.sweep_plan_cases import LOOSE, SEARCH, conv_inputs, linear_inputs, matmul_inputs

MODES = ("default", "scores", "nomemo")
ROUNDS = dict(SEARCH, search_round=3)


def _cuda(t):
    return None if t is None else t.cuda()


def _call(eng, job, mode):
    if mode == "nomemo":
        getattr(job.desc, "mm", job.desc).reserved |= 2      # (a sub-block descriptor wraps the MatMul's)
    eng.run_job(job)
    return [t for t in job.outputs if t is not None], [t for t in (job.scores, job.best) if t is not None]


def _linear(K, N, *, seed, metric="hessian", images=2, tokens=64, n_V=1, n_H=1, n_a=1, postgelu=False, variant=0):
    def run(eng, mode):
        w, b, x, out, grad = linear_inputs(K, N, seed=seed, images=images, tokens=tokens, postgelu=postgelu)
        eng.debug_variant(variant)
        try:
            job = eng.linear_job(weight=_cuda(w), bias=_cuda(b), x=_cuda(x), out=_cuda(out), grad=_cuda(grad) if metric == "hessian" else None,
                                 w_bit=8, a_bit=8, metric=metric, n_V=n_V, n_H=n_H, n_a=n_a, postgelu=postgelu,
                                 want_scores=mode == "scores", **ROUNDS)
            return _call(eng, job, mode)
        finally:
            eng.debug_variant(0)
    return run


def _linear_fixture(name):
    def run(eng, mode):
        g = load_golden(name)
        p, _, _ = layer_params(g)
        t = lambda k: _cuda(torch.from_numpy(g[k])) if k in g else None
        job = eng.linear_job(weight=t("weight"), bias=t("bias"), x=t("x"), out=t("out"), grad=None, want_scores=mode == "scores",
                             **dict(p, search_round=3))
        return _call(eng, job, mode)
    return run


def _matmul(M, K, N, *, seed, metric="hessian", sos=False):
    def run(eng, mode):
        A, B, out, grad = matmul_inputs(M, K, N, seed=seed, sos=sos)
        job = eng.matmul_job(A=_cuda(A), B=_cuda(B), out=_cuda(out), grad=_cuda(grad) if metric == "hessian" else None, A_bit=8, B_bit=8,
                             metric=metric, sos=sos, want_scores=mode == "scores", **ROUNDS)
        return _call(eng, job, mode)
    return run


def _matmul_blocks_fixture(name):
    def run(eng, mode):
        g = load_golden(name)
        p = dict(g["params"])
        sos = p["sos"]
        blocks = ((1, 1) if sos else (p.get("n_V_A", 1), p.get("n_H_A", 1))) + (p.get("n_V_B", 1), p.get("n_H_B", 1))
        t = lambda k: _cuda(torch.from_numpy(g[k]))
        job = eng.matmul_job(A=t("A"), B=t("B"), out=t("out"), grad=t("grad") if p["metric"] == "hessian" else None, A_bit=p["A_bit"],
                             B_bit=p["B_bit"], metric=p["metric"], eq_alpha=p["eq_alpha"], eq_beta=p["eq_beta"], eq_n=p["eq_n"],
                             search_round=3, sos=sos, want_scores=mode == "scores", blocks=blocks)
        return _call(eng, job, mode)
    return run


def _conv_fixture(name):
    def run(eng, mode):
        g = load_golden(name)
        p = dict(g["params"])
        p.pop("kind")
        geo = {k: tuple(p.pop(k)) for k in ("stride", "padding", "dilation")}
        t = lambda k: _cuda(torch.from_numpy(g[k]))
        job = eng.conv_job(weight=t("weight"), bias=t("bias"), x=t("x"), out=t("out"), grad=t("grad") if p["metric"] == "hessian" else None,
                           want_scores=mode == "scores", **geo, **dict(p, search_round=3))
        return _call(eng, job, mode)
    return run


def _conv(*, seed, metric="hessian", a_bit=32, channelwise=True):
    def run(eng, mode):
        w, b, x, out, grad = conv_inputs(seed=seed)
        job = eng.conv_job(weight=_cuda(w), bias=_cuda(b), x=_cuda(x), out=_cuda(out), grad=_cuda(grad) if metric == "hessian" else None,
                           stride=(16, 16), padding=(0, 0), dilation=(1, 1), w_bit=8, a_bit=a_bit, metric=metric, channelwise=channelwise,
                           want_scores=mode == "scores", **ROUNDS)
        return _call(eng, job, mode)
    return run


# (name, run)
CASES = [
    # Linear, hessian: the dense int8 path; the post-GELU twin (the fold, rebuilt per activation pass) on k_sweep6 and k_sweep7;
    # column / activation blocks (fp32 general path, candidate mixing, no memo on either side); the pruned passes of the 650-row layer
    ("linear_hessian_k192_n128", _linear(192, 128, seed=1)),
    ("postgelu_hessian_k192_n128", _linear(192, 128, seed=31, postgelu=True)),
    ("postgelu_hessian_k1024_n64", _linear(1024, 64, seed=4, postgelu=True)),
    ("linear_hessian_k192_n128_nH2_na2", _linear(192, 128, seed=3, n_H=2, n_a=2)),
    ("bound_650x96_k192", _linear(192, 96, seed=11, images=10, tokens=65, variant=LOOSE)),
    # Linear, cosine: k_sweep6 (cos6), k_sweep7 (cos7), swapped with one GEMM per V block, the segmented sweep
    ("linear_cosine_k192_n128", _linear(192, 128, seed=5, metric="cosine")),
    ("linear_cosine_k1024_n64", _linear(1024, 64, seed=6, metric="cosine")),
    ("linear_cosine_k192_n120_nV3", _linear(192, 120, seed=7, metric="cosine", n_V=3)),
    ("linblk_cos_v2h2a3_w4a4", _linear_fixture("linblk_cos_v2h2a3_w4a4")),
    # MatMul, 2 x 2 heads: head-wise A and B; the split search (k_sos_split: constant key, two-vector value); with cosine the fp32
    # split pass and the fp32 B search
    ("matmul_qk_49_hessian", _matmul(49, 64, 49, seed=8)),
    ("matmul_qk_49_cosine", _matmul(49, 64, 49, seed=9, metric="cosine")),
    ("matmul_sos_49_hessian", _matmul(49, 49, 64, seed=10, sos=True)),
    ("matmul_sos_49_cosine", _matmul(49, 49, 64, seed=12, metric="cosine", sos=True)),
    # Conv, the 2 x 3 x 32 x 32 patch embedding: unquantised input (constant key), both searches, layer-wise cosine
    ("conv_cw_hessian_a32", _conv(seed=13)),
    ("conv_cw_hessian_a8", _conv(seed=14, a_bit=8)),
    ("conv_lw_cosine", _conv(seed=15, metric="cosine", channelwise=False)),
    # MatMul with sub-blocks (fixtures of tests/test_hip_mmblk.py; no memo on this path): 4 x 3 heads, 13 x 8 x 13, ten block steps a
    # round -- the step enumeration and the [round][step] slots; split-of-softmax 13 x 13 x 8 -- the head-wise split step among the
    # block steps; 5 x 8 x 5 with n_V_A = 4 -- a block of nothing but padding, the abs-max start value
    ("mmblk_qk_hessian_vA2hA2_vB2hB3", _matmul_blocks_fixture("mmblk_qk_hessian_vA2hA2_vB2hB3")),
    ("mmblk_sos_hessian_vB2hB2", _matmul_blocks_fixture("mmblk_sos_hessian_vB2hB2")),
    ("mmblk_empty_block", _matmul_blocks_fixture("mmblk_empty_block")),
    # Conv, 3 x 5 x 17 x 23 with a dilated 3 x 5 kernel (a fixture of tests/test_hip_conv_geometry.py), a_bit 8: both sides on a
    # geometry that is not a patch grid
    ("convgeo_a_cw_hessian_a8_rect_dil", _conv_fixture("convgeo_a_cw_hessian_a8_rect_dil")),
]


def run_case(eng, run, mode):
    """One call with launch records: intervals, tables, [(kernel, stage, grid_x, grid_z)], (memo hits, memo misses), launch
    counters, prune counters."""
    eng.launch_counters(reset=True)
    eng.prune_counters(reset=True)
    eng.stats_reset()
    eng.stats_enable(True)
    try:
        intervals, tables = run(eng, mode)
        torch.cuda.synchronize()
        st = eng.stats_get()
        recs = [(r["kernel"], r["stage"], r["grid_x"], r["grid_z"]) for r in eng.stats_launches()]
    finally:
        eng.stats_enable(False)
    return dict(intervals=intervals, tables=tables, records=recs, memo=(int(st["memo_hits"]), int(st["memo_misses"])),
                launch_counters=eng.launch_counters(), prune_counters=eng.prune_counters())
