"""Shared by tests/test_hip_streams.py: the entry points of ptq4vit_amd/engine.py as stream-contract cases, and `Probe`, the
engine stand-in the cases are run through.

An ENTRY is (id, api, call, never_syncs): `call(eng)` makes the entry point's ABI call(s) through `eng` -- the engine module or a
Probe around it -- and returns its result tensors; `api` names the public functions of engine.py the call goes through;
`never_syncs`: include/ptq4vit_hip.h promises that the call returns without waiting for its stream.

The calibration cases are the seeded makers the suite already has (tests/sweep_plan_cases.py, tests/pruned_pass_cases.py,
tests/search_round_cases.py) and a few more on the edges of the mapped-host mirror (csrc/p4v_api.hip: MIR_BLK = 32 score blocks
with mirrored candidate ranges, MIR_SLOT = 2048 mirrored intervals), each in two modes: "scores" (want_scores=True: no memo, no
read-back, asynchronous) and "memo" (the default call: pass memo and survivor read-backs).

Probe modes:
  plain    Probe(engine): every ABI-making call is made as it is, on torch's current stream, and its host time is added up.
  ordered  Probe(engine, stream=s, delay=Delay, delay_ms=D), used inside `with torch.cuda.stream(s)`: every floating-point device
           tensor handed to the engine is replaced by a NaN-filled buffer of the same shape and strides; then, per ABI-making
           call: device synchronisation, D ms of GEMMs on s, the real inputs copied into the buffers on s, the call, its outputs
           copied on s -- and no host synchronisation in between.  A launch the engine put on another stream reads NaN (or its
           output is copied before it ran).  Integer tensors (multi_copy's pointer table) stay as they are: a NaN pattern
           read as an address would fault instead of failing.
  frozen   freeze_debug=True: the cases' own debug_variant / debug_tuning calls do nothing (the process-wide A/B words are set
           once by a test that runs cases in several threads)."""
import functools
import math
import time

import numpy as np
import torch

from tests import pruned_pass_cases as pp
from tests import search_round_cases as sr
from tests import sweep_plan_cases as sp
from tests.degen_cases import linear_params
from tests.helpers import load_golden
from tests.sweep_plan_cases import LOOSE, conv_inputs, linear_inputs, matmul_inputs

ROUNDS = sr.ROUNDS
NAN = float("nan")


# ---- delay ------------------------------------------------------------------------------------------------------------------
class Delay:
    """GPU work of a known duration: a chain of fp32 torch.mm on one fixed 4096 x 4096 pair, the time of one product measured
    once (event pair, after a warm-up) on the machine the tests run on."""

    def __init__(self, dev):
        g = torch.Generator().manual_seed(3200)
        self.a = torch.randn(4096, 4096, generator=g).to(dev)
        self.b = torch.randn(4096, 4096, generator=g).to(dev)
        self.c = torch.empty(4096, 4096, device=dev)
        for _ in range(16):
            torch.mm(self.a, self.b, out=self.c)
        torch.cuda.synchronize(dev)
        n = 8
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            torch.mm(self.a, self.b, out=self.c)
        e1.record()
        e1.synchronize()
        self.ms_per_gemm = e0.elapsed_time(e1) / n
        assert self.ms_per_gemm > 0.0

    def __call__(self, stream, ms):
        """at least `ms` milliseconds of work on `stream` (the products of concurrent delays share the output: nobody reads it)"""
        with torch.cuda.stream(stream):
            for _ in range(max(1, math.ceil(ms / self.ms_per_gemm))):
                torch.mm(self.a, self.b, out=self.c)


# ---- staging ----------------------------------------------------------------------------------------------------------------
def _nan_like(t):
    with torch.cuda.stream(torch.cuda.default_stream(t.device)):      # (the caller's stream keeps the blocks its outputs will take)
        buf = torch.empty_strided(t.size(), t.stride(), dtype=t.dtype, device=t.device)
        buf.fill_(NAN)
    return buf


def _stage(obj, pairs, memo):
    """`obj` with every floating-point device tensor replaced by a NaN buffer; (buffer, tensor) appended to `pairs`"""
    if torch.is_tensor(obj):
        if not (obj.is_cuda and obj.is_floating_point()):
            return obj
        if id(obj) not in memo:
            memo[id(obj)] = _nan_like(obj.detach())
            pairs.append((memo[id(obj)], obj.detach()))
        return memo[id(obj)]
    if isinstance(obj, dict):
        return {k: _stage(v, pairs, memo) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_stage(v, pairs, memo) for v in obj)
    return obj


def _clone(obj):
    if torch.is_tensor(obj):
        return obj.clone()
    if isinstance(obj, (list, tuple)):
        return type(obj)(_clone(v) for v in obj)
    return obj


def flat(obj):
    """the tensors of a result, in order"""
    if torch.is_tensor(obj):
        return [obj]
    if isinstance(obj, (list, tuple)):
        return [t for v in obj for t in flat(v)]
    assert obj is None, type(obj)
    return []


def to_host(obj):
    """a result as (dtype, shape, bytes) per tensor: what `bit for bit` compares"""
    return [(str(t.dtype), tuple(t.shape), t.detach().cpu().contiguous().numpy().tobytes()) for t in flat(obj)]


SINGLE = ("linear_quant_forward", "matmul_quant_forward", "matmul_blocks_quant_forward", "mlp_quant_forward", "attn_quant_forward",
          "window_attn_quant_forward", "qkv_attn_quant_forward", "quantize_i8", "pack_plane_i8", "fake_quant", "export_quantize",
          "score_argmax_gather", "multi_copy")
JOBS = ("linear_job", "matmul_job", "conv_job")
STEPPERS = ("LinearStepper", "MatMulStepper", "ConvStepper")


class Probe:
    def __init__(self, eng, *, stream=None, delay=None, delay_ms=None, freeze_debug=False):
        self.eng, self.stream, self.delay, self.delay_ms, self.freeze_debug = eng, stream, delay, delay_ms, freeze_debug
        self.ordered = delay_ms is not None
        self.host_ms, self.calls, self.busy = 0.0, 0, []
        self._pending, self._memo = [], {}

    # -- the two ways a call is made
    def _timed(self, fn):
        t0 = time.perf_counter()
        res = fn()
        self.host_ms += (time.perf_counter() - t0) * 1e3
        self.calls += 1
        return res

    def _ordered(self, pairs, fn):
        s = self.stream
        assert torch.cuda.current_stream() == s, "an ordered Probe is used inside `with torch.cuda.stream(its stream)`"
        torch.cuda.synchronize()
        self.delay(s, self.delay_ms)
        for buf, real in pairs:
            buf.copy_(real)
        res = self._timed(fn)
        self.busy.append(not s.query())
        return _clone(res)

    def _take_pending(self):
        pairs, self._pending, self._memo = self._pending, [], {}
        return pairs

    def staged(self, t):
        """a tensor the next call reads through a pointer the Probe cannot see (multi_copy's sources)"""
        return _stage(t, self._pending, self._memo) if self.ordered else t

    # -- the engine's surface
    def __getattr__(self, name):
        real = getattr(self.eng, name)
        if name in SINGLE:
            return functools.partial(self._single, real)
        if name in JOBS:
            return functools.partial(self._job, real)
        if name in STEPPERS:
            return functools.partial(_StepperProbe, self, real)
        if self.freeze_debug and name in ("debug_variant", "debug_tuning"):
            return lambda *a, **kw: None
        return real

    def _single(self, real, *a, **kw):
        if not self.ordered:
            return self._timed(lambda: real(*a, **kw))
        a, kw = _stage((a, kw), self._pending, self._memo)
        return self._ordered(self._take_pending(), lambda: real(*a, **kw))

    def _job(self, real, **kw):
        if self.ordered:
            kw = _stage(kw, self._pending, self._memo)
        return real(**kw)

    def _launch(self, fn, jobs):
        if not self.ordered:
            return self._timed(fn)
        self._ordered(self._take_pending(), fn)
        for job in jobs:            # the outputs as they are on the stream right behind the call
            job.outputs, job.scores, job.best = _clone(tuple(job.outputs)), _clone(job.scores), _clone(job.best)

    def run_job(self, job):
        self._launch(lambda: self.eng.run_job(job), [job])
        return job

    def calibrate_group(self, jobs, inputs_ready=None):
        jobs = list(jobs)
        self._launch(lambda: self.eng.calibrate_group(jobs, inputs_ready=inputs_ready), jobs)
        return jobs

    def linear_calibrate(self, **kw):
        job = self.run_job(self.linear_job(**kw))
        return job.outputs[0], job.outputs[1], job.scores, job.best

    def matmul_calibrate(self, **kw):
        job = self.run_job(self.matmul_job(**kw))
        return job.outputs[0], job.outputs[1], job.outputs[2], job.scores, job.best

    def conv_calibrate(self, **kw):
        job = self.run_job(self.conv_job(**kw))
        return job.outputs[0], job.outputs[1], job.scores, job.best


class _StepperProbe:
    """engine.*Stepper behind a Probe: ordered, the module's tensors are NaN buffers refilled before every call"""

    def __init__(self, probe, cls, **kw):
        self._p, self._pairs = probe, []
        if probe.ordered:
            kw = _stage(kw, self._pairs, {})
        self._st = cls(**kw)

    def __getattr__(self, name):
        if name in ("_p", "_pairs", "_st"):
            raise AttributeError(name)
        f = getattr(self._st, name)
        if name.startswith("_") or not callable(f):
            return f

        def call(*a, **kw):
            if not self._p.ordered:
                return self._p._timed(lambda: f(*a, **kw))
            pairs = list(self._pairs)
            a, kw = _stage((a, kw), pairs, {})
            for buf, _ in self._pairs:
                buf.fill_(NAN)
            return self._p._ordered(pairs, lambda: f(*a, **kw))
        return call


# ---- calibration cases ------------------------------------------------------------------------------------------------------
def _cuda(t):
    return None if t is None else t.cuda()


def _from_plan(run):            # sweep_plan_cases: run(eng, prune) with want_scores = not prune
    return lambda eng, scores: run(eng, not scores)


def _from_pruned(run):          # pruned_pass_cases: run(eng, mode, prune, want_scores)
    return lambda eng, scores: run(eng, "default", want_scores=scores)


def _from_rounds(run):          # search_round_cases: run(eng, mode)
    return lambda eng, scores: run(eng, "scores" if scores else "default")


def _matmul_heads(heads, *, sos, seed):
    """q.k^T / split-of-softmax attn.v of `heads` heads, batch 2, S = 65, D = 64, pruned by force: one score block per head"""
    def run(eng, scores):
        M, K, N = (65, 65, 64) if sos else (65, 64, 65)
        A, B, out, grad = matmul_inputs(M, K, N, seed=seed, sos=sos, batch=2, heads=heads)
        eng.debug_variant(LOOSE)
        try:
            job = eng.matmul_job(A=_cuda(A), B=_cuda(B), out=_cuda(out), grad=_cuda(grad), A_bit=8, B_bit=8, metric="hessian", sos=sos,
                                 want_scores=scores, **ROUNDS)
            return sr._call(eng, job, "default")
        finally:
            eng.debug_variant(0)
    return run


def conv_wide_inputs(filters, *, seed):
    """(weight, bias, x, out, grad) of `filters` 3 x 2 x 2 filters on 2 x 3 x 16 x 16 images, stride 2, on the host"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 3, 16, 16, generator=g)
    w = torch.randn(filters, 3, 2, 2, generator=g) * 0.3 * torch.linspace(0.5, 2.0, filters).view(-1, 1, 1, 1)
    b = torch.randn(filters, generator=g) * 0.05
    out = torch.nn.functional.conv2d(x, w, b, stride=2)
    return w, b, x, out, torch.randn(out.shape, generator=g) * 1e-10


def _conv_wide(filters, *, seed):
    def run(eng, scores):
        w, b, x, out, grad = conv_wide_inputs(filters, seed=seed)
        job = eng.conv_job(weight=_cuda(w), bias=_cuda(b), x=_cuda(x), out=_cuda(out), grad=_cuda(grad), stride=(2, 2), padding=(0, 0),
                           dilation=(1, 1), w_bit=8, a_bit=8, metric="hessian", channelwise=True, want_scores=scores, **ROUNDS)
        return sr._call(eng, job, "default")
    return run


DEGEN = "degen_linear_v3_hessian_zero_rows"


def _degen_linear(name):
    def run(eng, scores):
        g = load_golden(name)
        p = linear_params(g)
        t = lambda k: _cuda(torch.from_numpy(np.ascontiguousarray(g[k]))) if k in g else None
        job = eng.linear_job(weight=t("weight"), bias=t("bias"), x=t("x"), out=t("out"), grad=t("grad"), n_H=p.pop("n_H", 1),
                             n_a=p.pop("n_a", 1), want_scores=scores, **p)
        return sr._call(eng, job, "default")
    return run


TWIN = "postgelu_hessian_k192_n128"
# what a case's pruned passes do in "memo" mode, asserted on prune_counters(): "staged", "kept" (eligible, full sweep), "never"
PRUNE_EXPECT = {name: "staged" for name, _ in pp.CASES}
PRUNE_EXPECT.update(lin650_flat="kept", lin650_scores="never", bound_650x96_k192="staged", lin650_nV32="staged", lin650_nV33="staged",
                    qk65_h32="staged", qk65_h33="staged", sos65_h32="staged", sos65_h33="staged")


def _calibration_cases():
    """[(name, api, fn(eng, scores), modes)]"""
    lin, mm, cv = ("linear_job", "run_job"), ("matmul_job", "run_job"), ("conv_job", "run_job")
    api_of = lambda name: cv if name.startswith("conv") else mm if name.startswith(("matmul", "mmblk", "qk", "sos")) else lin
    direct = {lin: ("linear_calibrate",), mm: ("matmul_calibrate",), cv: ("conv_calibrate",)}
    both = ("scores", "memo")
    cases = []
    for name, run, _pruned in sp.CASES:       # (the sub-block fixture always returns its tables: one mode)
        cases.append((name, direct[api_of(name)], _from_plan(run), ("scores",) if name.startswith("mmblk") else both))
    for name, run in pp.CASES:
        cases.append((name, api_of(name), _from_pruned(run), both))
    L650 = pp.L650
    cases += [
        # per-block candidate ranges of the weight search on either side of MIR_BLK
        ("lin650_nV32", lin, _from_pruned(pp._linear(64, 32 * 64, seed=51, n_V=32, variant=LOOSE, **L650)), both),
        ("lin650_nV33", lin, _from_pruned(pp._linear(64, 33 * 64, seed=52, n_V=33, variant=LOOSE, **L650)), both),
        # head-wise ranges on either side of MIR_BLK
        ("qk65_h32", mm, _matmul_heads(32, sos=False, seed=53), both),
        ("qk65_h33", mm, _matmul_heads(33, sos=False, seed=54), both),
        ("sos65_h32", mm, _matmul_heads(32, sos=True, seed=55), both),
        ("sos65_h33", mm, _matmul_heads(33, sos=True, seed=56), both),
        # the interval vector on either side of MIR_SLOT
        ("conv_cw_2048", cv, _conv_wide(2048, seed=57), both),
        ("conv_cw_2080", cv, _conv_wide(2080, seed=58), both),
        # K-segment kernels, NaN score columns, pass-memo hits
        ("mmblk_sos_hessian_vB2hB2", mm, _from_rounds(sr._matmul_blocks_fixture("mmblk_sos_hessian_vB2hB2")), both),
        ("linblk_cos_v2h2a3_w4a4", lin, _from_rounds(sr._linear_fixture("linblk_cos_v2h2a3_w4a4")), both),
        (DEGEN, lin, _degen_linear(DEGEN), both),
        (TWIN, lin, _from_rounds(dict(sr.CASES)[TWIN]), both),
    ]
    return cases


CALIBRATIONS = _calibration_cases()


# ---- granular steppers ------------------------------------------------------------------------------------------------------
def _cands(eng, iv):
    return eng.candidate_multipliers(ROUNDS["eq_alpha"], ROUNDS["eq_beta"], ROUNDS["eq_n"], iv.device).view(-1, 1) * iv.reshape(1, -1)


def drive(gen):
    """run a stepper sequence to its end; the sequences yield between ABI calls, so a caller may switch streams there"""
    try:
        while True:
            next(gen)
    except StopIteration as e:
        return e.value


def linear_steps_gen(eng):
    w, b, x, out, grad = linear_inputs(192, 96, seed=41, **pp.L650)
    st = eng.LinearStepper(weight=_cuda(w), bias=_cuda(b), x=_cuda(x), out=_cuda(out), grad=_cuda(grad), w_bit=8, a_bit=8, metric="hessian",
                           eq_n=ROUNDS["eq_n"], n_V=3, n_H=1, n_a=1)
    yield
    w0, a0 = st.init_intervals()         # (a min-max initialisation: the mirror of what it wrote is not valid)
    yield
    w1, _, _ = st.search_w(_cands(eng, w0), w0, a0)
    yield
    a1, _, _ = st.search_a(_cands(eng, a0), w1, a0)
    return [w0, a0, w1, a1]


def sos_steps_gen(eng):
    A, B, out, grad = matmul_inputs(65, 65, 64, seed=48, sos=True)
    st = eng.MatMulStepper(A=_cuda(A), B=_cuda(B), out=_cuda(out), grad=_cuda(grad), A_bit=8, B_bit=8, metric="hessian", eq_n=ROUNDS["eq_n"],
                           sos=True)
    yield
    A0, B0 = st.init_intervals()
    assert A0 is None
    yield
    split, A1, _, _ = st.search_split()
    yield
    B1, _, _ = st.search_B(_cands(eng, B0), A1, B0, split=split)
    return [B0, split, A1, B1]


def qk_steps_gen(eng):
    A, B, out, grad = matmul_inputs(65, 64, 65, seed=46)
    st = eng.MatMulStepper(A=_cuda(A), B=_cuda(B), out=_cuda(out), grad=_cuda(grad), A_bit=8, B_bit=8, metric="hessian", eq_n=ROUNDS["eq_n"])
    yield
    A0, B0 = st.init_intervals()
    yield
    A1, _, _ = st.search_A(_cands(eng, A0), A0, B0)
    yield
    B1, _, _ = st.search_B(_cands(eng, B0), A1, B0)
    return [A0, B0, A1, B1]


def conv_steps_gen(eng):
    w, b, x, out, grad = conv_inputs(seed=50, images=10, size=64, patch=8)
    st = eng.ConvStepper(weight=_cuda(w), bias=_cuda(b), x=_cuda(x), out=_cuda(out), grad=_cuda(grad), stride=(8, 8), padding=(0, 0),
                         dilation=(1, 1), w_bit=8, a_bit=8, metric="hessian", eq_n=ROUNDS["eq_n"], channelwise=True)
    yield
    w0, a0 = st.init_intervals()
    yield
    w1, _, _ = st.search_w(_cands(eng, w0), w0, a0)
    yield
    a1, _, _ = st.search_a(_cands(eng, a0), w1, a0)
    return [w0, a0, w1, a1]


def linear_steps(eng):
    return drive(linear_steps_gen(eng))


def sos_steps(eng):
    return drive(sos_steps_gen(eng))


def qk_steps(eng):
    return drive(qk_steps_gen(eng))


def conv_steps(eng):
    return drive(conv_steps_gen(eng))


# ---- forwards and the small entry points: inputs made once, on the null stream -----------------------------------------------------
_PREP = {}


def _prep(key, make):
    if key not in _PREP:
        with torch.no_grad():
            _PREP[key] = make()
        torch.cuda.synchronize()
    return _PREP[key]


def _minmax(t, dims, q):
    return (t.abs().amax(dim=dims) / (q - 0.5)).contiguous()


def linear_forward(eng):
    def make():
        w, b, x, _, _ = (_cuda(t) for t in linear_inputs(192, 120, seed=6))
        return dict(weight=w, bias=b, x=x, w_interval=_minmax(w.view(3, 40, 192), (1, 2), 128), a_interval=_minmax(x, (0, 1, 2), 128).reshape(1),
                    w_bit=8, a_bit=8, n_V=3, n_H=1, n_a=1)
    return eng.linear_quant_forward(**_prep("linear", make))


def matmul_forward(eng):
    def make():
        A, B, _, _ = (_cuda(t) for t in matmul_inputs(49, 64, 49, seed=7))
        return dict(A=A, B=B, A_interval=_minmax(A, (0, 2, 3), 128), B_interval=_minmax(B, (0, 2, 3), 128), split=None, A_bit=8, B_bit=8)
    return eng.matmul_quant_forward(**_prep("matmul", make))


def matmul_blocks_forward(eng):
    def make():
        g = load_golden("mmblk_qk_hessian_vA2hA2_vB2hB3")
        p = g["params"]
        t = lambda k: _cuda(torch.from_numpy(np.ascontiguousarray(g[k])))
        return dict(A=t("A"), B=t("B"), A_interval=t("A_interval").reshape(-1), B_interval=t("B_interval").reshape(-1), split=None,
                    A_bit=p["A_bit"], B_bit=p["B_bit"], blocks=(p["n_V_A"], p["n_H_A"], p["n_V_B"], p["n_H_B"]))
    return eng.matmul_blocks_quant_forward(**_prep("matmul_blocks", make))


def mlp_forward(eng):
    def make():
        from ptq4vit_amd.utils.fuse import _layer
        from tests.test_hip_fused_mlp import CASES, _modules
        fc1, fc2, x = _modules(CASES[0])
        return dict(x=x, fc1=_layer(fc1), fc2=_layer(fc2))
    return eng.mlp_quant_forward(want_hidden=True, want_planes=True, **_prep("mlp", make))


def _attn_sides(q, kT, v, sos_bits=8):
    from tests.test_hip_fused_attention import HEAD_FACTORS, SPLIT
    H = q.shape[1]
    f = lambda k: torch.tensor(HEAD_FACTORS[k][:H], device=q.device)
    qm = 2 ** (sos_bits - 1)
    qk = dict(A_interval=_minmax(q, (0, 2, 3), 128) * f("qA"), B_interval=_minmax(kT, (0, 2, 3), 128) * f("qB"), split=None, A_bit=8, B_bit=8,
              sos=False)
    pv = dict(A_interval=torch.tensor(float(np.float32(SPLIT) / np.float32(qm - 1)), device=q.device),
              B_interval=_minmax(v, (0, 2, 3), 128) * f("pB"), split=torch.tensor(SPLIT, device=q.device), A_bit=8, B_bit=8, sos=True)
    return qk, pv


def attn_forward(eng):
    def make():
        from tests.test_hip_fused_attention import CASES, _inputs
        q, kT, v = _inputs(CASES[0])
        qk, pv = _attn_sides(q, kT, v)
        return dict(q=q, kT=kT, v=v, scale=q.shape[-1] ** -0.5, qk=qk, pv=pv)
    return eng.attn_quant_forward(want_probs=True, want_planes=True, **_prep("attn", make))


def window_attn_forward(eng):
    def make():
        from tests.test_hip_fused_window_attention import CASES, _inputs
        q, kT, v, bias, mask = _inputs(CASES[0])
        assert mask is not None
        qk, pv = _attn_sides(q, kT, v)
        return dict(q=q, kT=kT, v=v, bias=bias, mask=mask, qk=qk, pv=pv)
    return eng.window_attn_quant_forward(want_probs=True, want_planes=True, **_prep("wattn", make))


def qkv_attn_forward(eng):
    def make():
        from tests.test_hip_fused_qkv import CASES, _inputs, _slices
        case = CASES[0]
        x, W, bias = _inputs(case)
        lin = dict(weight=W, bias=bias, w_interval=_minmax(W.reshape(case.n_V, -1), (1,), 128), a_interval=_minmax(x, (0, 1, 2), 128).reshape(1),
                   w_bit=8, a_bit=8, n_V=case.n_V, n_H=1, n_a=1)
        q, kT, v = _slices(torch.nn.functional.linear(x, W, bias), case.H)
        qk, pv = _attn_sides(q, kT, v)
        return dict(x=x, qkv=lin, scale=case.D ** -0.5, qk=qk, pv=pv)
    return eng.qkv_attn_quant_forward(want_qkv=True, want_probs=True, want_planes=True, **_prep("qkv", make))


def _plane_input():
    def make():
        g = torch.Generator().manual_seed(3201)
        x = (torch.randn(6 * 37, 100, generator=g) * torch.linspace(0.5, 2.0, 6).repeat_interleave(37)[:, None]).cuda()
        return x, _minmax(x.view(6, 37, 100), (1, 2), 128)
    return _prep("plane", make)


def quantize_i8(eng):
    x, scales = _plane_input()
    return eng.quantize_i8(x, scales, 37, -128, 127)


def pack_plane_i8(eng):
    x, scales = _plane_input()
    return eng.pack_plane_i8(x, mode="sym", scales=scales, rows_per_scale=37, lo=-128, hi=127)


def fake_quant(eng):
    x, scales = _plane_input()
    return eng.fake_quant(x, scales, 37, -128, 127)


def export_quantize(eng):
    def make():
        g = torch.Generator().manual_seed(3202)
        src = torch.randn(2, 3, 50, 64, generator=g).cuda()
        return src, _minmax(src, (0, 2, 3), 128)
    src, scale = _prep("export", make)          # one scale per head (dimension 1)
    return eng.export_quantize(src, mode="sym_i8", scale1=scale, scale1_stride=(0, 1, 0, 0), scale1_div=(1, 1, 1, 1), lo1=-128, hi1=127)


def score_argmax_gather(eng):
    def make():
        g = torch.Generator().manual_seed(3203)
        scores = torch.randn(100, 33, generator=g)
        scores[:, 5] = NAN                       # a NaN column selects candidate 0
        return scores.cuda(), torch.rand(101, 33, generator=g).cuda()
    scores, cands = _prep("argmax", make)
    return eng.score_argmax_gather(scores, cands)


def multi_copy(eng):
    def make():
        g = torch.Generator().manual_seed(3204)
        return [torch.randn(n, generator=g).cuda() for n in (4096, 100003, 7)]
    srcs = _prep("multi_copy", make)
    staged = [eng.staged(s) for s in srcs]
    dsts = [torch.full((3 * s.numel(),), -7.0, device="cuda") for s in srcs]
    rows = [[s.data_ptr(), d.data_ptr(), s.numel() * 4] for s, d in zip(staged, dsts)]
    table = torch.tensor(rows, dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    eng.multi_copy(table, len(rows), 1, max(r[2] for r in rows), torch.device("cuda", torch.cuda.current_device()))
    return [d.clone() for d in dsts]


def _small_group_specs():
    def make():
        specs = []
        for seed in (61, 62, 63):
            w, b, x, out, grad = (_cuda(t) for t in linear_inputs(192, 128, seed=seed))
            specs.append(("linear", dict(weight=w, bias=b, x=x, out=out, grad=grad, w_bit=8, a_bit=8, metric="hessian", n_V=1, n_H=1, n_a=1, **ROUNDS)))
        A, B, out, grad = (_cuda(t) for t in matmul_inputs(49, 64, 49, seed=64))
        specs.append(("matmul", dict(A=A, B=B, out=out, grad=grad, A_bit=8, B_bit=8, metric="hessian", **ROUNDS)))
        return specs
    return _prep("group", make)


CAPTURED = {"linear": ("x", "out", "grad"), "matmul": ("A", "B", "out", "grad")}      # what a capture pass produces: not the weights


def small_group(eng):
    """three Linear jobs and one MatMul job in one p4v_calibrate_group call"""
    jobs = eng.calibrate_group([getattr(eng, kind + "_job")(**kw) for kind, kw in _small_group_specs()])
    return [j.outputs for j in jobs]


class Entry:
    def __init__(self, id, api, call, never_syncs=False, prune=None, calibration=False):
        self.id, self.api, self.call, self.never_syncs, self.prune, self.calibration = id, api, call, never_syncs, prune, calibration

    def __repr__(self):
        return self.id


def _entries():
    out = []
    for name, api, fn, modes in CALIBRATIONS:
        for mode in modes:
            out.append(Entry(f"{'+'.join(api)}-{name}-{mode}", api, functools.partial(fn, scores=mode == "scores"),
                             prune=PRUNE_EXPECT.get(name) if mode == "memo" else None, calibration=True))
    for fn, api in ((linear_steps, "LinearStepper"), (qk_steps, "MatMulStepper"), (sos_steps, "MatMulStepper"), (conv_steps, "ConvStepper")):
        out.append(Entry(f"{api}-{fn.__name__}", (api,), fn))
    out.append(Entry("calibrate_group-3_linear_1_matmul", ("calibrate_group", "linear_job", "matmul_job"), small_group))
    for fn in (linear_forward, matmul_forward, matmul_blocks_forward, mlp_forward, attn_forward, window_attn_forward, qkv_attn_forward):
        name = fn.__name__.replace("_forward", "_quant_forward")
        out.append(Entry(name, (name,), fn, never_syncs=True))
    for fn in (quantize_i8, pack_plane_i8, fake_quant, export_quantize):
        out.append(Entry(fn.__name__, (fn.__name__,), fn, never_syncs=True))
    for fn in (score_argmax_gather, multi_copy):
        out.append(Entry(fn.__name__, (fn.__name__,), fn))
    return out


ENTRIES = _entries()
BY_ID = {e.id: e for e in ENTRIES}
assert len(BY_ID) == len(ENTRIES)
