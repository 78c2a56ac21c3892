"""GPU: MatMul operands in any memory layout, through every entry point and every sweep route.

p4v_matmul_desc carries a_stride[4] / b_stride[4], and engine.py hands A.stride() / B.stride() through without a copy.  The rest
of the suite runs two layouts (A dense; B dense or k transposed in memory); a network hands over views of the packed qkv tensor.
A wrong stride pairing in one host planner branch would not fault -- it would read other plausible floats -- so every case here
holds the call on a view to the call on the canonical tensors BIT FOR BIT (the values are the same and no kernel's order of
summation depends on the source layout), including the list of (kernel, stage) the call launched, and the canonical call
itself to the oracle, so that "equal to the copy" cannot mean "equally wrong".

The views come from tests/matmul_layouts.py: each inside an allocation of its own, NaN everywhere around its elements (row gaps,
the sibling q / k / v slices, margins of three times its buffer), so a read through a wrong stride shows as NaN.  After EVERY
call the operands' allocations are compared with their state before it: no entry point stores to A or B.

Layouts are not crossed: A over all of its layouts with B canonical, B over all of its layouts with A canonical, and the pair as
the network hands it over (q and k^T of ONE packed buffer; dense probabilities with the v slice of a packed buffer).

With $P4V_MARGINS_OUT set the kernels recorded per case and the number of tensors compared are written there
(profiles/r30_matmul_layouts_margins.json)."""
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import fused_window_reference as fw
from tests import matmul_layouts as ml
from tests.helpers import assert_argmax_tie_aware, assert_scores_close, load_golden, record_margin, record_note
from tests.workspace_guard import Guard

pytestmark = pytest.mark.gpu

B_IMG, HEADS = 2, 3
HP = dict(eq_alpha=0.01, eq_beta=1.2, eq_n=100, search_round=2)
FORCE_PRUNE, CROSS_CHECK = 8388608, 134217728      # debug_variant bits (tests/test_hip_parity.py, tests/test_hip_production_path.py)
SPLIT = 2.0 ** -5

Shape = namedtuple("Shape", "name kind M K N metric golden routes", defaults=("hessian", None, ()))
#              id             operands              metric     fixture                             kernels the canonical calls must record
# (the plan as stats_launches() showed it: below 64 rows per (image, head) plan_prune keeps the full sweep, so qk_w7 has no pruned
# route; at 130 x 130 the 128-tiles of k_sweep8 would be 3.2 x padding and the 16 x 16 blocks of k_sweep9 sweep instead, slices
# included; k_sweep8 keeps sizes whose 128-tiles carry less than 1.4 x padding and k_slice_a takes at most 208 keys, which a square
# q k^T meets together from 97 to 128 tokens only: 113 = 7 x 16 + 1; at 233 x 233 -- two ragged 128-tiles per side -- the full
# sweep and stages B1 / B2 run k_sweep8 and the 16-row slices of stage A the 16 x 16 blocks of k_sweep9)
SHAPES = [Shape("qk_w7",      "qk", 49, 32, 49,     routes=("k_sweep9",)),
          Shape("qk_130",     "qk", 130, 64, 130,   routes=("k_sweep9:full", "k_sweep9:B1", "k_sweep9:B2", "k_slice_a", "k_slice_b")),
          Shape("qk_113",     "qk", 113, 64, 113,   routes=("k_sweep8:full", "k_sweep8:B1", "k_sweep8:B2", "k_slice_a", "k_slice_b")),
          Shape("qk_233",     "qk", 233, 64, 233,   routes=("k_sweep8:full", "k_sweep8:B1", "k_sweep8:B2", "k_sweep9:A")),
          Shape("qk_d96",     "qk", 129, 96, 129,   routes=("k_sweep2",)),
          Shape("sv_65",      "sv", 65, 65, 64,     routes=("k_sos_split:A", "k_sos_split:B1", "k_sos_split:B2", "k_sweep2", "k_slice_b")),
          Shape("sv_130_n40", "sv", 130, 130, 40,   routes=("k_sos_split:A", "k_sos_split:B1", "k_sos_split:B2")),
          Shape("sv_257",     "sv", 257, 257, 64,   routes=("k_sweep<float>",)),
          Shape("qk_cos",     "qk", 49, 32, 49,     "cosine", routes=("k_sweep2",)),
          Shape("blk_qk",     "qk", 13, 8, 13,      golden="mmblk_qk_hessian_vA2hA2_vB2hB3", routes=("k_sweep_seg",)),
          Shape("blk_sv",     "sv", 13, 13, 8,      golden="mmblk_sos_hessian_vB2hB2", routes=("k_sweep_seg",))]
SHAPE_IDS = [s.name for s in SHAPES]
# Layouts the plan routes to ANOTHER sweep kernel on purpose: {(shape, pair label, entry point): reason}.  Such a case names both
# kernel lists in its failure / margins and is held to the oracle with the helpers of tests/helpers.py at their constants instead
# of to the canonical bits.  Anything not listed here that records another list is a failure.
ROUTE_EXCEPTIONS = {}

Pair = namedtuple("Pair", "label A B canon")       # canon: key of the canonical operands this pair's values equal
_KERNELS = set()                                   # every "kernel:stage" a call of this file recorded


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    yield engine
    engine.debug_variant(0)
    engine.stats_enable(False)
    engine.release_workspace()
    _OPS.clear()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


class _Operands:
    """Everything one shape's tests share, built once: the canonical tensors, raw_out / raw_grad, every layout of A and of B on the
    GPU with a copy of its allocation as it was, and the (A, B) pairs to run."""

    def __init__(self, shape):
        self.shape, self.sos = shape, shape.kind == "sv"
        role_B = "B_sv" if self.sos else "B_qk"
        if shape.golden:
            g = self.golden = load_golden(shape.golden)
            p = g["params"]
            A, B = torch.from_numpy(g["A"].copy()), torch.from_numpy(g["B"].copy())
            out, grad = torch.from_numpy(g["out"].copy()), torch.from_numpy(g["grad"].copy())
            self.blocks = ((1, 1) if self.sos else (p["n_V_A"], p["n_H_A"])) + (p["n_V_B"], p["n_H_B"])
        else:
            gen = torch.Generator().manual_seed(3000 + SHAPE_IDS.index(shape.name))
            f = torch.linspace(0.5, 2.0, HEADS).view(1, HEADS, 1, 1)
            if self.sos:
                A = torch.softmax(torch.randn(B_IMG, HEADS, shape.M, shape.K, generator=gen) * 3, -1)
                B = torch.randn(B_IMG, HEADS, shape.K, shape.N, generator=gen) * f
            else:
                A = torch.randn(B_IMG, HEADS, shape.M, shape.K, generator=gen) * shape.K ** -0.5 * f
                B = torch.randn(B_IMG, HEADS, shape.K, shape.N, generator=gen) * f.flip(1)
            out = A @ B
            grad = torch.randn(out.shape, generator=gen) * 1e-3
            self.blocks = None
        assert A.shape[2:] == (shape.M, shape.K) and B.shape[2:] == (shape.K, shape.N)
        self.A_cpu, self.B_cpu, self.out_cpu, self.grad_cpu = A, B, out, grad
        self.out, self.grad = out.cuda(), (None if shape.metric == "cosine" else grad.cuda())
        self.hp = dict(A_bit=8, B_bit=8, metric=shape.metric, sos=self.sos)
        self.before = {}
        A_views = {n: self._keep(v) for n, v in ml.layouts(A, "A").items()}
        B_views = {n: self._keep(v) for n, v in ml.layouts(B, role_B).items()}
        cA, cB = ml.canonical_name("A"), ml.canonical_name(role_B)
        self.canon = {"": (A_views[cA], B_views[cB]),
                      "A_broadcast": (self._keep(ml.layouts(ml.canonical_of(A, "batch_broadcast"), "A")[cA]), B_views[cB]),
                      "B_broadcast": (A_views[cA], self._keep(ml.layouts(ml.canonical_of(B, "batch_broadcast"), role_B)[cB]))}
        self.pairs = [Pair(f"A:{n}", v, B_views[cB], "A_broadcast" if n == "batch_broadcast" else "") for n, v in A_views.items() if n != cA]
        self.pairs += [Pair(f"B:{n}", A_views[cA], v, "B_broadcast" if n == "batch_broadcast" else "") for n, v in B_views.items() if n != cB]
        if self.sos:
            _, _, v = ml.packed_qkv_views(None, None, B)
            self.pairs.append(Pair("network", A_views[cA], self._keep(v), ""))
        else:
            q, kT, _ = ml.packed_qkv_views(A, B.transpose(-2, -1), None)
            moved = {}
            self.pairs.append(Pair("network", self._keep(q, moved), self._keep(kT, moved), ""))
            assert self.pairs[-1].A.untyped_storage().data_ptr() == self.pairs[-1].B.untyped_storage().data_ptr()
        for p in self.pairs:
            assert torch.equal(p.A, self.canon[p.canon][0]) and torch.equal(p.B, self.canon[p.canon][1]), p.label
        self.ref = {}

    def _keep(self, view, moved=None):
        dev = ml.to_device(view, "cuda", moved)
        self.before[dev.untyped_storage().data_ptr()] = ml.allocation(dev).clone()
        return dev

    def untouched(self, *views):
        for v in views:
            was = self.before[v.untyped_storage().data_ptr()]
            assert torch.equal(_bits(ml.allocation(v)), _bits(was)), "the call stored into an operand's allocation"


_OPS = {}


def _ops(shape):
    if shape.name not in _OPS:
        _OPS[shape.name] = _Operands(shape)
    return _OPS[shape.name]


# ---- the entry points: fn(eng, ops, canon, A, B) -> the tensors the call returns -------------------------------------------------
def _search_kw(ops, A, B):
    kw = dict(A=A, B=B, out=ops.out, grad=ops.grad, **ops.hp, **HP)
    if ops.blocks:
        kw["blocks"] = ops.blocks
    return kw


def ep_scores(eng, ops, canon, A, B):
    return eng.matmul_calibrate(want_scores=True, **_search_kw(ops, A, B))


def _pruned(variant):
    def ep(eng, ops, canon, A, B):
        eng.prune_counters(reset=True)
        try:
            eng.debug_variant(variant)
            res = eng.matmul_calibrate(prune=True, **_search_kw(ops, A, B))
            torch.cuda.synchronize()
        finally:
            eng.debug_variant(0)
        cnt = eng.prune_counters()
        return res[:3] + (torch.tensor([cnt[k] for k in ("staged", "staged_no_survivors", "kept_full_sweep", "not_eligible")]),)
    return ep


def ep_init(eng, ops, canon, A, B):
    st = eng.MatMulStepper(A=A, B=B, out=ops.out, grad=ops.grad, eq_n=HP["eq_n"], blocks=ops.blocks, **ops.hp)
    return st.init_intervals()


def ep_stepper(eng, ops, canon, A, B):
    """The granular calls chained as the reference's methods chain them, on the candidate tables of the CANONICAL run's initial
    intervals (head-wise: search_A / search_split, search_B; sub-blocks: search_split, then search_block over every block)."""
    st = eng.MatMulStepper(A=A, B=B, out=ops.out, grad=ops.grad, eq_n=HP["eq_n"], blocks=ops.blocks, **ops.hp)
    mult = eng.candidate_multipliers(HP["eq_alpha"], HP["eq_beta"], HP["eq_n"], ops.out.device)
    init = _reference(eng, ops, canon, "init")[0]          # (split-of-softmax: B's alone)
    A0, B0 = (None if ops.sos else init[0]), init[-1]
    got, split = [], None
    if ops.sos:
        split, A_cur, scores, best = st.search_split(want_scores=True)
        got += [split, A_cur, scores, best]
    if not ops.blocks:
        if not ops.sos:
            A_cur, scores, best = st.search_A(mult[:, None] * A0[None], A0, B0, want_scores=True)
            got += [A_cur, scores, best]
        B_cur, scores, best = st.search_B(mult[:, None] * B0[None], A_cur, B0, split=split, want_scores=True)
        return got + [B_cur, scores, best]
    H, (nVA, nHA, nVB, nHB) = st.H, ops.blocks
    B_cur = B0
    for operand, nV, nH in (("A", nVA, nHA), ("B", nVB, nHB)):
        if operand == "A" and ops.sos:
            continue
        if operand == "A":
            A_cur = A0
        for v in range(nV):
            for h in range(nH):
                base = (A0 if operand == "A" else B0).view(H, nV, nH)[:, v, h]
                new, scores, best = st.search_block(operand, v, h, mult[:, None] * base[None], A_cur, B_cur, split=split, want_scores=True)
                A_cur, B_cur = (new, B_cur) if operand == "A" else (A_cur, new)
                got += [new, scores, best]
    return got


def ep_forward(eng, ops, canon, A, B):
    ref = _reference(eng, ops, canon, "scores")[0]
    A_iv, B_iv, split = ref[0], ref[1], (ref[2] if ops.sos else None)
    kw = dict(A=A, B=B, A_interval=A_iv, B_interval=B_iv, split=split, sos=ops.sos, A_bit=8, B_bit=8)
    return (eng.matmul_blocks_quant_forward(blocks=ops.blocks, **kw) if ops.blocks else eng.matmul_quant_forward(**kw),)


ENTRY = {"scores": ep_scores, "pruned": _pruned(FORCE_PRUNE), "pruned_cross_check": _pruned(FORCE_PRUNE | CROSS_CHECK),
         "init": ep_init, "stepper": ep_stepper, "forward": ep_forward}


def _call(eng, ops, canon, entry, A, B):
    """One call with launch recording on: (the returned tensors, [kernel:stage]); the operands' allocations checked after it."""
    eng.stats_enable(True)
    try:
        eng.stats_reset()
        res = ENTRY[entry](eng, ops, canon, A, B)
        torch.cuda.synchronize()
        kernels = [f"{r['kernel']}:{r['stage']}" for r in eng.stats_launches()]
    finally:
        eng.stats_enable(False)
    ops.untouched(A, B)
    _KERNELS.update(kernels)
    return [t.clone() for t in res if t is not None], kernels


def _reference(eng, ops, canon, entry):
    """The call on the canonical tensors (`canon`: which of them), once per shape and entry point."""
    key = (canon, entry)
    if key not in ops.ref:
        A, B = ops.canon[canon]
        res, kernels = _call(eng, ops, canon, entry, A, B)
        for t in res:
            assert not bool(torch.isnan(t).any()) and (t.dtype != torch.float32 or bool(torch.isfinite(t).all())), \
                f"{ops.shape.name} {entry}: the canonical call returns non-finite values"
        ops.ref[key] = (res, kernels)
    return ops.ref[key]


def _identical(got, ref, what):
    assert len(got) == len(ref), f"{what}: {len(got)} tensors, canonical {len(ref)}"
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: tensor {i}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        if not torch.equal(_bits(a), _bits(b)):
            bad = (_bits(a) != _bits(b)).flatten().nonzero().flatten()
            raise AssertionError(f"{what}: tensor {i} differs from the canonical call's at {bad.numel()} of {a.numel()} elements, first "
                                 f"{int(bad[0])}: {a.flatten()[bad[0]].item()!r} vs {b.flatten()[bad[0]].item()!r}; NaN: {int(torch.isnan(a.float()).sum())}")
    return len(got)


def _unique(kernels):
    return list(dict.fromkeys(kernels))


# ---- the canonical call against the oracle ----------------------------------------------------------------------------------------
def _check_tables(pairs, what):
    flips = 0
    for i, (got, best, ref) in enumerate(pairs):
        ref2 = ref.reshape(ref.shape[0], -1)
        got = got[: ref2.shape[0], : ref2.shape[1]]
        assert_scores_close(got, ref2, what=f"{what}[{i}]")
        flips += assert_argmax_tie_aware(best[: ref2.shape[1]], ref2, what=f"{what}[{i}]")
        np.testing.assert_array_equal(best[: ref2.shape[1]], np.argmax(got, axis=0), err_msg=f"{what}[{i}] select")
    return flips


def _held_to_the_oracle(ops, res, what):
    """`res` = (A_interval, B_interval, split, scores, best) of a fused search on ops' values: the bar of
    test_random_attention_geometries_vs_oracle (sub-blocks: of test_hip_mmblk.py::test_fused_search_vs_reference)."""
    A_iv, B_iv = res[0].cpu().numpy(), res[1].cpu().numpy()
    split = res[2] if ops.sos else None
    scores, best = res[-2].cpu().numpy(), res[-1].cpu().numpy()
    if ops.shape.golden:
        g = ops.golden
        R, steps = scores.shape[:2]
        assert R * steps == len(g["scores"])
        pairs = []
        for r in range(R):
            for s in range(steps):
                ref = g["scores"][r * steps + s]
                pairs.append((scores[r, 0][:20, :1], best[r, 0][:1], ref.reshape(-1, 1)) if ops.sos and s == 0 else (scores[r, s], best[r, s], ref))
        want = dict(A_interval=g["A_interval"], B_interval=g["B_interval"], split=g.get("split"))
    else:
        from oracle.ptq4vit_oracle import MatMulOracle
        o = MatMulOracle(sos=ops.sos, A_bit=8, B_bit=8, metric=ops.shape.metric, **HP)
        want = o.calibration_step2(ops.A_cpu.numpy(), ops.B_cpu.numpy(), ops.out_cpu.numpy(), ops.grad_cpu.numpy())
        pairs = []
        for r in range(HP["search_round"]):
            ta, tb = o.trace[2 * r][1], o.trace[2 * r + 1][1]
            pairs.append((scores[r, 0][:20, :1], best[r, 0][:1], ta) if ops.sos else (scores[r, 0], best[r, 0], ta))
            pairs.append((scores[r, 1], best[r, 1], tb))
    flips = _check_tables(pairs, what)
    if flips == 0:
        np.testing.assert_array_equal(B_iv.reshape(-1), np.asarray(want["B_interval"]).reshape(-1))
        np.testing.assert_array_equal(A_iv.reshape(-1), np.asarray(want["A_interval"]).reshape(-1))
        if ops.sos:
            assert float(split.cpu()) == float(want["split"])
    return flips


def _prunable(shape):
    """plan_prune stages a MatMul pass from 64 rows per (image, head) on; never the cosine metric or the sub-block search."""
    return shape.M >= 64 and shape.metric != "cosine" and not shape.golden


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_canonical_call_against_the_oracle_and_its_route(eng, shape):
    ops = _ops(shape)
    res, kernels = _reference(eng, ops, "", "scores")
    flips = _held_to_the_oracle(ops, res, f"{shape.name} canonical")
    seen = set(kernels) | {k.split(":")[0] for k in kernels}
    for entry in ("pruned", "pruned_cross_check"):
        r, k = _reference(eng, ops, "", entry)
        seen |= set(k) | {x.split(":")[0] for x in k}
        _identical(r[:-1], res[:3 if ops.sos else 2], f"{shape.name}: {entry} against the unpruned search")
    record_note("kernels", _unique(kernels))
    record_note("kernels_pruned", _unique(_reference(eng, ops, "", "pruned_cross_check")[1]))
    record_margin(None, None, {"near_tie_flips": flips})
    print(f"[layouts] {shape.name}: unpruned {_unique(kernels)}; pruned {_unique(_reference(eng, ops, '', 'pruned')[1])}; "
          f"counters {_reference(eng, ops, '', 'pruned')[0][-1].tolist()}")
    missing = [k for k in shape.routes if k not in seen]
    assert not missing, f"{shape.name} no longer reaches {missing}: recorded {sorted(seen)}"
    staged = int(_reference(eng, ops, "", "pruned")[0][-1][0])
    assert (staged > 0) == _prunable(shape), f"{shape.name}: {staged} passes of the forced pruned search ran in stages"


# ---- every pair through every entry point -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", list(ENTRY))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_every_layout_gives_the_canonical_bits(eng, shape, entry):
    ops = _ops(shape)
    compared, routes = 0, {}
    for p in ops.pairs:
        ref, ref_kernels = _reference(eng, ops, p.canon, entry)
        what = f"{shape.name} {entry} {p.label}"
        got, kernels = _call(eng, ops, p.canon, entry, p.A, p.B)
        if kernels != ref_kernels:
            reason = ROUTE_EXCEPTIONS.get((shape.name, p.label, entry))
            assert reason and entry == "scores", (f"{what}: launched another list of sweep kernels than the canonical call and no exception names "
                                                  f"it:\n  {_unique(kernels)}\n  {_unique(ref_kernels)}")
            routes[p.label] = dict(kernels=_unique(kernels), canonical=_unique(ref_kernels), reason=reason)
            _held_to_the_oracle(ops, got, what)
            continue
        compared += _identical(got, ref, what)
    record_note("kernels", _unique(_reference(eng, ops, "", entry)[1]))
    if routes:
        record_note("other_routes", routes)
    record_margin(None, None, {"layout_pairs": len(ops.pairs), "tensors_compared": compared})
    if entry.startswith("pruned") and _prunable(shape):
        assert int(_reference(eng, ops, "", entry)[0][-1][0]) > 0, "no staged pass"


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_group_members_of_different_layouts_equal_their_single_calls(eng, shape):
    ops = _ops(shape)
    compared = 0
    job = lambda p: eng.matmul_job(**_search_kw(ops, p.A, p.B))
    single = {c: [t.clone() for t in eng.run_job(job(Pair("", *ops.canon[c], c))).outputs if t is not None] for c in ops.canon}
    n, third = len(ops.pairs), -(-len(ops.pairs) // 3)
    for i in range(third):                      # every pair is a member once; a group mixes layouts of A, of B and the network's
        members = [ops.pairs[(i + k * third) % n] for k in range(3)]
        assert len({p.label for p in members}) == 3 and len({(tuple(p.A.stride()), tuple(p.B.stride())) for p in members}) >= 2
        jobs = eng.calibrate_group([job(p) for p in members])
        torch.cuda.synchronize()
        for p, j in zip(members, jobs):
            got = [t.clone() for t in j.outputs if t is not None]
            ops.untouched(p.A, p.B)
            own = [t.clone() for t in eng.run_job(job(p)).outputs if t is not None]
            torch.cuda.synchronize()
            ops.untouched(p.A, p.B)
            compared += _identical(got, own, f"{shape.name} group member {p.label} against its single call")
            compared += _identical(got, single[p.canon], f"{shape.name} group member {p.label} against the canonical single call")
            assert all(bool(torch.isfinite(t).all()) for t in got)
    record_margin(None, None, {"layout_pairs": len(ops.pairs), "tensors_compared": compared})


# ---- the module level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["MinMaxQuantMatMul", "PTQSLBatchingQuantMatMul", "SoSPTQSLBatchingQuantMatMul"])
def test_modules_give_views_the_results_of_copies(eng, cls):
    """calibration_step2 on the GPU path and quant_forward, once per class: the network pair and the padded / offset views against
    the canonical tensors."""
    from ptq4vit_amd.quant_layers import matmul as mm
    ops = _ops(SHAPES[SHAPE_IDS.index("sv_65" if cls.startswith("SoS") else "qk_w7")])

    def run(A, B):
        if cls == "MinMaxQuantMatMul":
            # This class is plain torch: its product is torch's fp32 GEMM, whose order of summation follows the operands' layout.
            # Identity is asked of everything up to the product -- the intervals, both quantised operands --; the two products are
            # held to the float64 product of the quantised operands within the forward error bound of a length-K fp32 dot product
            # in any order, gamma_K sum |a| |b| with gamma_K = K u / (1 - K u) < (K + 1) u, u = 2^-24.
            m = mm.MinMaxQuantMatMul()
            with torch.no_grad():
                out = m.calibration_step2(A, B)
                fwd = m.quant_forward(A, B)
                Aq, Bq = m.quant_input(A, m.A_interval, m.A_qmax), m.quant_input(B, m.B_interval, m.B_qmax)
            exact, bound = Aq.double() @ Bq.double(), (A.shape[-1] + 1) * 2.0 ** -24 * (Aq.double().abs() @ Bq.double().abs())
            for t in (out, fwd):
                assert bool(((t.double() - exact).abs() <= bound).all()), "MinMaxQuantMatMul: product outside the fp32 dot-product bound"
            return [m.A_interval.reshape(-1), m.B_interval.reshape(-1), Aq, Bq]
        m = getattr(mm, cls)(metric="hessian", **HP)
        m.raw_input, m.raw_out, m.raw_grad = [A, B], ops.out, ops.grad
        m.calibration_step2()
        m.mode = "quant_forward"
        with torch.no_grad():
            out = m(A, B)
        torch.cuda.synchronize()
        return [m.A_interval.reshape(-1), m.B_interval.reshape(-1)] + ([m.split.reshape(-1)] if m._sos else []) + [out]

    ref = {c: run(*ops.canon[c]) for c in ops.canon}
    assert all(bool(torch.isfinite(t).all()) for t in ref[""])
    compared = 0
    for p in ops.pairs:
        got = run(p.A, p.B)
        ops.untouched(p.A, p.B)
        compared += _identical(got, ref[p.canon], f"{cls} {p.label}")
    record_margin(None, None, {"layout_pairs": len(ops.pairs), "tensors_compared": compared})


# ---- controls: the comparison sees one changed element, and a read of a sibling slice -------------------------------------------------
@pytest.mark.parametrize("name", ["qk_w7", "sv_65"])
def test_controls_one_changed_element_and_a_sibling_slice_show(eng, name):
    ops = _ops(SHAPES[SHAPE_IDS.index(name)])
    A, B = ops.canon[""]
    for entry in ("scores", "forward"):
        ref = _reference(eng, ops, "", entry)[0]
        B1 = B.clone()
        r, c = divmod(int(B1[1, 2].abs().argmax()), B1.shape[3])
        B1[1, 2, r, c] *= 0.5                              # ONE element: the largest of the last (image, head), halved
        got = [t.clone() for t in ENTRY[entry](eng, ops, "", A, B1) if t is not None]
        torch.cuda.synchronize()
        with pytest.raises(AssertionError, match="differs from the canonical"):
            _identical(got, ref, f"{name} {entry} control")
    # the q slice of a packed buffer read at the k slice's offset: NaN and nothing else
    p = next(p for p in ops.pairs if p.label == "A:packed_qkv_0")
    sibling = p.A.as_strided(p.A.shape, p.A.stride(), p.A.storage_offset() + p.A.stride(2) // 3)
    assert bool(torch.isnan(sibling).all())
    got = [t.clone() for t in ep_scores(eng, ops, "", sibling, B) if t is not None]
    torch.cuda.synchronize()
    ops.untouched(p.A)
    with pytest.raises(AssertionError, match="differs from the canonical"):
        _identical(got, _reference(eng, ops, "", "scores")[0], f"{name} sibling slice control")


# ---- the fused forwards -------------------------------------------------------------------------------------------------------------
class _Attention:
    """q, k^T, v of one attention shape in every layout, head-wise intervals with another factor per head."""

    def __init__(self, B, H, N, D, seed, window):
        gen = torch.Generator().manual_seed(seed)
        f = torch.linspace(0.6, 1.6, H).view(1, H, 1, 1)
        q, k, v = (torch.randn(B, H, N, D, generator=gen) for _ in range(3))
        q, k, v = q * f * D ** -0.25, k * f.flip(1) * D ** -0.25, v * f
        self.H, self.before = H, {}
        self.cpu = dict(q=q, kT=k.transpose(-2, -1).contiguous(), v=v)
        roles = dict(q="A", kT="B_qk", v="B_sv")
        self.views = {n: {l: self._keep(x) for l, x in ml.layouts(t, roles[n]).items()} for n, t in self.cpu.items()}
        self.canon_name = {n: ml.canonical_name(r) for n, r in roles.items()}
        canon = {n: self.views[n][self.canon_name[n]] for n in roles}
        self.triples = []                                   # (label, {q, kT, v}, which operand holds a broadcast batch or None)
        for n in roles:
            for l, x in self.views[n].items():
                if l != self.canon_name[n]:
                    self.triples.append((f"{n}:{l}", dict(canon, **{n: x}), n if l == "batch_broadcast" else None))
        moved = {}
        net = dict(zip(("q", "kT", "v"), (self._keep(x, moved) for x in ml.packed_qkv_views(q, k, v))))
        assert len({x.untyped_storage().data_ptr() for x in net.values()}) == 1
        self.triples.append(("network", net, None))
        self.canon = {None: canon}
        for n in roles:
            t = ml.canonical_of(self.cpu[n], "batch_broadcast")
            self.canon[n] = dict(canon, **{n: self._keep(ml.layouts(t, roles[n])[self.canon_name[n]])})
        iv = lambda x: (x.abs().amax(dim=(0, 2, 3)) / 127.5).cuda()
        self.qk = dict(A_interval=iv(q) * torch.tensor([1.0, 0.8, 1.25]).cuda(), B_interval=iv(k) * torch.tensor([0.9, 1.15, 1.0]).cuda(),
                       A_bit=8, B_bit=8)
        split = torch.tensor(SPLIT, device="cuda")
        self.pv = dict(A_interval=split / 127, B_interval=iv(v) * torch.tensor([1.2, 1.0, 0.85]).cuda(), split=split, sos=True, A_bit=8, B_bit=8)
        self.extra = dict(scale=1.0)
        if window:
            nW = 4
            rng = np.random.default_rng(seed)
            self.extra = dict(bias=(torch.randn(H, N, N, generator=gen) * 0.5).cuda(),
                              mask=torch.from_numpy(fw.shift_mask(nW + 1, N, rng, -100.0)[1:]).cuda())

    _keep = _Operands._keep
    untouched = _Operands.untouched


@pytest.mark.parametrize("kind,dims", [("attn", (2, 3, 130, 64)), ("wattn", (8, 3, 49, 32))], ids=["attention", "window_attention"])
def test_fused_forwards_give_every_layout_the_canonical_bits(eng, kind, dims):
    """attn_quant_forward at (2, 3, 130, 130, 64, 64) and window_attn_quant_forward at (8, 3, 49, 49, 32, 32) with bias and mask: out,
    probs and every byte of the planes."""
    at = _Attention(*dims, seed=3100 + len(kind), window=kind == "wattn")
    fn = eng.window_attn_quant_forward if kind == "wattn" else eng.attn_quant_forward

    def run(t):
        eng.stats_enable(True)
        try:
            eng.stats_reset()
            out, probs, planes = fn(q=t["q"], kT=t["kT"], v=t["v"], qk=at.qk, pv=at.pv, want_probs=True, want_planes=True, **at.extra)
            torch.cuda.synchronize()
            kernels = [f"{r['kernel']}:{r['stage']}" for r in eng.stats_launches()]
        finally:
            eng.stats_enable(False)
        at.untouched(*t.values())
        return [out.clone(), probs.clone()] + [p.clone() for p in planes], kernels

    ref = {c: run(t) for c, t in at.canon.items()}
    res, kernels = ref[None]
    assert len(res) == 4 and bool(torch.isfinite(res[0]).all()) and bool(torch.isfinite(res[1]).all())
    assert torch.allclose(res[1].sum(-1), torch.ones_like(res[1][..., 0]), atol=1e-5)
    assert not torch.equal(ref["q"][0][0], res[0]), "the broadcast operand's canonical tensor is another tensor"
    compared = 0
    for label, t, bcast in at.triples:
        got, k = run(t)
        assert k == ref[bcast][1], f"{kind} {label}: kernels {k}, canonical {ref[bcast][1]}"
        compared += _identical(got, ref[bcast][0], f"{kind} {label}")
    record_note("kernels", _unique(kernels))
    record_margin(None, None, {"layout_triples": len(at.triples), "tensors_compared": compared})


# ---- the workspace under guard ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["qk_w7", "sv_65"])
def test_strided_descriptors_size_their_workspace(eng, monkeypatch, name):
    """*_workspace_bytes is asked with the strided descriptor: the fused search and the forward of every layout in an exact,
    guarded workspace under both poisons -- the canonical bits, and no byte outside the declared size touched."""
    ops = _ops(SHAPES[SHAPE_IDS.index(name)])
    refs = {(c, e): _reference(eng, ops, c, e)[0] for c in ops.canon for e in ("scores", "forward")}
    calls = 0
    for poison in (0xFF, 0x00):
        with Guard(eng, monkeypatch, poison) as g:
            for p in ops.pairs:
                for entry in ("scores", "forward"):
                    got = [t.clone() for t in ENTRY[entry](eng, ops, p.canon, p.A, p.B) if t is not None]
                    _identical(got, refs[(p.canon, entry)], f"{name} {entry} {p.label} poison {poison:#04x}")
                    ops.untouched(p.A, p.B)
            reps = g.finish()
        assert len(reps) >= 2 * len(ops.pairs), f"the guard saw {len(reps)} calls"
        for r in reps:
            assert r["guard_changed"] == 0 and 0 < r["touched"] <= r["need"] == r["declared"], r
        calls += len(reps)
    record_margin(None, None, {"guarded_calls": calls})


# ---- the routes the file as a whole reaches ----------------------------------------------------------------------------------------
def test_the_file_reaches_every_sweep_route(eng):
    """The union of the kernels recorded above (every layout records the list of its canonical call, so the canonical calls of every
    shape are the union): a plan change that empties a row fails here."""
    for shape in SHAPES:
        for entry in ("scores", "pruned", "pruned_cross_check"):
            _reference(eng, _ops(shape), "", entry)
    names = {k.split(":")[0] for k in _KERNELS}
    # (as stats_launches() names them: "k_slice_b" is k_slice_b2's record, "k_sweep<float>" the generic kernel of the fp32 split fallback)
    want = {"k_sweep9", "k_sweep8", "k_sweep2", "k_slice_a", "k_slice_b", "k_sweep<float>", "k_sweep_seg"}
    record_note("kernels", sorted(_KERNELS))
    assert want <= names, f"not reached: {sorted(want - names)}; recorded {sorted(_KERNELS)}"
    assert {"k_sos_split:A", "k_sos_split:B1", "k_sos_split:B2"} <= _KERNELS, sorted(_KERNELS)
