"""GPU: MatMul row / column sub-blocks (n_V, n_H > 1) -- k_pack_seg / k_sweep_seg behind the p4v_matmul_blocks_* entry points.

Fixtures tests/golden/mmblk_*.npz were made by running the reference's own classes (tools/gen_golden_mmblk.py).
  1  exact integer data: every partial sum is representable, the int8 forward must equal the float64 product bit for bit
     (pins the segment table, the scale tables and the MFMA row / column maps; B is not symmetric)
  2  quant_forward of the modules against the reference's output, through the int8 entry point
  3  the fused search against the reference: every score table, every selection, the intervals
  4  the granular entry points chained like the reference's methods = the fused call, bit for bit
  5  the non-batching classes (configured group counts) against their fixtures
  6  through HessianQuantCalibrator (grouped launches) on the mini ViT
  7  boundaries: cosine, n_V = 9, and (1, 1, 1, 1) makes the head-wise launches
"""
import copy
import json

import numpy as np
import pytest
import torch

from tests.helpers import (SCORE_RTOL, assert_argmax_tie_aware, assert_scores_close, golden_names, load_golden, record_margin)

pytestmark = pytest.mark.gpu

NAMES = golden_names("mmblk_")
BATCHING = [n for n in NAMES if not n.startswith("mmblk_ptqsl_")]
NONBATCHING = [n for n in NAMES if n.startswith("mmblk_ptqsl_")]


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    return engine


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _blocks(p):
    sos = p.get("sos", False)
    return ((1, 1) if sos else (p.get("n_V_A", 1), p.get("n_H_A", 1))) + (p.get("n_V_B", 1), p.get("n_H_B", 1))


def _module(g, batching):
    from ptq4vit_amd.quant_layers import matmul as mm
    p = dict(g["params"])
    p.pop("kind")
    sos = p.pop("sos")
    cls = {(True, False): mm.PTQSLBatchingQuantMatMul, (True, True): mm.SoSPTQSLBatchingQuantMatMul,
           (False, False): mm.PTQSLQuantMatMul, (False, True): mm.SoSPTQSLQuantMatMul}[(batching, sos)]
    m = cls(**p)
    m.raw_input, m.raw_out = [_t(g["A"]), _t(g["B"])], _t(g["out"])
    m.raw_grad = _t(g["grad"]) if p["metric"] == "hessian" else None
    return m, p, sos


# ---- 1 ---------------------------------------------------------------------------------------------------------------
def _block_scales(rng_exp, H, nV, nH):
    """Distinct powers of two per block, another set per head."""
    e = np.arange(nV * nH).reshape(nV, nH)[None] + np.arange(H)[:, None, None] + rng_exp
    return (2.0 ** -e).astype(np.float32)


def _expand(s, rows, cols):
    """[H][nV][nH] block values -> [H][rows][cols] (blocks of ceil(dim / n), reference matmul.py:109-122)."""
    H, nV, nH = s.shape
    cr, cc = -(-rows // nV), -(-cols // nH)
    return s[:, np.arange(rows) // cr][:, :, np.arange(cols) // cc]


@pytest.mark.parametrize("shape,blocks", [((1, 2, 133, 70, 37), (2, 2, 3, 2)), ((1, 1, 5, 9, 5), (1, 2, 4, 1))])
def test_forward_is_exact_on_integer_data(eng, shape, blocks):
    b, H, M, K, N = shape
    nVA, nHA, nVB, nHB = blocks
    rng = np.random.default_rng(5)
    sA, sB = _block_scales(0, H, nVA, nHA), _block_scales(1, H, nVB, nHB)
    kA = rng.integers(-4, 5, size=(b, H, M, K)).astype(np.float32)
    kB = rng.integers(-4, 5, size=(b, H, K, N)).astype(np.float32)
    kB[..., 0, :] = 4.0                     # not symmetric in any sense: a transposed or shifted tile map shows
    kB[..., :, 0] = -3.0
    A = kA * _expand(sA, M, K)[None]
    B = kB * _expand(sB, K, N)[None]
    if shape == (1, 1, 5, 9, 5):
        # K = 9 in 4 row blocks of 3: the fourth is empty (interval 0, as the search leaves it); cuts 3, 5, 6: a length-1 segment
        sB = sB.copy()
        sB[:, 3] = 0.0
    want = A.astype(np.float64) @ B.astype(np.float64)
    got = eng.matmul_blocks_quant_forward(A=_t(A), B=_t(B), A_interval=_t(sA), B_interval=_t(sB), split=None, A_bit=8,
                                          B_bit=8, blocks=blocks)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all()
    bad = np.argwhere(got.astype(np.float64) != want)
    assert bad.size == 0, f"{len(bad)} of {want.size} outputs differ, first at {bad[0]}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("shape,blocks", [((1, 2, 133, 70, 37), (1, 1, 3, 2)), ((1, 1, 5, 9, 5), (1, 1, 4, 1))])
def test_forward_is_exact_on_integer_data_with_the_twin_planes(eng, shape, blocks):
    """Split-of-softmax A on a 2-bit grid (q - 1 = 1: both range scales, 1 and the split 2^-3, are powers of two)."""
    from ptq4vit_amd.quant_layers.matmul import SoSPTQSLBatchingQuantMatMul
    b, H, M, K, N = shape
    _, _, nVB, nHB = blocks
    rng = np.random.default_rng(6)
    split = 0.125
    A = rng.choice(np.array([0.0, 0.03125, 0.0625, 0.125, 0.25, 0.5, 0.75, 1.0], dtype=np.float32), size=(b, H, M, K))
    sB = _block_scales(1, H, nVB, nHB)
    kB = rng.integers(-4, 5, size=(b, H, K, N)).astype(np.float32)
    kB[..., 0, :] = 4.0
    kB[..., :, 0] = -3.0
    B = kB * _expand(sB, K, N)[None]
    m = SoSPTQSLBatchingQuantMatMul(A_bit=2, B_bit=8, split=torch.tensor(split, dtype=torch.float64))
    want = (m.quant_input_A(torch.from_numpy(A).double()) @ torch.from_numpy(B).double()).numpy()
    assert len(np.unique(m.quant_input_A(torch.from_numpy(A).double()).numpy())) == 3          # 0, split, 1 + split
    got = eng.matmul_blocks_quant_forward(A=_t(A), B=_t(B), A_interval=torch.tensor([split]), B_interval=_t(sB),
                                          split=torch.tensor([split]), A_bit=2, B_bit=8, blocks=blocks, sos=True)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    bad = np.argwhere(got.astype(np.float64) != want)
    assert bad.size == 0, f"{len(bad)} of {want.size} outputs differ, first at {bad[0]}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


# ---- 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_module_quant_forward_vs_reference_output(eng, name, monkeypatch):
    g = load_golden(name)
    m, p, sos = _module(g, batching=name in BATCHING)
    dev = torch.device("cuda")
    m.A_interval, m.B_interval = _t(g["A_interval"]), _t(g["B_interval"])
    if sos:
        m.split = _t(g["split"])
    m.calibrated, m.mode = True, "quant_forward"
    calls = []
    orig = eng.matmul_blocks_quant_forward
    monkeypatch.setattr(eng, "matmul_blocks_quant_forward", lambda **kw: calls.append(kw["blocks"]) or orig(**kw))
    with torch.no_grad():
        out = m(*m.raw_input)
    assert calls == [_blocks(dict(p, sos=sos))], "quant_forward did not take the int8 sub-block entry point"
    assert out.device.type == dev.type
    got, ref = out.cpu().numpy().astype(np.float64), g["quant_forward"].astype(np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref).max() / np.abs(ref).max()
    bar = 2e-6 * g["A"].shape[-1] ** 0.5          # the project's bar (tests/test_hip_planes.py::_close_to_reference)
    print(f"[quant_forward] {name}: max |diff| / max |ref| = {err:.2e} (bar {bar:.2e})")
    record_margin("quant_forward_rel_err_over_bar", err / bar)
    assert err <= bar, f"{name}: {err:.3e} > {bar:.3e}"


# ---- 3 ---------------------------------------------------------------------------------------------------------------
def _fused(eng, g, p, sos):
    return eng.matmul_calibrate(A=_t(g["A"]), B=_t(g["B"]), out=_t(g["out"]),
                                grad=_t(g["grad"]) if p["metric"] == "hessian" else None, A_bit=p["A_bit"], B_bit=p["B_bit"],
                                metric=p["metric"], eq_alpha=p["eq_alpha"], eq_beta=p["eq_beta"], eq_n=p["eq_n"],
                                search_round=p["search_round"], sos=sos, want_scores=True, blocks=_blocks(dict(p, sos=sos)))


@pytest.mark.parametrize("name", BATCHING)
def test_fused_search_vs_reference(eng, name):
    g = load_golden(name)
    p = dict(g["params"])
    sos = p["sos"]
    A_iv, B_iv, split, scores, best = _fused(eng, g, p, sos)
    torch.cuda.synchronize()
    scores, best = scores.cpu().numpy(), best.cpu().numpy()
    R, steps = scores.shape[:2]
    assert R * steps == len(g["scores"]), (scores.shape, len(g["scores"]))
    flips = 0
    for r in range(R):
        for s in range(steps):
            ref = g["scores"][r * steps + s]
            what = f"{name}[round {r} step {s}]"
            if sos and s == 0:                       # the split table: 20 rows, one column
                assert_scores_close(scores[r, 0, :20, 0], ref.reshape(-1), what=what)
                flips += assert_argmax_tie_aware(best[r, 0, :1], ref.reshape(-1, 1), what=what)
                continue
            assert_scores_close(scores[r, s], ref.reshape(ref.shape[0], -1), what=what)
            flips += assert_argmax_tie_aware(best[r, s], ref.reshape(ref.shape[0], -1), what=what)
    A_iv, B_iv = A_iv.cpu().numpy(), B_iv.cpu().numpy()
    assert not np.isnan(scores).any() and not np.isnan(A_iv).any() and not np.isnan(B_iv).any()
    print(f"[parity] {name}: {R * steps} tables, {flips} differing selections")
    if flips == 0:
        np.testing.assert_array_equal(A_iv.reshape(-1), np.asarray(g["A_interval"]).reshape(-1))
        np.testing.assert_array_equal(B_iv.reshape(-1), g["B_interval"].reshape(-1))
        if sos:
            assert float(split.cpu()) == float(g["split"])
    if name == "mmblk_empty_block":
        H = g["A"].shape[1]
        assert np.all(A_iv.reshape(H, 4, 1)[:, 3] == 0) and np.all(B_iv.reshape(H, 1, 4)[:, :, 3] == 0)
        assert np.all(A_iv.reshape(H, 4, 1)[:, :3] > 0) and np.all(B_iv.reshape(H, 1, 4)[:, :, :3] > 0)


# ---- 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mmblk_qk_hessian_vA2hA2_vB2hB3", "mmblk_sos_hessian_vB2hB2", "mmblk_empty_block"])
def test_granular_sequence_equals_fused_call(eng, name):
    g = load_golden(name)
    fused, p, sos = _module(g, batching=True)
    fused.calibration_step2()
    m, _, _ = _module(g, batching=True)
    m._initialize_intervals()
    mult = torch.tensor([m.eq_alpha + i * (m.eq_beta - m.eq_alpha) / m.eq_n for i in range(m.eq_n + 1)]).cuda().view(-1, 1, 1, 1, 1, 1, 1, 1)
    B_cands = mult * m.B_interval.unsqueeze(0)
    A_cands = None if sos else mult * m.A_interval.unsqueeze(0)
    for _ in range(m.search_round):
        if sos:
            m._search_best_A_interval()
        else:
            m._search_best_A_interval(A_cands)
        m._search_best_B_interval(B_cands)
    torch.cuda.synchronize()
    assert m.B_interval.shape == fused.B_interval.shape == (1, g["A"].shape[1], 1, m.n_V_B, 1, m.n_H_B, 1)
    assert torch.equal(m.B_interval, fused.B_interval)
    assert torch.equal(torch.as_tensor(m.A_interval), torch.as_tensor(fused.A_interval))
    if sos:
        assert m.A_interval.shape == () and torch.equal(m.split, fused.split)
    else:
        assert m.A_interval.shape == (1, g["A"].shape[1], 1, m.n_V_A, 1, m.n_H_A, 1)


# ---- 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NONBATCHING)
def test_nonbatching_module_vs_reference(eng, name, monkeypatch):
    g = load_golden(name)
    m, p, sos = _module(g, batching=False)
    A, B = m.raw_input
    b, H = g["A"].shape[:2]
    seen = []

    class Spy(eng.MatMulStepper):
        def search_block(self, operand, *a, **k):
            r = super().search_block(operand, *a, **k)
            seen.append((operand, r[1].cpu().numpy()))
            return r

        def search_split(self, *a, **k):
            r = super().search_split(want_scores=True)
            seen.append(("split", r[2].cpu().numpy()))
            return r

    monkeypatch.setattr(eng, "MatMulStepper", Spy)
    with torch.no_grad():
        qf = m.calibration_step2(A, B)
    assert m.calibrated and len(seen) == len(g["scores"])
    nGA, nGB = (1 if sos else p.get("n_G_A", 1)), p.get("n_G_B", 1)
    flips = 0
    for i, ((kind, tab), ref) in enumerate(zip(seen, g["scores"])):
        what = f"{name}[{i}:{kind}]"
        if kind == "split":
            got = tab / b                                  # sum over the batch of means -> one mean (matmul.py:335)
            ref = ref.reshape(-1, 1)
        else:
            nG = nGA if kind == "A" else nGB
            crb = -(-H // nG)
            got = np.zeros((tab.shape[0], nG), dtype=np.float64)
            for h in range(H):
                got[:, h // crb] += tab[:, h]
            got /= b * crb                                 # matmul.py:199-205: mean over the batch and the crb heads incl. padding
        assert_scores_close(got, ref.reshape(ref.shape[0], -1), what=what)
        flips += assert_argmax_tie_aware(np.argmax(got, axis=0), ref.reshape(ref.shape[0], -1), what=what)
    assert tuple(m.B_interval.shape) == g["B_interval"].shape == (1, nGB, 1, p.get("n_V_B", 1), 1, p.get("n_H_B", 1), 1)
    print(f"[parity] {name}: {len(seen)} group-folded tables, {flips} differing selections")
    if flips == 0:
        np.testing.assert_array_equal(m.B_interval.cpu().numpy(), g["B_interval"])
        np.testing.assert_array_equal(np.asarray(torch.as_tensor(m.A_interval).cpu()).reshape(-1), np.asarray(g["A_interval"]).reshape(-1))
        if sos:
            assert float(m.split) == float(g["split"])
        got, ref = qf.cpu().numpy().astype(np.float64), g["quant_forward"].astype(np.float64)
        assert np.abs(got - ref).max() <= 2e-6 * g["A"].shape[-1] ** 0.5 * np.abs(ref).max()


# ---- 6 ---------------------------------------------------------------------------------------------------------------
def test_calibrator_with_sub_block_matmuls(eng, monkeypatch):
    from ptq4vit_amd import _lib
    from ptq4vit_amd.configs import PTQ4ViT
    from ptq4vit_amd.quant_layers.matmul import PTQSLBatchingQuantMatMul
    from ptq4vit_amd.utils import models, net_wrap
    from ptq4vit_amd.utils.quant_calib import HessianQuantCalibrator
    g = np.load("tests/golden/minivit_ptq4vit.npz", allow_pickle=False)
    kw = json.loads(str(g["model_kwargs"]))
    images = torch.from_numpy(g["images"]).cuda()
    monkeypatch.setitem(PTQ4ViT.ptqsl_matmul_kwargs, "n_V_A", 2)
    monkeypatch.setitem(PTQ4ViT.ptqsl_matmul_kwargs, "n_H_A", 2)
    monkeypatch.setitem(PTQ4ViT.ptqsl_matmul_kwargs, "n_V_B", 2)
    monkeypatch.setitem(PTQ4ViT.ptqsl_matmul_kwargs, "n_H_B", 2)
    net = models.get_net("vit_tiny_patch16_224", seed=0, device="cuda", **kw)
    wrapped = net_wrap.wrap_modules_in_net(net, PTQ4ViT)
    matmuls = {n: m for n, m in wrapped.items() if isinstance(m, PTQSLBatchingQuantMatMul)}
    assert len(matmuls) >= 4
    fresh = {n: copy.deepcopy(m) for n, m in matmuls.items()}
    caps = {}
    for n, m in matmuls.items():
        def rec(_o=m.calibration_job, _m=m, _n=n):
            caps[_n] = ([t.clone() for t in _m.raw_input], _m.raw_out.clone(), _m.raw_grad.clone())
            return _o()
        m.calibration_job = rec
    kinds = []
    orig_group = eng.calibrate_group
    monkeypatch.setattr(eng, "calibrate_group", lambda jobs, **k: kinds.extend(j.kind for j in jobs) or orig_group(jobs, **k))

    class Loader:
        batch_size = images.shape[0]

        def __iter__(self):
            yield images, torch.zeros(images.shape[0], dtype=torch.long)

    HessianQuantCalibrator(net, wrapped, Loader(), sequential=False, batch_size=4).batching_quant_calib()
    assert set(caps) == set(matmuls) and kinds.count(_lib.JOB_MATMUL_BLOCKS) == len(matmuls)
    for n, m in matmuls.items():
        H = caps[n][0][0].shape[1]
        assert m.calibrated and tuple(m.B_interval.shape) == (1, H, 1, 2, 1, 2, 1), n
        if m._sos:
            assert m.A_interval.shape == () and m.split.shape == ()
        else:
            assert tuple(m.A_interval.shape) == (1, H, 1, 2, 1, 2, 1), n
        alone = fresh[n]
        alone.raw_input, alone.raw_out, alone.raw_grad = caps[n]
        alone.calibration_step2()
        assert torch.equal(alone.B_interval, m.B_interval), n
        assert torch.equal(torch.as_tensor(alone.A_interval), torch.as_tensor(m.A_interval)), n
        if m._sos:
            assert torch.equal(alone.split, m.split), n
    calls = []
    orig_fwd = eng.matmul_blocks_quant_forward
    monkeypatch.setattr(eng, "matmul_blocks_quant_forward", lambda **k: calls.append(1) or orig_fwd(**k))
    with torch.no_grad():
        assert torch.isfinite(net(images)).all()      # every module now runs in quant_forward mode
    assert len(calls) == len(matmuls)


# ---- 7 ---------------------------------------------------------------------------------------------------------------
def test_cosine_with_sub_blocks_is_refused(eng):
    g = load_golden("mmblk_qk_hessian_vA2hA2_vB2hB3")
    m, _, _ = _module(g, batching=True)
    m.metric = "cosine"
    with pytest.raises(NotImplementedError, match="cosine"):
        m.calibration_step2()


def test_more_than_eight_blocks_are_refused(eng):
    g = load_golden("mmblk_qk_hessian_vA2hA2_vB2hB3")
    m, _, _ = _module(g, batching=True)
    m.n_V_A = 9
    with pytest.raises(NotImplementedError, match="8"):
        m.calibration_step2()


def test_headwise_module_makes_the_headwise_launches(eng):
    """All four block counts 1: the launches of the head-wise engine call, none of them the segment kernels."""
    g = load_golden("matmul_qk_hessian_w8a8")
    p = dict(g["params"])
    p.pop("kind")
    sos = p.pop("sos")
    args = dict(A=_t(g["A"]), B=_t(g["B"]), out=_t(g["out"]), grad=_t(g["grad"]), sos=sos, **p)

    def counted(run):
        eng.launch_counters(reset=True)
        eng.stats_reset()
        eng.stats_enable(True)
        try:
            res = run()
            torch.cuda.synchronize()
            kernels = [r["kernel"] for r in eng.stats_launches()]
        finally:
            eng.stats_enable(False)
        return res, eng.launch_counters(), kernels

    from ptq4vit_amd.quant_layers.matmul import PTQSLBatchingQuantMatMul

    def through_module():
        m = PTQSLBatchingQuantMatMul(n_V_A=1, n_H_A=1, n_V_B=1, n_H_B=1, **p)
        m.raw_input, m.raw_out, m.raw_grad = [args["A"], args["B"]], args["out"], args["grad"]
        m.calibration_step2()
        return m.A_interval.reshape(-1), m.B_interval.reshape(-1)

    (A1, B1), n1, k1 = counted(through_module)
    (A0, B0, _, _, _), n0, k0 = counted(lambda: eng.matmul_calibrate(**args))
    assert n1 == n0 and k1 == k0 and k0 and "k_sweep_seg" not in k1
    assert torch.equal(A1, A0) and torch.equal(B1, B0)
    # ... and the segment kernels do run where there are blocks
    gb = load_golden("mmblk_qk_hessian_vA2hA2_vB2hB3")
    mb, _, _ = _module(gb, batching=True)
    _, _, kb = counted(mb.calibration_step2)
    assert set(kb) == {"k_sweep_seg"}
