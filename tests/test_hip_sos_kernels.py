"""The instances of k_sos_split (the split search of the split-of-softmax matmul) against the kernel as it was.

Tuning key 12 = 13 runs the previous kernel in every stage.  The default build path takes, per sweep, the paired instance
(slices of at most 16 rows: two candidates per 32-row MFMA tile, pairs dealt 3 / 3 / 2 / 2 over the four waves), the light
instance (few candidates over all rows: the two images of an element computed where they are used) or the resident one, all
with the one-burst prologue and the B tile in 16-byte loads where its layout allows.  None of this reorders a sum, so every
score table here must be BIT-identical to the previous kernel's on the same tensors."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_IMG, HEADS = 2, 3          # Z = 6 (image, head) pairs
FORCE_PRUNE, CROSS_CHECK = 8388608, 134217728     # debug_variant bits (tests/test_hip_parity.py, tests/test_hip_production_path.py)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    return engine


_cache = {}


def _mk(M, K, N, seed=5):
    """softmax(scores) . v operands: A [b][H][M][K] rows sum to 1, B [b][H][K][N]; raw_out and a raw_grad (made once per shape)."""
    key = (M, K, N, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed + 1000 * M + 10 * K + N)
        A = torch.softmax(torch.from_numpy(rng.standard_normal((B_IMG, HEADS, M, K)).astype(np.float32) * 3), -1)
        B = torch.from_numpy(rng.standard_normal((B_IMG, HEADS, K, N)).astype(np.float32)) * torch.linspace(0.5, 2.0, HEADS)[None, :, None, None]
        out = A @ B
        grad = torch.from_numpy((rng.standard_normal(out.shape) * 1e-3).astype(np.float32))
        _cache[key] = tuple(t.contiguous().cuda() for t in (A, B, out, grad))
    return _cache[key]


class _previous:
    """with _previous(eng): tuning 12 = 13, the previous kernel in every stage (other values: the crossover handles)."""

    def __init__(self, eng, value=13):
        self.eng, self.value = eng, value

    def __enter__(self):
        self.eng.debug_tuning(12, self.value)

    def __exit__(self, *exc):
        self.eng.debug_tuning(12, 0)


def _search(eng, A, B, out, grad, metric="hessian", bit=8):
    st = eng.MatMulStepper(A=A, B=B, out=out, grad=grad, A_bit=bit, B_bit=bit, metric=metric, eq_n=100, sos=True)
    split, A_iv, scores, best = st.search_split(want_scores=True)
    torch.cuda.synchronize()
    return split.clone(), A_iv.clone(), scores.clone(), best.clone()


def _same(new, old, what):
    for a, b, name in zip(new, old, ("split", "A_interval", "score table", "selection")):
        assert torch.equal(a, b), f"{what}: {name} differs from the previous kernel's\n{a.flatten()}\n{b.flatten()}"
    assert torch.isfinite(new[2]).all(), f"{what}: non-finite scores"


@pytest.mark.gpu
@pytest.mark.parametrize("N", [64, 40])
@pytest.mark.parametrize("S", [65, 130, 197])
def test_full_split_search_is_bit_identical(eng, S, N):
    """KS 72 and 100, ragged K, N < 64, a last 128-row half that is mostly padding: the 20-row table of the full search."""
    A, B, out, grad = _mk(S, S, N)
    new = _search(eng, A, B, out, grad)
    with _previous(eng):
        old = _search(eng, A, B, out, grad)
    assert new[2].shape == (20, 1)
    _same(new, old, f"full search {S}x{S}x{N}")


@pytest.mark.gpu
@pytest.mark.parametrize("M,K", [(16, 64), (16, 197), (9, 64), (9, 197), (24, 197)])
def test_slice_instances_are_bit_identical(eng, M, K):
    """M <= 16: the paired instance (KS 32 and 100); M = 24: the unpaired share path.  The 3 / 3 / 2 / 2 deal of whole pairs
    keeps every candidate's order of summation, so the tables are compared for identity."""
    A, B, out, grad = _mk(M, K, 64)
    new = _search(eng, A, B, out, grad)
    with _previous(eng):
        old = _search(eng, A, B, out, grad)
    _same(new, old, f"slice {M}x{K}")


@pytest.mark.gpu
@pytest.mark.parametrize("metric,bit", [("hessian", 8), ("L2_norm", 8), ("L1_norm", 6), ("linear_weighted_L2_norm", 8),
                                        ("square_weighted_L2_norm", 6)])
def test_every_epilogue_and_weight_mode(eng, metric, bit):
    """All four wt_modes / epilogues, 8 and 6 bit (qm1, lo_top), on the paired and on the resident instance."""
    for M, K, N in ((16, 130, 64), (130, 130, 40)):
        A, B, out, grad = _mk(M, K, N)
        new = _search(eng, A, B, out, grad, metric, bit)
        with _previous(eng):
            old = _search(eng, A, B, out, grad, metric, bit)
        _same(new, old, f"{metric} {bit} bit {M}x{K}x{N}")


def _sweep(eng, ops, **kw):
    A, B, out, grad = ops
    s = eng.debug_sos_sweep(A=A, B=B, out=out, grad=grad, A_bit=kw.pop("bit", 8), metric=kw.pop("metric", "hessian"), **kw)
    torch.cuda.synchronize()
    return s


def _check_range(s, crange, n, what):
    lo, hi = (0, n) if crange is None else crange
    inside = torch.zeros(n, dtype=torch.bool)
    inside[max(lo, 0):min(hi, n)] = True
    s = s.cpu()
    assert torch.isfinite(s[inside]).all(), f"{what}: an evaluated candidate has no finite score: {s}"
    assert (s[~inside] == -float("inf")).all(), f"{what}: entries outside the range are not what k_finish leaves there: {s}"


@pytest.mark.gpu
@pytest.mark.parametrize("crange,n", [((3, 8), 20), ((0, 1), 20), ((19, 20), 20), ((5, 5), 20), (None, 19), ((4, 19), 19), ((2, 7), 20)],
                         ids=["3-8", "0-1", "19-20", "empty", "C19", "C19-4-19", "2-7"])
def test_paired_instance_on_ranges_the_search_does_not_produce(eng, crange, n):
    """An odd candidate count, ranges that start or end inside a pair of the full table, a single candidate, none."""
    for M, K in ((16, 197), (9, 64)):
        ops = _mk(M, K, 64)
        new = _sweep(eng, ops, crange=crange, n_cands=n)
        with _previous(eng):
            old = _sweep(eng, ops, crange=crange, n_cands=n)
        assert torch.equal(new, old), f"paired instance {M}x{K} range {crange} of {n}:\n{new}\n{old}"
        _check_range(new, crange, n, f"paired instance {M}x{K} range {crange} of {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("known", [1, 2, 3])
@pytest.mark.parametrize("S,bit", [(65, 8), (197, 8), (197, 6)])
def test_light_instance_is_bit_identical(eng, S, bit, known):
    """known_cands 1-3 over all rows: the default choice (light up to the crossover count), the light instance forced
    (12 = 15) and the resident one forced (12 = 14) against the previous kernel; outside the range the sentinel -inf."""
    ops = _mk(S, S, 64)
    crange = (4, 4 + known)
    kw = dict(crange=crange, known_cands=known, bit=bit)
    with _previous(eng):
        old = _sweep(eng, ops, **kw)
    got = {"default": _sweep(eng, ops, **kw)}
    for value, name in ((15, "light"), (14, "resident")):
        with _previous(eng, value):
            got[name] = _sweep(eng, ops, **kw)
    for name, s in got.items():
        assert torch.equal(s, old), f"{name} instance, {S} rows, {known} candidates:\n{s}\n{old}"
    _check_range(old, crange, 20, "previous kernel")


def _layouts(B):
    """B [b][H][K][N] in layouts the 16-byte path must refuse, and one two-level-stride layout it takes."""
    b, H, K, N = B.shape
    out = {}
    out["transposed view"] = B.transpose(-2, -1).contiguous().transpose(-2, -1)                    # b_n = K
    wide = torch.zeros(b, H, K, N + 1, device=B.device)
    wide[..., :N] = B
    out["row stride 65"] = wide[..., :N]                                                              # b_n = 1, b_k = N + 1
    flat = torch.zeros(B.numel() + 1, device=B.device)
    flat[1:] = B.reshape(-1)
    out["base offset of one float"] = flat[1:].view(b, H, K, N)
    qkv = torch.randn(b, K, 3, H, N, device=B.device)                                                 # packed qkv: v = qkv[:, :, 2]
    qkv[:, :, 2] = B.permute(0, 2, 1, 3)
    out["slice of packed qkv"] = qkv[:, :, 2].permute(0, 2, 1, 3)                                   # strides (3 K H N, N, 3 H N, 1)
    qkv1 = torch.zeros(qkv.numel() + 1, device=B.device)
    qkv1[1:] = qkv.reshape(-1)
    out["slice of packed qkv, base offset of one float"] = qkv1[1:].view(b, K, 3, H, N)[:, :, 2].permute(0, 2, 1, 3)
    for name, v in out.items():
        assert torch.equal(v, B) and (name == "slice of packed qkv" or not (v.stride(-1) == 1 and v.stride(-2) % 4 == 0 and v.data_ptr() % 16 == 0))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("S,N", [(130, 64), (65, 40)])
def test_b_layouts_give_the_aligned_copys_table(eng, S, N):
    A, B, out, grad = _mk(S, S, N)
    ref = _search(eng, A, B, out, grad)
    ref1 = _sweep(eng, (A, B, out, grad), crange=(6, 7), known_cands=1)
    for name, Bv in _layouts(B).items():
        _same(_search(eng, A, Bv, out, grad), ref, f"B as {name}")
        got1 = _sweep(eng, (A, Bv, out, grad), crange=(6, 7), known_cands=1)
        assert torch.equal(got1, ref1), f"B as {name}, light instance:\n{got1}\n{ref1}"
        with _previous(eng):
            _same(_search(eng, A, Bv, out, grad), ref, f"B as {name}, previous kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("bit", [8, 6])
@pytest.mark.parametrize("metric", ["hessian", "L2_norm", "L1_norm"])
def test_pruned_split_search_end_to_end(eng, metric, bit):
    """matmul_calibrate(sos) at 2 x 3 x 197 under the cross-check against the full sweep (and pruning forced: synthetic
    operands of this size have loose slice bounds, which would keep the full sweep): split and intervals equal those of the
    previous kernel, and stages A, B1 and B2 ran k_sos_split."""
    A, B, out, grad = _mk(197, 197, 64)
    hp = dict(A_bit=bit, B_bit=bit, metric=metric, eq_alpha=0.01, eq_beta=1.2, eq_n=100, search_round=2, sos=True)
    args = dict(A=A, B=B, out=out, grad=grad)
    eng.debug_variant(CROSS_CHECK | FORCE_PRUNE)
    eng.stats_enable(True)
    try:
        eng.stats_reset()
        new = eng.matmul_calibrate(**args, **hp)
        torch.cuda.synchronize()
        recs = eng.stats_launches()
        with _previous(eng):
            old = eng.matmul_calibrate(**args, **hp)
            torch.cuda.synchronize()
    finally:
        eng.stats_enable(False)
        eng.debug_variant(0)
    for a, b, name in zip(new[:3], old[:3], ("A_interval", "B_interval", "split")):
        assert torch.equal(a, b), f"{metric} {bit} bit: {name} differs from the previous kernel's: {a} {b}"
    stages = {r["stage"] for r in recs if r["kernel"] == "k_sos_split"}
    assert {"A", "B1", "B2"} <= stages, f"stages that ran k_sos_split: {sorted(stages)}"


# ---- register / scratch budget of the instances, from the cross-compiled ISA (no GPU needed) -------------------------------
_TU = """#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <type_traits>
#include <utility>
#include "%s"
namespace p4v {
%s
}
"""


@pytest.fixture(scope="module")
def sos_resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    inst = [(ks, epi, var) for ks, epi in ((100, 0), (72, 2), (32, 3)) for var in (1, 2, 3)]
    body = "\n".join(f"template __global__ void k_sos_split<{ks}, {epi}, {var}>(SosSplitParams);" for ks, epi, var in inst)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++20", "-Wno-unused-value", "-mllvm", "-amdgpu-mfma-vgpr-form",
             "-fno-slp-vectorize", "--cuda-device-only", "-S"]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "sos.hip")
        with open(src, "w") as f:
            f.write(_TU % (os.path.join(ROOT, "ptq4vit_amd", "csrc", "p4v_kernels.h"), body))
        subprocess.run([hipcc] + flags + [src, "-o", os.path.join(d, "sos.s")], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        lines = open(os.path.join(d, "sos.s")).read().split("\n")
    res, name = {}, None
    for l in lines:
        m = re.match(r"^_ZN3p4v11k_sos_splitILi(\d+)ELi(\d+)ELi(\d+)EEEvNS_14SosSplitParamsE:", l)
        if m:
            name = tuple(int(v) for v in m.groups())
        elif re.match(r"^_Z\S*:", l):
            name = None
        m = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", l)
        if m and name:
            res.setdefault(name, {})[m.group(1)] = int(m.group(2))
    assert set(res) == set(inst), sorted(res)
    return res


def test_sos_instances_budget(sos_resources):
    """No scratch anywhere; the light instance (VAR 3) fits 256 registers, i.e. two workgroups per CU (2 x 51 KB of LDS fit as
    well), the others the 512 of a wave that is alone on its SIMD."""
    for (ks, epi, var), v in sos_resources.items():
        print(f"k_sos_split<{ks}, {epi}, {var}>: {v}")
        assert v["ScratchSize"] == 0, (ks, epi, var, v)
        if var == 3:
            assert v["NumVgprs"] + v["NumAgprs"] <= 256 and v["Occupancy"] >= 2, (ks, epi, var, v)
        else:
            assert v["NumVgprs"] + v["NumAgprs"] <= 512, (ks, epi, var, v)
