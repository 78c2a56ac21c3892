"""The C-ABI shared library loads on a CPU-only host and exports every symbol include/*.h declares.
No compute call is made here (no GPU): only planning (workspace sizing) and argument validation."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ptq4vit_amd import _lib
    return _lib.load()


def test_every_declared_symbol_is_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "ptq4vit_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ptq4vit_hip_debug.h")).read()
    assert "p4v_debug_" not in hdr.split("#ifndef PTQ4VIT_HIP_H")[1].replace("p4v_debug_*", ""), "debug entry points belong in ptq4vit_hip_debug.h"
    declared = set(re.findall(r"\b(p4v_[A-Za-z0-9_]+)\s*\(", hdr)) | set(re.findall(r"\b(p4v_[A-Za-z0-9_]+)\s*\(", dbg))
    assert {"p4v_linear_calibrate", "p4v_matmul_calibrate", "p4v_conv_calibrate", "p4v_version"} <= declared
    from ptq4vit_amd import _lib
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    for sym in declared:
        assert hasattr(lib, sym), f"{sym} is declared in the header but not exported by libptq4vit_hip.so"


def test_version(lib):
    hdr = open(os.path.join(ROOT, "include", "ptq4vit_hip.h")).read()
    assert lib.p4v_version() == int(re.search(r"#define P4V_VERSION (\d+)", hdr).group(1)) >= 130


def test_workspace_planning_matches_shapes(lib):
    from ptq4vit_amd import _lib
    d = _lib.LinearDesc(32, 197, 768, 2304, 3, 1, 1, 8, 8, 4, 100, 3, 0, 0, 1, 0)
    need = lib.p4v_linear_workspace_bytes(C.byref(d))
    # candidate-expanded int8 plane of the activation search dominates: 100 x 6400(pad) x 768
    assert 100 * 6304 * 768 < need < 4 * 100 * 6656 * 768
    m = _lib.MatMulDesc()
    m.batch, m.heads, m.M, m.K, m.N = 32, 12, 197, 64, 197
    m.A_bit = m.B_bit = 8
    m.metric, m.eq_n, m.search_round = 4, 100, 3
    assert lib.p4v_matmul_workspace_bytes(C.byref(m)) > 100 * 384 * 256 * 64
    c = _lib.ConvDesc(32, 3, 224, 224, 768, 16, 16, 16, 16, 0, 0, 1, 1, 8, 32, 4, 100, 3, 1, 0, 1, 0)
    assert lib.p4v_conv_workspace_bytes(C.byref(c)) > 100 * 768 * 768 * 4


def test_invalid_arguments_are_reported_not_crashed(lib):
    from ptq4vit_amd import _lib
    d = _lib.LinearDesc(32, 197, 768, 2304, 3, 1, 1, 8, 8, 4, 100, 3, 0, 0, 1, 0)
    null = C.c_void_p(0)
    rc = lib.p4v_linear_calibrate(C.byref(d), null, null, null, null, null, null, null, null, null, null, null, 0, null)
    assert rc == -1 and b"null pointer" in lib.p4v_last_error()
    bad = _lib.LinearDesc(32, 197, 768, 2304, 5, 1, 1, 8, 8, 4, 100, 3, 0, 0, 1, 0)   # 2304 % 5 != 0
    assert lib.p4v_linear_workspace_bytes(C.byref(bad)) == 0
    assert b"must divide" in lib.p4v_last_error()


def test_granular_entry_points_validate_arguments(lib):
    """the per-pass entry points exist and refuse bad arguments without touching a GPU."""
    from ptq4vit_amd import _lib
    null = C.c_void_p(0)
    d = _lib.LinearDesc(32, 197, 768, 2304, 3, 1, 1, 8, 8, 4, 100, 3, 0, 0, 1, 0)
    assert lib.p4v_amax_init_linear(C.byref(d), null, null, null, null, null, 0, null) == -1
    assert b"p4v_amax_init_linear" in lib.p4v_last_error()
    for fn in (lib.p4v_linear_search_w, lib.p4v_linear_search_a):
        assert fn(C.byref(d), *([null] * 10), null, 0, null) == -1
    m = _lib.MatMulDesc()
    m.batch, m.heads, m.M, m.K, m.N = 2, 3, 8, 4, 8
    m.A_bit = m.B_bit = 8
    m.metric, m.eq_n, m.search_round, m.sos = 4, 20, 1, 1
    one = C.c_void_p(64)   # never dereferenced: the sos / non-sos mismatch is refused first
    assert lib.p4v_matmul_search_A(C.byref(m), *([one] * 9), one, 64, null) == -1
    assert b"p4v_sos_search_split" in lib.p4v_last_error()
    m.sos = 0
    assert lib.p4v_sos_search_split(C.byref(m), *([one] * 8), one, 64, null) == -1
    assert b"not a split-of-softmax" in lib.p4v_last_error()
    c = _lib.ConvDesc(2, 3, 32, 32, 8, 16, 16, 16, 16, 0, 0, 1, 1, 8, 32, 4, 100, 3, 1, 0, 1, 0)
    assert lib.p4v_conv_search_w_layerwise(C.byref(c), *([one] * 10), one, 64, null) == -1
    assert b"channelwise does not match" in lib.p4v_last_error()
    assert lib.p4v_conv_search_a(C.byref(c), *([one] * 10), one, 64, null) == -1
    assert b"a_bit >= 32" in lib.p4v_last_error()
    assert lib.p4v_score_argmax_gather(null, 0, 0, null, null, null, null) == -1
    # the plane / export entry points of version 1.3 (rows a9, f-3)
    pd = _lib.PlaneDesc(16, 16, 64, 1, 7, -128, 127, 128, 0.0, 0)                       # unknown mode
    assert lib.p4v_pack_plane_i8(C.byref(pd), one, one, one, null) == -1 and b"unknown mode" in lib.p4v_last_error()
    pd = _lib.PlaneDesc(16, 16, 64, 1, _lib.PLANE_SOS_HI, 0, 127, 128, 0.0, 0)
    assert lib.p4v_pack_plane_i8(C.byref(pd), one, null, one, null) == -1 and b"split" in lib.p4v_last_error()
    ed = _lib.ExportDesc()
    ed.mode = 9
    assert lib.p4v_export_quantize(C.byref(ed), one, one, null, one, null) == -1 and b"unknown mode" in lib.p4v_last_error()
    assert lib.p4v_debug_set_variant(-1, 0) == -1 and lib.p4v_debug_set_tuning(99, 0) == -1
    # switches of removed paths (variant bit 8, key 12 = 8) fail instead of timing production under a stale label
    assert lib.p4v_debug_set_variant(8, 0) == -1 and b"removed" in lib.p4v_last_error()
    assert lib.p4v_debug_set_tuning(12, 8) == -1 and b"removed" in lib.p4v_last_error()
    assert lib.p4v_debug_set_variant(0, 0) == 0 and lib.p4v_stats_enable(0) == 0


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from ptq4vit_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load()


# ---- the workspace contract (include/ptq4vit_hip.h, Conventions): what can be checked without a GPU ---------------------------
def _linear_desc(images, tokens, K, N, *, n_V=1, n_H=1, n_a=1, bits=8, metric="hessian", rounds=1, postgelu=False, reserved=0):
    from ptq4vit_amd import _lib
    return _lib.LinearDesc(images, tokens, K, N, n_V, n_H, n_a, bits, bits, _lib.METRICS[metric], 100, rounds, int(postgelu), 0, 1, reserved)


def _matmul_desc(M, K, N, *, sos=False, metric="hessian", rounds=1, reserved=0, batch=2, heads=2, blocks=None):
    import torch
    from ptq4vit_amd import _lib
    bd = _lib.MatMulBlocksDesc() if blocks else None
    d = bd.mm if blocks else _lib.MatMulDesc()
    A = torch.empty(batch, heads, M, K)
    B = torch.empty(batch, heads, K, N) if sos else torch.empty(batch, heads, N, K).transpose(-2, -1)    # q.k^T: k transposed in memory
    d.batch, d.heads, d.M, d.K, d.N = batch, heads, M, K, N
    for i in range(4):
        d.a_stride[i], d.b_stride[i] = A.stride(i), B.stride(i)
    d.A_bit = d.B_bit = 8
    d.metric, d.eq_n, d.search_round, d.sos, d.init_layerwise, d.reserved = _lib.METRICS[metric], 100, rounds, int(sos), 0, reserved
    if blocks:
        bd.n_V_A, bd.n_H_A, bd.n_V_B, bd.n_H_B = blocks
    return bd if blocks else d


def _conv_desc(*, a_bit=32, metric="hessian", rounds=1, channelwise=True, reserved=0, geometry=(2, 3, 32, 32, 16, 16, 16, 16, 16, 0, 0, 1, 1)):
    """`geometry`: batch, channels, height, width, out channels, kernel h / w, stride h / w, padding h / w, dilation h / w."""
    from ptq4vit_amd import _lib
    return _lib.ConvDesc(*geometry, 8, a_bit, _lib.METRICS[metric], 100, rounds, int(channelwise), 0, 1, reserved)


def _contract_descs():
    """(query, descriptor) of every case of tests/sweep_plan_cases.py::CASES (one round; reserved bit 3 where the case runs unpruned)
    and of tests/search_round_cases.py::CASES (three rounds; the default call and the one with reserved bit 1)."""
    L, M, B, Cv = ("p4v_linear_workspace_bytes", "p4v_matmul_workspace_bytes", "p4v_matmul_blocks_workspace_bytes", "p4v_conv_workspace_bytes")
    out = [(L, _linear_desc(2, 64, 192, 128, reserved=8)), (L, _linear_desc(2, 64, 128, 128, reserved=8)),
           (L, _linear_desc(2, 64, 1024, 64, reserved=8)), (L, _linear_desc(2, 64, 1024, 64, postgelu=True, reserved=8)),
           (L, _linear_desc(2, 64, 1088, 64, reserved=8)), (L, _linear_desc(2, 64, 192, 120, n_V=3, reserved=8)),
           (M, _matmul_desc(49, 64, 49, reserved=8)), (M, _matmul_desc(120, 64, 120, reserved=8)),
           (M, _matmul_desc(49, 49, 64, sos=True, reserved=8)), (Cv, _conv_desc(reserved=8)), (L, _linear_desc(10, 65, 192, 96)),
           (B, _matmul_desc(13, 8, 13, batch=4, heads=3, rounds=2, blocks=(2, 2, 2, 3)))]
    for res in (0, 2):
        kw = dict(rounds=3, reserved=res)
        out += [(L, _linear_desc(2, 64, 192, 128, **kw)), (L, _linear_desc(2, 64, 192, 128, postgelu=True, **kw)),
                (L, _linear_desc(2, 64, 1024, 64, postgelu=True, **kw)), (L, _linear_desc(2, 64, 192, 128, n_H=2, n_a=2, **kw)),
                (L, _linear_desc(10, 65, 192, 96, **kw)), (L, _linear_desc(2, 64, 192, 128, metric="cosine", **kw)),
                (L, _linear_desc(2, 64, 1024, 64, metric="cosine", **kw)), (L, _linear_desc(2, 64, 192, 120, n_V=3, metric="cosine", **kw)),
                (L, _linear_desc(3, 11, 24, 16, n_V=2, n_H=2, n_a=3, bits=4, metric="cosine", **kw)),
                (M, _matmul_desc(49, 64, 49, **kw)), (M, _matmul_desc(49, 64, 49, metric="cosine", **kw)),
                (M, _matmul_desc(49, 49, 64, sos=True, **kw)), (M, _matmul_desc(49, 49, 64, sos=True, metric="cosine", **kw)),
                (Cv, _conv_desc(**kw)), (Cv, _conv_desc(a_bit=8, **kw)), (Cv, _conv_desc(metric="cosine", channelwise=False, **kw)),
                (B, _matmul_desc(13, 8, 13, batch=4, heads=3, blocks=(2, 2, 2, 3), **kw)),
                (B, _matmul_desc(13, 13, 8, batch=4, heads=3, sos=True, blocks=(1, 1, 2, 2), **kw)),
                (B, _matmul_desc(5, 8, 5, blocks=(4, 1, 1, 4), **kw)),
                (Cv, _conv_desc(a_bit=8, geometry=(3, 5, 17, 23, 10, 3, 5, 2, 1, 1, 2, 2, 1), **kw))]
    # (the lists themselves build their tensors on the GPU and expose no parameters: hold the count of this table to theirs, so that a
    # case added or removed there cannot pass here unnoticed)
    from tests import search_round_cases, sweep_plan_cases
    assert len(out) == len(sweep_plan_cases.CASES) + 2 * len(search_round_cases.CASES), "update _contract_descs() with the case lists"
    loose = {i for i, (q, d) in enumerate(out) if q == L and (d.batch, d.tokens) == (10, 65)}      # the bound cases run under LOOSE
    assert len(loose) == 3
    return [(q, d, sweep_plan_cases.LOOSE if i in loose else 0) for i, (q, d) in enumerate(out)]


def test_arena_gap_only_grows_the_sizing_and_resets(lib):
    """p4v_debug_set_arena_gap: the sizing run includes the gaps (>= the value without), both values are repeatable and do not depend
    on the order of the queries, only multiples of the arena's 256-byte alignment are taken, and 0 restores the plain sizes."""
    descs = _contract_descs()
    def size(q, d, variant):
        assert lib.p4v_debug_set_variant(variant, 0) == 0
        try:
            return getattr(lib, q)(C.byref(d))
        finally:
            assert lib.p4v_debug_set_variant(0, 0) == 0
    try:
        plain = [size(*c) for c in descs]
        assert all(n > 4096 for n in plain), plain
        assert lib.p4v_debug_set_arena_gap(100) == -1 and b"256" in lib.p4v_last_error()
        assert [size(*c) for c in descs] == plain                      # (a refused value changes nothing)
        assert lib.p4v_debug_set_arena_gap(4096) == 0
        gapped = [size(*c) for c in descs]
        assert all(g >= p + 4096 for g, p in zip(gapped, plain)), list(zip(gapped, plain))
        assert [size(*c) for c in reversed(descs)] == gapped[::-1]     # repeatable, whatever the order of the queries
        assert lib.p4v_debug_set_arena_gap(8192) == 0
        assert all(g2 >= g for g2, g in zip([size(*c) for c in descs], gapped))
    finally:
        assert lib.p4v_debug_set_arena_gap(0) == 0
    assert [size(*c) for c in reversed(descs)] == plain[::-1]
    assert [size(*c) for c in descs] == plain
    assert lib.p4v_debug_arena_ranges(None, 0) >= 0                          # host-side record: callable without a GPU


def test_misaligned_workspace_pointer_is_refused_on_the_host(lib):
    """Every entry point that takes a workspace refuses a d_workspace below the documented 16-byte alignment with P4V_ERR_INVALID
    before anything is launched (no GPU here: a call that got past the check would fail differently or crash).  The pointers are
    fakes that are never dereferenced; 72 is 8-byte aligned only."""
    from ptq4vit_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ptq4vit_hip.h")).read()
    assert "aligned to at least 16 bytes" in hdr
    one, bad, null = C.c_void_p(64), C.c_void_p(72), C.c_void_p(0)
    ld, cd = _linear_desc(2, 64, 192, 128), _conv_desc(a_bit=8)
    cl = _conv_desc(a_bit=8, channelwise=False)
    md, sd = _matmul_desc(49, 64, 49), _matmul_desc(49, 49, 64, sos=True)
    bd = _matmul_desc(13, 8, 13, batch=4, heads=3, blocks=(2, 2, 2, 3))
    r = C.byref
    calls = [
        ("p4v_linear_calibrate", (r(ld), *[one] * 10)), ("p4v_matmul_calibrate", (r(md), *[one] * 10)),
        ("p4v_matmul_blocks_calibrate", (r(bd), *[one] * 10)), ("p4v_conv_calibrate", (r(cd), *[one] * 10)),
        ("p4v_linear_quant_forward", (r(ld), *[one] * 6)), ("p4v_matmul_quant_forward", (r(md), *[one] * 6)),
        ("p4v_matmul_blocks_quant_forward", (r(bd), *[one] * 6)),
        ("p4v_amax_init_linear", (r(ld), *[one] * 4)), ("p4v_linear_search_w", (r(ld), *[one] * 10)),
        ("p4v_linear_search_a", (r(ld), *[one] * 10)),
        ("p4v_amax_init_matmul", (r(md), *[one] * 4)), ("p4v_matmul_search_A", (r(md), *[one] * 9)),
        ("p4v_sos_search_split", (r(sd), *[one] * 8)), ("p4v_matmul_search_B", (r(md), *[one] * 10)),
        ("p4v_amax_init_matmul_blocks", (r(bd), *[one] * 4)), ("p4v_matmul_blocks_search", (r(bd), 1, 0, 0, *[one] * 10)),
        ("p4v_amax_init_conv", (r(cd), *[one] * 4)), ("p4v_conv_search_w_channelwise", (r(cd), *[one] * 10)),
        ("p4v_conv_search_w_layerwise", (r(cl), *[one] * 10)), ("p4v_conv_search_a", (r(cd), *[one] * 10)),
    ]
    with_ws = {s for s in _lib.EXPORTS if s not in ("p4v_calibrate_group", "p4v_debug_sos_sweep") and
               re.search(r"\b%s\s*\([^;]*d_workspace" % s, hdr)}
    assert with_ws == {name for name, _ in calls}, with_ws ^ {name for name, _ in calls}
    for name, args in calls:
        rc = getattr(lib, name)(*args, bad, 1 << 20, null)
        assert rc == -1 and b"aligned" in lib.p4v_last_error(), (name, rc, lib.p4v_last_error())
    rc = lib.p4v_debug_sos_sweep(r(sd), one, one, one, one, 20, -1, -1, -1, one, bad, 1 << 20, null)
    assert rc == -1 and b"aligned" in lib.p4v_last_error(), lib.p4v_last_error()
    jobs = (_lib.GroupJob * 1)()
    jobs[0].kind, jobs[0].desc, jobs[0].workspace, jobs[0].workspace_bytes = _lib.JOB_LINEAR, C.cast(C.pointer(ld), C.c_void_p), 72, 1 << 20
    assert lib.p4v_calibrate_group(jobs, 1, null, null) == -1 and b"aligned" in lib.p4v_last_error()


# ---- required pointers (include/ptq4vit_hip.h): every workspace-taking entry point refuses a missing one on the host -----------------
# (entry point, descriptor, integer arguments behind the descriptor, the pointer arguments in the header's order; "?name": optional)
def _required_pointer_table():
    from ptq4vit_amd import _lib
    ld, cd, cl = _linear_desc(2, 64, 192, 128), _conv_desc(a_bit=8), _conv_desc(channelwise=False)
    md, sd = _matmul_desc(49, 64, 49), _matmul_desc(49, 49, 64, sos=True)
    bd = _matmul_desc(13, 8, 13, batch=4, heads=3, blocks=(2, 2, 2, 3))
    bsd = _matmul_desc(13, 13, 8, batch=4, heads=3, sos=True, blocks=(1, 1, 2, 2))
    mlp = _lib.MlpDesc()
    mlp.fc1, mlp.fc2 = _linear_desc(2, 64, 64, 256), _linear_desc(2, 64, 256, 64, postgelu=True)
    attn = _lib.AttnDesc()
    attn.qk, attn.pv, attn.scale = _matmul_desc(49, 64, 49), _matmul_desc(49, 49, 64, sos=True), 0.125
    lin_search = "weight bias x out grad cands w_interval a_interval ?scores ?best"
    mm_cal = "A B out grad mult A_interval B_interval split ?scores ?best"
    return [
        ("p4v_linear_calibrate", ld, (), "weight bias x out grad mult w_interval a_interval ?scores ?best"),
        ("p4v_matmul_calibrate", sd, (), mm_cal), ("p4v_matmul_blocks_calibrate", bsd, (), mm_cal),
        ("p4v_conv_calibrate", cd, (), "weight bias x out grad mult w_interval a_interval ?scores ?best"),
        ("p4v_linear_quant_forward", ld, (), "weight bias x w_interval a_interval out"),
        ("p4v_matmul_quant_forward", sd, (), "A B A_interval B_interval split out"),
        ("p4v_matmul_blocks_quant_forward", bsd, (), "A B A_interval B_interval split out"),
        ("p4v_mlp_quant_forward", mlp, (), "w1 bias1 w2 bias2 x w1_interval a1_interval w2_interval a2_interval out ?hidden"),
        ("p4v_attn_quant_forward", attn, (), "q kT v qk_A_interval qk_B_interval pv_A_interval pv_B_interval split out ?probs"),
        ("p4v_amax_init_linear", ld, (), "weight x w_interval a_interval"),
        ("p4v_linear_search_w", ld, (), lin_search), ("p4v_linear_search_a", ld, (), lin_search),
        ("p4v_amax_init_matmul", md, (), "A B A_interval B_interval"),
        ("p4v_matmul_search_A", md, (), "A B out grad cands A_interval B_interval ?scores ?best"),
        ("p4v_sos_search_split", sd, (), "A B out grad split A_interval ?scores ?best"),
        ("p4v_matmul_search_B", sd, (), "A B out grad cands A_interval split B_interval ?scores ?best"),
        ("p4v_amax_init_matmul_blocks", bd, (), "A B A_interval B_interval"),
        ("p4v_matmul_blocks_search", bsd, (1, 0, 0), "A B out grad cands A_interval B_interval split ?scores ?best"),
        ("p4v_amax_init_conv", cd, (), "weight x w_interval a_interval"),
        ("p4v_conv_search_w_channelwise", cd, (), lin_search), ("p4v_conv_search_w_layerwise", cl, (), lin_search),
        ("p4v_conv_search_a", cd, (), lin_search),
    ]


def _missing_says(name, missing):
    """The message of `name` with `missing` NULL, word for word.  Every descriptor of the table has a bias, the hessian metric and --
    where the header asks for d_split -- the split-of-softmax class.  The three head-wise *_calibrate entry points and the checks
    inside the engine name the module, every other check the entry point."""
    module = "conv" if "conv" in name else "matmul" if ("matmul" in name or "sos" in name) else "linear"
    who = module if name in ("p4v_linear_calibrate", "p4v_matmul_calibrate", "p4v_conv_calibrate") else name
    if missing in ("bias", "bias1", "bias2"):
        return who + (": has_bias set but the bias is null" if "mlp" in name else ": has_bias set but d_bias is null" if "forward" in name else
                      ": has_bias set but d_bias is NULL")
    if missing == "grad":
        return module + ": hessian metric needs raw_grad" + (" (linear.py:418)" if module == "linear" else "")
    if missing == "split" and name != "p4v_sos_search_split":
        return ("matmul" if name.endswith("_calibrate") else name) + ": sos needs d_split"
    return who + ": null pointer"


def test_every_required_pointer_is_checked_before_any_launch(lib):
    """One at a time, every pointer include/ptq4vit_hip.h documents as required is NULL: P4V_ERR_INVALID, with the entry point's own
    message, before anything is launched (no GPU here).  The other pointers are fakes that are never dereferenced."""
    from ptq4vit_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ptq4vit_hip.h")).read()
    one, null = C.c_void_p(64), C.c_void_p(0)
    table = _required_pointer_table()
    with_ws = {s for s in _lib.EXPORTS if s != "p4v_calibrate_group" and not s.endswith("_workspace_bytes") and
               re.search(r"\b%s\s*\([^;]*\bd_(workspace|ws)\b" % s, hdr)}
    assert with_ws == {name for name, *_ in table}, with_ws ^ {name for name, *_ in table}
    for name, desc, ints, names in table:
        fn, names = getattr(lib, name), names.split()
        # (the header's parameter list has as many pointers as the table's row)
        proto = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr).group(1)
        assert proto.count("*") == 1 + len(names) + 2, (name, proto)       # desc, the tensors, workspace, stream
        def call(missing):
            args = [null if n.lstrip("?") == missing else one for n in names]
            return fn(None if missing == "desc" else C.byref(desc), *ints, *args, null if missing == "workspace" else one, 1 << 30, null)
        for missing in ["desc", "workspace"] + [n for n in names if not n.startswith("?")]:
            rc, msg = call(missing), lib.p4v_last_error().decode()
            assert rc == -1 and msg == _missing_says(name, missing), (name, missing, rc, msg)
    # the fused MLP forward takes its workspace as d_ws: below the 16-byte alignment it is refused like every d_workspace
    name, desc, ints, names = next(r for r in table if r[0] == "p4v_mlp_quant_forward")
    assert lib.p4v_mlp_quant_forward(C.byref(desc), *[one] * len(names.split()), C.c_void_p(72), 1 << 30, null) == -1
    assert b"aligned" in lib.p4v_last_error(), lib.p4v_last_error()


def test_sizing_refuses_null_and_unsupported_descriptors(lib):
    """*_workspace_bytes(NULL) and an unsupported descriptor return 0 (the latter with its message), forward-only sizing included."""
    from ptq4vit_amd import _lib
    for q in ("p4v_linear_workspace_bytes", "p4v_matmul_workspace_bytes", "p4v_matmul_blocks_workspace_bytes", "p4v_conv_workspace_bytes",
              "p4v_mlp_workspace_bytes", "p4v_attn_workspace_bytes"):
        assert getattr(lib, q)(None) == 0, q
    for reserved in (0, 4):
        bad = _linear_desc(2, 64, 192, 128, n_V=5, reserved=reserved)               # 128 % 5 != 0
        assert lib.p4v_linear_workspace_bytes(C.byref(bad)) == 0 and b"must divide" in lib.p4v_last_error()
        bad = _matmul_desc(49, 64, 49, reserved=reserved)
        bad.A_bit = 9
        assert lib.p4v_matmul_workspace_bytes(C.byref(bad)) == 0 and b"bit widths" in lib.p4v_last_error()
        bad = _matmul_desc(13, 8, 13, batch=4, heads=3, reserved=reserved, blocks=(2, 9, 2, 3))
        assert lib.p4v_matmul_blocks_workspace_bytes(C.byref(bad)) == 0 and b"up to n_V, n_H = 8" in lib.p4v_last_error()
        bad = _matmul_desc(13, 8, 13, batch=4, heads=3, reserved=reserved, blocks=(2, 0, 2, 3))
        assert lib.p4v_matmul_blocks_workspace_bytes(C.byref(bad)) == 0 and b"non-positive block count" in lib.p4v_last_error()
    bad = _conv_desc(a_bit=8, metric="cosine")
    assert lib.p4v_conv_workspace_bytes(C.byref(bad)) == 0 and b"cosine does not support the activation search" in lib.p4v_last_error()
    mlp = _lib.MlpDesc()
    mlp.fc1, mlp.fc2 = _linear_desc(2, 64, 64, 256, postgelu=True), _linear_desc(2, 64, 256, 64)
    assert lib.p4v_mlp_workspace_bytes(C.byref(mlp)) == 0 and b"twin_postgelu belongs on fc2" in lib.p4v_last_error()
    mlp.fc1, mlp.fc2 = _linear_desc(2, 64, 64, 256), _linear_desc(2, 64, 128, 64)
    assert lib.p4v_mlp_workspace_bytes(C.byref(mlp)) == 0 and b"is not fc2's input" in lib.p4v_last_error()
    # the sizes a supported descriptor gets: the forward alone needs no more than the search, and something
    ld, md = _linear_desc(2, 64, 192, 128), _matmul_desc(49, 64, 49)
    full = lib.p4v_linear_workspace_bytes(C.byref(ld))
    ld.reserved = 4
    assert 4096 < lib.p4v_linear_workspace_bytes(C.byref(ld)) <= full
    full = lib.p4v_matmul_workspace_bytes(C.byref(md))
    md.reserved = 4
    assert 4096 < lib.p4v_matmul_workspace_bytes(C.byref(md)) <= full


def test_prune_decide_refuses_bad_arguments_before_any_launch(lib):
    """p4v_debug_prune_decide: every null pointer, C < 1, nj < 1, nj > 4096 and the synthetic candidate on one score block are
    refused on the host (the pointers are never dereferenced: no GPU here); p4v_debug_prune_tables starts and stops without one."""
    null, one = C.c_void_p(0), C.c_void_p(64)
    info = (C.c_int32 * 3)()

    def call(C_=32, nj=2, virt=0, **nulls):
        a = dict(SA=one, SA2=one, T=one, cands=one, ranges=one, rblk=one, best=one, interval=one, best_out=one, info=info)
        a.update({k: (None if k == "info" else null) for k in nulls})
        return lib.p4v_debug_prune_decide(a["SA"], a["SA2"], a["T"], a["cands"], C_, nj, virt, 0, 0, a["ranges"], a["rblk"], a["best"],
                                          a["interval"], a["best_out"], a["info"], null)
    for name in ("SA", "T", "cands", "ranges", "rblk", "best", "interval", "best_out", "info"):      # (SA2 is optional)
        assert call(**{name: True}) == -1 and b"p4v_debug_prune_decide: null pointer" in lib.p4v_last_error(), name
    for kw in (dict(C_=0), dict(C_=-3), dict(nj=0), dict(nj=4097), dict(nj=1, virt=1)):
        assert call(**kw) == -1 and b"p4v_debug_prune_decide: 1 <= C" in lib.p4v_last_error(), kw
    n = C.c_int64(-1)
    assert lib.p4v_debug_prune_tables(None, 0, None) == 0 and lib.p4v_debug_prune_tables(None, 0, C.byref(n)) == 0 and n.value == 0
