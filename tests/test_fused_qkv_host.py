"""No GPU: the host side of the fused qkv + attention forward -- p4v_qkv_attn_workspace_bytes / p4v_qkv_attn_quant_forward's
argument checks and envelope (nothing is launched: every pointer is a fake that is never dereferenced), the sizing, and the
bookkeeping of utils/fuse.py::fuse_qkv_attention on a CPU mini ViT: which containers it patches, that it shares fuse_attention's
saved forward (the later call decides, unfuse_attention undoes either) and that a CPU net keeps its original forward.

The entry point takes its tensors, its workspace and the workspace's size in a record (p4v_qkv_attn_tensors), so -- as for
p4v_wattn_quant_forward -- the rule of tests/test_cabi.py's table is applied to it here: every required pointer NULL, one at a
time, is P4V_ERR_INVALID with the entry point's own message before any launch.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = "x w w_interval a_interval qk_A_interval qk_B_interval pv_A_interval pv_B_interval out ws".split()
OPTIONAL = "bias split qkv_out probs".split()     # (bias: required with has_bias, split: with sos -- messages of their own)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ptq4vit_amd import _lib
    return _lib.load()


def _desc(B=2, N=50, H=3, D=64, K=192, sos=True, bits=8, n_V=3, has_bias=1):
    from ptq4vit_amd import _lib
    d = _lib.QkvAttnDesc()
    d.qkv = _lib.LinearDesc(B, N, K, 3 * H * D, n_V, 1, 1, bits, bits, _lib.METRICS["L2_norm"], 1, 1, 0, 0, has_bias, _lib.RESERVED_FORWARD_ONLY)
    for mm, (M_, K_, N_) in ((d.qk, (N, D, N)), (d.pv, (N, N, D))):
        mm.batch, mm.heads, mm.M, mm.K, mm.N = B, H, M_, K_, N_
        mm.A_bit = mm.B_bit = bits
        mm.metric, mm.eq_n, mm.search_round, mm.reserved = _lib.METRICS["L2_norm"], 1, 1, _lib.RESERVED_FORWARD_ONLY
    d.pv.sos = int(sos)
    d.scale = D ** -0.5
    return d


def _tensors(d, missing=(), ws=64, nbytes=1 << 30):
    from ptq4vit_amd import _lib
    t = _lib.QkvAttnTensors()
    for n in _lib.QkvAttnTensors.POINTERS:
        setattr(t, n, 0 if n in missing else 64)
    t.ws, t.ws_bytes = (0 if "ws" in missing else ws), nbytes
    return t


def test_header_prototype_and_version(lib):
    from ptq4vit_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ptq4vit_hip.h")).read()
    proto = re.search(r"\bp4v_qkv_attn_quant_forward\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert proto.count("*") == 3 and "p4v_qkv_attn_desc" in proto and "p4v_qkv_attn_tensors" in proto      # desc, the record, stream
    assert re.search(r"size_t\s+p4v_qkv_attn_workspace_bytes\s*\(\s*const\s+p4v_qkv_attn_desc\s*\*", hdr)
    body = re.search(r"typedef struct p4v_qkv_attn_tensors \{(.*?)\} p4v_qkv_attn_tensors;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = re.findall(r"\*?\s*([A-Za-z_][A-Za-z0-9_]*)\s*[,;]", body)
    assert tuple(members) == _lib.QkvAttnTensors.POINTERS + ("ws_bytes",), members
    assert set(REQUIRED + OPTIONAL) == set(_lib.QkvAttnTensors.POINTERS)
    assert C.sizeof(_lib.QkvAttnDesc) == C.sizeof(_lib.LinearDesc) + 2 * C.sizeof(_lib.MatMulDesc) + 8
    assert lib.p4v_version() >= 145
    assert {"p4v_qkv_attn_workspace_bytes", "p4v_qkv_attn_quant_forward", "p4v_debug_qkv_planes"} <= set(_lib.EXPORTS)
    assert _lib.LAUNCH_KINDS[18] == "k_qkv_heads"
    info = (C.c_uint64 * 9)()
    assert lib.p4v_debug_qkv_planes(None) == -1
    assert lib.p4v_debug_qkv_planes(info) == -1 and b"no p4v_qkv_attn_quant_forward call" in lib.p4v_last_error()


def test_sizing_holds_the_three_planes_on_top_of_the_attention_calls(lib):
    """The workspace: the attention chain's, the three int8 planes outside everything that is handed back, and the scratch of the
    qkv GEMM (Q(x), Q(W), the scale table) or of the attention chain, whichever is larger -- so never below attention's + the planes
    - the two operand planes attention's own produce() would have packed, never above attention's + planes + the qkv scratch."""
    from ptq4vit_amd import _lib
    up = lambda v, m: (v + m - 1) // m * m
    for kw in (dict(), dict(sos=False), dict(B=3, N=197), dict(B=1, N=5, H=1, K=64), dict(D=40, K=120), dict(B=1, N=1025, H=1, K=64)):
        d = _desc(**kw)
        a = _lib.AttnDesc()
        C.memmove(C.byref(a.qk), C.byref(d.qk), C.sizeof(_lib.MatMulDesc))
        C.memmove(C.byref(a.pv), C.byref(d.pv), C.sizeof(_lib.MatMulDesc))
        a.scale = d.scale
        attn, need = lib.p4v_attn_workspace_bytes(C.byref(a)), lib.p4v_qkv_attn_workspace_bytes(C.byref(d))
        assert attn > 0 and need > 0, lib.p4v_last_error()
        B, N, H, D, K = d.qkv.batch, d.qkv.tokens, d.qk.heads, d.qk.K, d.qkv.in_features
        Z, K1p = B * H, up(D, 64)
        planes = Z * K1p * (up(N, 128) + up(N, 128)) + Z * D * up(N, 64)     # (v: at least its valid rows)
        gemm = up(B * N, 128) * up(K, 64) + up(3 * H * D, 128) * up(K, 64)
        assert need >= planes and need <= attn + 2 * planes + gemm + (1 << 16), (kw, need, attn, planes, gemm)
    assert lib.p4v_qkv_attn_workspace_bytes(None) == 0


def test_envelope_refusals_launch_nothing(lib):
    from ptq4vit_amd import engine
    before = engine.launch_counters()

    def refused(d, code, msg):
        assert lib.p4v_qkv_attn_workspace_bytes(C.byref(d)) == 0 and msg in lib.p4v_last_error(), lib.p4v_last_error()
        assert lib.p4v_qkv_attn_quant_forward(C.byref(d), C.byref(_tensors(d)), None) == code and msg in lib.p4v_last_error(), lib.p4v_last_error()

    # the qkv layer
    d = _desc(); d.qkv.n_H = 2
    refused(d, -2, b"n_H = n_a = 1 on qkv")
    d = _desc(); d.qkv.n_a = 2
    refused(d, -2, b"n_H = n_a = 1 on qkv")
    d = _desc(); d.qkv.twin_postgelu = 1
    refused(d, -2, b"twin_postgelu")
    d = _desc(); d.qkv.reserved |= 1
    refused(d, -2, b"int8 planes only")
    d = _desc(); d.qkv.n_V = 7
    refused(d, -2, b"must divide the layer")
    for field in ("w_bit", "a_bit"):
        for bad in (1, 9):
            d = _desc(); setattr(d.qkv, field, bad)
            refused(d, -2, b"bit widths 2..8")
    # its seam with the chain
    d = _desc(); d.qkv.out_features += 3
    refused(d, -1, b"not 3 x 3 heads x head_dim 64")
    d = _desc(); d.pv.N = 32
    refused(d, -1, b"not 3 x 3 heads x head_dim 64")
    d = _desc(); d.qkv.tokens = 49
    refused(d, -1, b"qkv's rows 98 are not 2 images of 50")
    d = _desc(); d.qk.N = d.pv.K = 48
    refused(d, -1, b"tokens")
    d = _desc(); d.qk.heads = 0
    refused(d, -1, b"non-positive dimension")
    # the attention chain's own
    d = _desc(); d.qk.sos = 1
    refused(d, -2, b"no split-of-softmax operand")
    d = _desc(); d.pv.heads = 2
    refused(d, -1, b"is not the row operand")
    d = _desc(); d.scale = float("nan")
    refused(d, -1, b"scale is NaN")
    for side, field in (("qk", "A_bit"), ("qk", "B_bit"), ("pv", "A_bit"), ("pv", "B_bit")):
        for bad in (1, 9):
            d = _desc(); setattr(getattr(d, side), field, bad)
            refused(d, -2, b"bit widths 2..8")
    d = _desc(); d.pv.reserved |= 1
    refused(d, -2, b"int8 planes only")
    # inside: any n_V that divides, any in_features, mixed widths, no bias
    for kw in (dict(n_V=1), dict(n_V=9), dict(K=48), dict(K=1000), dict(has_bias=0), dict(bits=2), dict(D=40, K=120)):
        assert lib.p4v_qkv_attn_workspace_bytes(C.byref(_desc(**kw))) > 0, (kw, lib.p4v_last_error())
    d = _desc(); d.qkv.w_bit, d.qk.B_bit, d.pv.A_bit = 4, 4, 4
    assert lib.p4v_qkv_attn_workspace_bytes(C.byref(d)) > 0
    assert engine.launch_counters() == before


def test_every_required_pointer_is_checked_before_any_launch(lib):
    from ptq4vit_amd import engine
    before = engine.launch_counters()
    d = _desc()
    says = "p4v_qkv_attn_quant_forward: null pointer"
    assert lib.p4v_qkv_attn_quant_forward(None, C.byref(_tensors(d)), None) == -1 and lib.p4v_last_error().decode() == says
    assert lib.p4v_qkv_attn_quant_forward(C.byref(d), None, None) == -1 and lib.p4v_last_error().decode() == says
    for missing in REQUIRED:
        rc = lib.p4v_qkv_attn_quant_forward(C.byref(d), C.byref(_tensors(d, missing=(missing,))), None)
        assert rc == -1 and lib.p4v_last_error().decode() == says, (missing, rc, lib.p4v_last_error())
    rc = lib.p4v_qkv_attn_quant_forward(C.byref(d), C.byref(_tensors(d, missing=("split",))), None)
    assert rc == -1 and lib.p4v_last_error().decode() == "p4v_qkv_attn_quant_forward: sos needs split"
    rc = lib.p4v_qkv_attn_quant_forward(C.byref(d), C.byref(_tensors(d, missing=("bias",))), None)
    assert rc == -1 and lib.p4v_last_error().decode() == "p4v_qkv_attn_quant_forward: has_bias set but the bias is null"
    # the optional members: no complaint about them -- the call gets as far as the declared size (one byte: too small)
    plain, nobias = _desc(sos=False), _desc(has_bias=0)
    for dd, missing in ((d, ("probs",)), (d, ("qkv_out",)), (d, ("probs", "qkv_out")), (plain, ("split",)), (nobias, ("bias",))):
        rc = lib.p4v_qkv_attn_quant_forward(C.byref(dd), C.byref(_tensors(dd, missing=missing, nbytes=1)), None)
        assert rc == -3 and b"workspace too small" in lib.p4v_last_error(), (missing, rc, lib.p4v_last_error())
    # alignment, and one byte too few
    assert lib.p4v_qkv_attn_quant_forward(C.byref(d), C.byref(_tensors(d, ws=72)), None) == -1 and b"aligned" in lib.p4v_last_error()
    need = lib.p4v_qkv_attn_workspace_bytes(C.byref(d))
    assert lib.p4v_qkv_attn_quant_forward(C.byref(d), C.byref(_tensors(d, nbytes=need - 1)), None) == -3
    assert b"workspace too small: need >= %d bytes" % need in lib.p4v_last_error()
    assert engine.launch_counters() == before


# ---- utils/fuse.py on a CPU mini ViT -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_vit():
    from ptq4vit_amd.configs import PTQ4ViT
    from ptq4vit_amd.utils import models, net_wrap
    g = np.load(os.path.join(ROOT, "tests", "golden", "minivit_ptq4vit.npz"), allow_pickle=False)
    kw = json.loads(str(g["model_kwargs"]))
    net = models.get_net("vit_tiny_patch16_224", seed=0, device="cpu", **kw)
    net_wrap.wrap_modules_in_net(net, PTQ4ViT)
    return net, torch.from_numpy(g["images"][:2])


def _installed(m):
    f = m.__dict__.get("forward")
    return None if f is None else f.__func__.__name__


def test_fuse_qkv_attention_shares_fuse_attentions_saved_forward(cpu_vit, monkeypatch):
    from ptq4vit_amd import engine
    from ptq4vit_amd.utils import fuse, models
    net, x = cpu_vit
    attns = [n for n, m in net.named_modules() if isinstance(m, models.Attention)]
    mlps = [n for n, m in net.named_modules() if isinstance(m, models.Mlp)]
    assert len(attns) >= 2 and len(mlps) == len(attns)
    mods = dict(net.named_modules())
    for name in ("qkv_attn_quant_forward", "attn_quant_forward", "mlp_quant_forward"):
        monkeypatch.setattr(engine, name, lambda **kw: pytest.fail("a fused path ran on a CPU net"))
    cls_forward = models.Attention.forward
    installed = lambda: {_installed(mods[n]) for n in attns}
    with torch.no_grad():
        y = net(x)
        assert all(fuse.qkv_attention_fusable(mods[n]) and fuse.attention_fusable(mods[n]) for n in attns)
        assert fuse.fuse_qkv_attention(net) == attns and fuse.fuse_qkv_attention(net) == attns      # idempotent
        assert installed() == {"_fused_qkv_attention_forward"}
        saved = [mods[n].__dict__[fuse._ORIG_ATTN] for n in attns]
        assert all(s.__func__ is cls_forward for s in saved)
        probe = torch.randn(2, 5, mods[attns[0]].qkv.in_features)
        assert not any(fuse.takes_fused_qkv_attention_path(mods[n], probe) or fuse.takes_fused_attention_path(mods[n], probe) for n in attns)
        assert torch.equal(net(x), y), "a CPU net keeps its original forward, bit for bit"
        # the later call decides; the saved forward stays the module's own
        assert fuse.fuse_attention(net) == attns and installed() == {"_fused_attention_forward"}
        assert [mods[n].__dict__[fuse._ORIG_ATTN] for n in attns] == saved
        assert torch.equal(net(x), y)
        assert fuse.fuse_qkv_attention(net) == attns and installed() == {"_fused_qkv_attention_forward"}
        assert [mods[n].__dict__[fuse._ORIG_ATTN] for n in attns] == saved
        # unfuse_attention undoes either, in either order; fuse_mlp keeps a saved forward of its own
        assert fuse.fuse_mlp(net) == mlps
        assert fuse.unfuse_attention(net) == attns and fuse.unfuse_attention(net) == []
        assert all("forward" not in mods[n].__dict__ and mods[n].forward.__func__ is cls_forward for n in attns)
        assert all("forward" in mods[n].__dict__ for n in mlps)
        assert fuse.fuse_attention(net) == attns and fuse.fuse_qkv_attention(net) == attns
        assert fuse.unfuse_mlp(net) == mlps and installed() == {"_fused_qkv_attention_forward"}
        assert torch.equal(net(x), y)
        assert fuse.unfuse_attention(net) == attns
        assert torch.equal(net(x), y)
        # an instance-attribute forward that was there before comes back
        att = mods[attns[-1]]
        mine = lambda t: cls_forward(att, t)
        att.forward = mine
        try:
            assert fuse.fuse_qkv_attention(net) == attns and att.__dict__["forward"] is not mine
            assert fuse.fuse_attention(net) == attns
            assert fuse.unfuse_attention(net) == attns and att.__dict__["forward"] is mine
        finally:
            att.__dict__.pop("forward", None)
    assert not any("forward" in m.__dict__ for m in net.modules())


def test_fuse_qkv_attention_skips_what_it_cannot_fuse():
    from ptq4vit_amd.quant_layers.linear import PTQSLBatchingQuantLinear
    from ptq4vit_amd.quant_layers.matmul import PTQSLBatchingQuantMatMul, SoSPTQSLBatchingQuantMatMul
    from ptq4vit_amd.utils import fuse, models
    vit = models.Attention(192, 3)
    vit.matmul1, vit.matmul2 = PTQSLBatchingQuantMatMul(), SoSPTQSLBatchingQuantMatMul()
    holder = torch.nn.Sequential(vit)
    # a plain nn.Linear qkv: fuse_attention's container, not this one's
    assert fuse.attention_fusable(vit) and not fuse.qkv_attention_fusable(vit)
    assert fuse.fuse_qkv_attention(holder) == [] and "forward" not in vit.__dict__
    assert fuse.fuse_attention(holder) == ["0"] and fuse.fuse_qkv_attention(holder) == []
    assert _installed(vit) == "_fused_attention_forward"               # (fuse_qkv_attention leaves fuse_attention's patch alone there)
    assert fuse.unfuse_attention(holder) == ["0"]
    vit.qkv = PTQSLBatchingQuantLinear(192, 576)
    assert fuse.qkv_attention_fusable(vit) and fuse.fuse_qkv_attention(holder) == ["0"]
    assert fuse.unfuse_attention(holder) == ["0"]
    vit.attn_drop = torch.nn.Dropout(0.1)
    assert not fuse.qkv_attention_fusable(vit) and fuse.fuse_qkv_attention(holder) == []
    # Swin's WindowAttention is left alone
    watt = models.WindowAttention(96, (7, 7), 3)
    watt.matmul1, watt.matmul2 = PTQSLBatchingQuantMatMul(), SoSPTQSLBatchingQuantMatMul()
    watt.qkv = PTQSLBatchingQuantLinear(96, 288)
    assert fuse.window_attention_fusable(watt) and not fuse.qkv_attention_fusable(watt)
    assert fuse.fuse_qkv_attention(torch.nn.Sequential(watt)) == []
