"""No GPU: the host side of the fused window attention forward -- p4v_wattn_workspace_bytes / p4v_wattn_quant_forward's argument
checks and envelope (nothing is launched: every pointer is a fake that is never dereferenced), the sizing, and the mechanics of
utils/fuse.py::fuse_window_attention on a CPU tiny Swin.

The entry point takes its tensors, its workspace and the workspace's size in a record (p4v_wattn_tensors), so the table of
tests/test_cabi.py, which finds workspace-taking entry points by their prototype, does not list it: the rule of that table --
every required pointer NULL, one at a time, is P4V_ERR_INVALID with the entry point's own message before any launch -- is
applied to it here.
"""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = "q kT v bias qk_A_interval qk_B_interval pv_A_interval pv_B_interval out ws".split()
OPTIONAL = "mask probs split".split()             # (split: required with sos, its own message)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ptq4vit_amd import _lib
    return _lib.load()


def _fill(d, windows=8, heads=3, N=49, D=32, sos=True, bits=8):
    from ptq4vit_amd import _lib
    q, kT = torch.empty(windows, heads, N, D), torch.empty(windows, heads, N, D).transpose(-2, -1)
    p, v = torch.empty(windows, heads, N, N), torch.empty(windows, heads, N, D)
    for mm, A, B in ((d.qk, q, kT), (d.pv, p, v)):
        mm.batch, mm.heads, mm.M, mm.K, mm.N = windows, heads, A.shape[2], A.shape[3], B.shape[3]
        for i in range(4):
            mm.a_stride[i], mm.b_stride[i] = A.stride(i), B.stride(i)
        mm.A_bit = mm.B_bit = bits
        mm.metric, mm.eq_n, mm.search_round, mm.reserved = _lib.METRICS["L2_norm"], 1, 1, _lib.RESERVED_FORWARD_ONLY
    d.pv.sos = int(sos)
    return d


def _desc(n_windows=4, has_mask=1, **kw):
    from ptq4vit_amd import _lib
    d = _fill(_lib.WattnDesc(), **kw)
    d.n_windows, d.has_mask = n_windows, has_mask
    return d


def _tensors(d, missing=(), ws=64, nbytes=1 << 30):
    from ptq4vit_amd import _lib
    t = _lib.WattnTensors()
    for n in _lib.WattnTensors.POINTERS:
        setattr(t, n, 0 if n in missing else 64)
    if not d.has_mask:
        t.mask = 0
    t.ws, t.ws_bytes = (0 if "ws" in missing else ws), nbytes
    return t


def test_header_prototype_and_version(lib):
    from ptq4vit_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ptq4vit_hip.h")).read()
    proto = re.search(r"\bp4v_wattn_quant_forward\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert proto.count("*") == 3 and "p4v_wattn_desc" in proto and "p4v_wattn_tensors" in proto      # desc, the record, stream
    assert re.search(r"size_t\s+p4v_wattn_workspace_bytes\s*\(\s*const\s+p4v_wattn_desc\s*\*", hdr)
    body = re.search(r"typedef struct p4v_wattn_tensors \{(.*?)\} p4v_wattn_tensors;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = re.findall(r"\*?\s*([A-Za-z_][A-Za-z0-9_]*)\s*[,;]", body)
    assert tuple(members) == _lib.WattnTensors.POINTERS + ("ws_bytes",), members
    assert set(REQUIRED + OPTIONAL) == set(_lib.WattnTensors.POINTERS)
    assert lib.p4v_version() >= 144
    assert {"p4v_wattn_workspace_bytes", "p4v_wattn_quant_forward"} <= set(_lib.EXPORTS)


def test_sizing_is_the_plain_attention_calls(lib):
    from ptq4vit_amd import _lib
    for kw in (dict(), dict(sos=False), dict(windows=4, heads=4, N=144), dict(windows=8, heads=2, N=49, D=12, bits=6)):
        for n_windows, has_mask in ((4, 1), (1, 0), (2, 1)):
            a = _fill(_lib.AttnDesc(), **kw)
            a.scale = 1.0
            need = lib.p4v_attn_workspace_bytes(C.byref(a))
            assert need > 4096
            assert lib.p4v_wattn_workspace_bytes(C.byref(_desc(n_windows, has_mask, **kw))) == need, (kw, n_windows, has_mask)
    assert lib.p4v_wattn_workspace_bytes(None) == 0
    # Swin-B/384 x 128, stage 1: 128 * 64 windows of 144 tokens, 4 heads -- accepted
    assert lib.p4v_wattn_workspace_bytes(C.byref(_desc(64, 1, windows=8192, heads=4, N=144))) > 2 * 8192 * 4 * 256 * 192


def test_envelope_refusals_launch_nothing(lib):
    from ptq4vit_amd import engine
    before = engine.launch_counters()

    def refused(d, code, msg, sizing=True):
        if sizing:
            assert lib.p4v_wattn_workspace_bytes(C.byref(d)) == 0 and msg in lib.p4v_last_error(), lib.p4v_last_error()
        assert lib.p4v_wattn_quant_forward(C.byref(d), C.byref(_tensors(d)), None) == code and msg in lib.p4v_last_error(), lib.p4v_last_error()

    # the new ones
    refused(_desc(n_windows=0), -1, b"n_windows = 0 is not positive")
    refused(_desc(n_windows=-2), -1, b"is not positive")
    refused(_desc(n_windows=3), -1, b"qk.batch = 8 is no multiple of n_windows = 3")
    d = _desc(has_mask=1)
    t = _tensors(d)
    t.mask = 0
    assert lib.p4v_wattn_quant_forward(C.byref(d), C.byref(t), None) == -1 and b"has_mask = 1 but the mask pointer is null" in lib.p4v_last_error()
    d = _desc(has_mask=0)
    t = _tensors(d)
    t.mask = 64
    assert lib.p4v_wattn_quant_forward(C.byref(d), C.byref(t), None) == -1 and b"has_mask = 0 but the mask pointer is set" in lib.p4v_last_error()
    d = _desc()                                       # (the kernel addresses bias and mask with 32-bit element offsets)
    d.qk.M = d.pv.M = d.qk.N = d.pv.K = 20000
    refused(d, -2, b"of 2^30 elements or more")
    # the plain attention call's, through this entry point
    d = _desc()
    d.qk.sos = 1
    refused(d, -2, b"no split-of-softmax operand")
    d = _desc()
    d.pv.K = 48
    refused(d, -1, b"is not the row operand")
    d = _desc()
    d.pv.heads = 2
    refused(d, -1, b"is not the row operand")
    for side, field in (("qk", "A_bit"), ("pv", "B_bit")):
        for bad in (1, 9):
            d = _desc()
            setattr(getattr(d, side), field, bad)
            refused(d, -2, b"bit widths 2..8")
    d = _desc()
    d.pv.reserved |= 1
    refused(d, -2, b"int8 planes only")
    assert engine.launch_counters() == before


def test_every_required_pointer_is_checked_before_any_launch(lib):
    from ptq4vit_amd import engine
    before = engine.launch_counters()
    d = _desc()
    says = "p4v_wattn_quant_forward: null pointer"
    assert lib.p4v_wattn_quant_forward(None, C.byref(_tensors(d)), None) == -1 and lib.p4v_last_error().decode() == says
    assert lib.p4v_wattn_quant_forward(C.byref(d), None, None) == -1 and lib.p4v_last_error().decode() == says
    for missing in REQUIRED:
        rc = lib.p4v_wattn_quant_forward(C.byref(d), C.byref(_tensors(d, missing=(missing,))), None)
        assert rc == -1 and lib.p4v_last_error().decode() == says, (missing, rc, lib.p4v_last_error())
    rc = lib.p4v_wattn_quant_forward(C.byref(d), C.byref(_tensors(d, missing=("split",))), None)
    assert rc == -1 and lib.p4v_last_error().decode() == "p4v_wattn_quant_forward: sos needs split"
    # the optional members: no complaint about them -- the call gets as far as the declared size (one byte: too small)
    plain, nomask = _desc(sos=False), _desc(has_mask=0)
    for dd, missing in ((d, ("probs",)), (plain, ("split",)), (plain, ("split", "probs")), (nomask, ("mask",)), (nomask, ("mask", "probs"))):
        rc = lib.p4v_wattn_quant_forward(C.byref(dd), C.byref(_tensors(dd, missing=missing, nbytes=1)), None)
        assert rc == -3 and b"workspace too small" in lib.p4v_last_error(), (missing, rc, lib.p4v_last_error())
    # alignment, and one byte too few
    assert lib.p4v_wattn_quant_forward(C.byref(d), C.byref(_tensors(d, ws=72)), None) == -1 and b"aligned" in lib.p4v_last_error()
    need = lib.p4v_wattn_workspace_bytes(C.byref(d))
    assert lib.p4v_wattn_quant_forward(C.byref(d), C.byref(_tensors(d, nbytes=need - 1)), None) == -3
    assert b"workspace too small: need >= %d bytes" % need in lib.p4v_last_error()
    assert engine.launch_counters() == before


# ---- utils/fuse.py on a CPU tiny Swin ----------------------------------------------------------------------------------------------
SWIN_KW = dict(img_size=56, embed_dim=24, depths=(2, 2), num_heads=(2, 4))


@pytest.fixture(scope="module")
def cpu_swin():
    from ptq4vit_amd.configs import PTQ4ViT
    from ptq4vit_amd.utils import models, net_wrap
    net = models.get_net("swin_tiny_patch4_window7_224", seed=0, device="cpu", **SWIN_KW)
    net_wrap.wrap_modules_in_net(net, PTQ4ViT)
    return net


def test_fuse_window_attention_patches_window_attention_containers_only(cpu_swin, monkeypatch):
    from ptq4vit_amd import engine
    from ptq4vit_amd.utils import fuse, models
    net = cpu_swin
    watts = [n for n, m in net.named_modules() if isinstance(m, models.WindowAttention)]
    mlps = [n for n, m in net.named_modules() if isinstance(m, models.Mlp)]
    assert len(watts) == 4 and len(mlps) == 4
    mods = dict(net.named_modules())
    assert any(getattr(m, "attn_mask", None) is not None for m in net.modules()), "the tiny Swin has a shifted block"
    for name in ("window_attn_quant_forward", "attn_quant_forward", "mlp_quant_forward"):
        monkeypatch.setattr(engine, name, lambda **kw: pytest.fail("a fused path ran on a CPU net"))
    cls_forward = models.WindowAttention.forward
    x = torch.randn(2, 3, 56, 56, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        y = net(x)
        assert fuse.fuse_attention(net) == []                                        # as before: nothing on a Swin net
        assert fuse.fuse_window_attention(net) == watts and fuse.fuse_window_attention(net) == watts      # idempotent
        assert all(fuse.window_attention_fusable(mods[n]) and not fuse.attention_fusable(mods[n]) for n in watts)
        assert fuse.fuse_mlp(net) == mlps                                            # saved forwards of their own: they compose
        assert fuse.fuse_attention(net) == []
        assert all("forward" in mods[n].__dict__ for n in watts + mlps)
        probe = torch.randn(4, 49, mods[watts[0]].qkv.in_features)
        assert not any(fuse.takes_fused_window_attention_path(mods[n], torch.randn(4, 49, mods[n].qkv.in_features)) for n in watts)
        assert not fuse.takes_fused_window_attention_path(mods[watts[0]], probe, torch.zeros(4, 49, 49))
        assert torch.equal(net(x), y), "a CPU net keeps its original forward, bit for bit"
        assert fuse.unfuse_window_attention(net) == watts and fuse.unfuse_window_attention(net) == []
        assert all("forward" not in mods[n].__dict__ and mods[n].forward.__func__ is cls_forward for n in watts)
        assert all("forward" in mods[n].__dict__ for n in mlps)
        assert torch.equal(net(x), y)
        # the other order
        assert fuse.fuse_window_attention(net) == watts
        assert fuse.unfuse_mlp(net) == mlps and all("forward" in mods[n].__dict__ for n in watts)
        assert torch.equal(net(x), y)
        assert fuse.unfuse_window_attention(net) == watts
        assert torch.equal(net(x), y)
    assert not any("forward" in m.__dict__ for m in net.modules())


def test_fuse_window_attention_skips_what_it_cannot_fuse():
    from ptq4vit_amd.quant_layers.matmul import PTQSLBatchingQuantMatMul, SoSPTQSLBatchingQuantMatMul
    from ptq4vit_amd.utils import fuse, models
    att = models.WindowAttention(96, (7, 7), 3)                          # plain MatMul modules: not this package's quant classes
    assert not fuse.window_attention_fusable(att) and fuse.fuse_window_attention(torch.nn.Sequential(att)) == []
    att.matmul1, att.matmul2 = PTQSLBatchingQuantMatMul(), SoSPTQSLBatchingQuantMatMul()
    assert fuse.window_attention_fusable(att) and not fuse.attention_fusable(att)
    att.attn_drop = torch.nn.Dropout(0.1)
    assert not fuse.window_attention_fusable(att)
    vit = models.Attention(192, 3)
    vit.matmul1, vit.matmul2 = PTQSLBatchingQuantMatMul(), SoSPTQSLBatchingQuantMatMul()
    assert fuse.attention_fusable(vit) and not fuse.window_attention_fusable(vit)
