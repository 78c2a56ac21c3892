"""No GPU: the host side of the fused attention forward -- the C entry points' argument checks and envelope (nothing is launched:
every pointer is a fake that is never dereferenced), the sizing, and the mechanics of utils/fuse.py::fuse_attention on a CPU net.

That every required pointer is checked is asserted by the table of tests/test_cabi.py (p4v_attn_quant_forward takes its workspace
as d_ws and has its row there); here: the alignment, the declared size, the debug entry point.
"""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTERS = "q kT v qk_A_interval qk_B_interval pv_A_interval pv_B_interval split out ?probs".split()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ptq4vit_amd import _lib
    return _lib.load()


def _desc(batch=2, heads=3, N=197, D=64, sos=True, bits=8):
    from ptq4vit_amd import _lib
    d = _lib.AttnDesc()
    q, kT = torch.empty(batch, heads, N, D), torch.empty(batch, heads, N, D).transpose(-2, -1)
    p, v = torch.empty(batch, heads, N, N), torch.empty(batch, heads, N, D)
    for mm, A, B in ((d.qk, q, kT), (d.pv, p, v)):
        mm.batch, mm.heads, mm.M, mm.K, mm.N = batch, heads, A.shape[2], A.shape[3], B.shape[3]
        for i in range(4):
            mm.a_stride[i], mm.b_stride[i] = A.stride(i), B.stride(i)
        mm.A_bit = mm.B_bit = bits
        mm.metric, mm.eq_n, mm.search_round, mm.reserved = _lib.METRICS["L2_norm"], 1, 1, _lib.RESERVED_FORWARD_ONLY
    d.pv.sos, d.scale = int(sos), D ** -0.5
    return d


def test_header_prototype_and_version(lib):
    hdr = open(os.path.join(ROOT, "include", "ptq4vit_hip.h")).read()
    proto = re.search(r"\bp4v_attn_quant_forward\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert proto.count("*") == 1 + len(POINTERS) + 2                   # desc, the tensors, workspace, stream
    assert lib.p4v_version() >= 143


def test_sizing_and_envelope(lib):
    need = lib.p4v_attn_workspace_bytes(C.byref(_desc()))
    Z, Mp, Kp = 6, 256, 256
    assert 2 * Z * Mp * Kp <= need < 16 * Z * Mp * Kp                  # the two planes of p, the planes of q, k^T and v, the tables
    assert lib.p4v_attn_workspace_bytes(C.byref(_desc(sos=False))) < need
    assert lib.p4v_attn_workspace_bytes(C.byref(_desc(batch=1, heads=2, N=577))) > 2 * 2 * 640 * 640   # ViT-B/384's 577 keys
    assert lib.p4v_attn_workspace_bytes(None) == 0
    one = C.c_void_p(64)

    def refused(d, code, msg):
        assert lib.p4v_attn_workspace_bytes(C.byref(d)) == 0 and msg in lib.p4v_last_error(), lib.p4v_last_error()
        assert lib.p4v_attn_quant_forward(C.byref(d), *[one] * 10, one, 1 << 30, None) == code and msg in lib.p4v_last_error()

    from ptq4vit_amd import engine
    before = engine.launch_counters()
    d = _desc()
    d.qk.sos = 1
    refused(d, -2, b"no split-of-softmax operand")
    d = _desc()
    d.pv.K = 196
    refused(d, -1, b"is not the row operand")
    d = _desc()
    d.pv.heads = 2
    refused(d, -1, b"is not the row operand")
    for side, field in (("qk", "A_bit"), ("qk", "B_bit"), ("pv", "A_bit"), ("pv", "B_bit")):
        for bad in (1, 9):
            d = _desc()
            setattr(getattr(d, side), field, bad)
            refused(d, -2, b"bit widths 2..8")
    d = _desc()
    d.pv.reserved |= 1
    refused(d, -2, b"int8 planes only")
    assert engine.launch_counters() == before


def test_required_pointers_alignment_and_size(lib):
    d = _desc()
    one, null = C.c_void_p(64), C.c_void_p(0)

    def call(ws=one, nbytes=1 << 30):
        return lib.p4v_attn_quant_forward(C.byref(d), *[one] * len(POINTERS), ws, nbytes, null)

    assert call(ws=C.c_void_p(72)) == -1 and b"aligned" in lib.p4v_last_error()
    need = lib.p4v_attn_workspace_bytes(C.byref(d))
    assert call(nbytes=need - 1) == -3 and b"workspace too small" in lib.p4v_last_error()
    assert lib.p4v_debug_attn_planes(None) == -1


# ---- utils/fuse.py on a CPU net: what fuse_attention patches, and that an uncalibrated / CPU net keeps its original forward --------
@pytest.fixture(scope="module")
def cpu_net():
    from ptq4vit_amd.configs import PTQ4ViT
    from ptq4vit_amd.utils import models, net_wrap
    net = models.get_net("vit_tiny_patch16_224", seed=0, device="cpu", img_size=32, depth=2)
    net_wrap.wrap_modules_in_net(net, PTQ4ViT)
    return net


def test_fuse_attention_patches_attention_containers_only(cpu_net, monkeypatch):
    from ptq4vit_amd import engine
    from ptq4vit_amd.utils import fuse, models
    net = cpu_net
    attns = [n for n, m in net.named_modules() if isinstance(m, models.Attention)]
    mlps = [n for n, m in net.named_modules() if isinstance(m, models.Mlp)]
    assert len(attns) == 2 and len(mlps) == 2
    monkeypatch.setattr(engine, "attn_quant_forward", lambda **kw: pytest.fail("the fused path ran on a CPU net"))
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        y = net(x)
        assert fuse.fuse_attention(net) == attns and fuse.fuse_attention(net) == attns
        assert fuse.fuse_mlp(net) == mlps                               # a saved forward of its own: the two compose
        mods = dict(net.named_modules())
        assert all("forward" in mods[n].__dict__ for n in attns + mlps)
        assert not any(fuse.takes_fused_attention_path(mods[n], torch.randn(2, 5, mods[n].qkv.in_features)) for n in attns)
        assert torch.equal(net(x), y)
        assert fuse.unfuse_attention(net) == attns and fuse.unfuse_attention(net) == []
        assert all("forward" not in mods[n].__dict__ for n in attns) and all("forward" in mods[n].__dict__ for n in mlps)
        assert fuse.unfuse_mlp(net) == mlps
        assert torch.equal(net(x), y)


def test_fuse_attention_skips_what_it_cannot_fuse():
    from ptq4vit_amd.utils import fuse, models
    att = models.Attention(192, 3)                                      # plain MatMul modules: not this package's quant classes
    assert not fuse.attention_fusable(att) and fuse.fuse_attention(torch.nn.Sequential(att)) == []
    from ptq4vit_amd.quant_layers.matmul import PTQSLBatchingQuantMatMul, SoSPTQSLBatchingQuantMatMul
    att.matmul1, att.matmul2 = PTQSLBatchingQuantMatMul(), SoSPTQSLBatchingQuantMatMul()
    assert fuse.attention_fusable(att)
    att.attn_drop = torch.nn.Dropout(0.1)
    assert not fuse.attention_fusable(att)                              # an active dropout
    att.eval()
    assert fuse.attention_fusable(att)
    att.train()
    att.attn_drop = torch.nn.Dropout(0.0)
    assert fuse.attention_fusable(att)
    assert not any(fuse.attention_fusable(m) for m in models.WindowAttention(96, (7, 7), 3).modules())
