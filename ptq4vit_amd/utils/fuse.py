"""Opt-in, network-level fusion of the quantised MLP forward: fc1 -> GELU -> fc2's activation quantiser -> fc2 with int8 in
between (engine.mlp_quant_forward / p4v_mlp_quant_forward).

The drop-in contract keeps every quant module doing what the reference's does; nothing here changes a module.  `fuse_mlp(net)`
patches the `forward` of the MLP *containers* -- every module with `fc1`, `act`, `fc2` where `act` is the exact (erf) nn.GELU
and fc1 / fc2 are this package's PTQSL Linear classes: models.Mlp, so ViT, DeiT and Swin alike -- and the patched forward decides
per call: the fused path only when both layers are calibrated, in quant_forward, on the int8 path and inside the engine's
envelope, the tensor is on the GPU, autograd is not recording and none of the three modules carries a forward (pre-)hook.  In
every other state (raw, the calibration modes, capture hooks, CPU tensors) it calls the original forward, so calibrators behave
exactly as on an unfused net.  Nothing calls `fuse_mlp` by default; `unfuse_mlp(net)` restores.

`fuse_attention(net)` / `unfuse_attention(net)` / `takes_fused_attention_path(m, x)` are the same for the attention side: the
patched forward of a `models.Attention` repeats its forward -- the same qkv call, the same P4V_QKV_CONTIGUOUS branch, the same proj
-- and replaces matmul1 -> `* scale` -> softmax -> matmul2 by engine.attn_quant_forward (p4v_attn_quant_forward)
when both MatMuls are calibrated, in quant_forward, head-wise, on the int8 path and unhooked; otherwise the original forward.
"""
import os
import types

import torch
import torch.nn as nn

from .. import engine
from ..quant_layers.linear import PTQSLQuantLinear
from ..quant_layers.matmul import PTQSLQuantMatMul
from . import models

_ORIG = "_p4v_unfused_forward"


def _exact_gelu(act):
    return isinstance(act, nn.GELU) and getattr(act, "approximate", "none") == "none"


def fusable(m):
    """The static half of the decision: an MLP container whose forward `fuse_mlp` patches."""
    fc1, act, fc2 = getattr(m, "fc1", None), getattr(m, "act", None), getattr(m, "fc2", None)
    return _exact_gelu(act) and isinstance(fc1, PTQSLQuantLinear) and isinstance(fc2, PTQSLQuantLinear)


def _hooked(m):
    return bool(m._forward_hooks) or bool(m._forward_pre_hooks)


def _in_envelope(fc):
    """What p4v_mlp_quant_forward takes of one layer (include/ptq4vit_hip.h)."""
    return (2 <= fc.w_bit <= 8 and 2 <= fc.a_bit <= 8 and fc.n_H == 1 and fc.n_a == 1 and fc.out_features % fc.n_V == 0)


def _ready(fc):
    return (getattr(fc, "calibrated", None) and fc.mode == "quant_forward" and fc.int8_forward and _in_envelope(fc)
            and fc.w_interval is not None and fc.a_interval is not None)


def takes_fused_path(m, x):
    """The per-call half: would the patched forward of `m` run the fused kernel chain on `x`?"""
    if not fusable(m):
        return False
    fc1, act, fc2 = m.fc1, m.act, m.fc2
    if not (_ready(fc1) and _ready(fc2)) or fc1._postgelu:
        return False
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() >= 2 and x.shape[-1] == fc1.in_features
            and fc1.out_features == fc2.in_features):
        return False
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for fc in (fc1, fc2) for p in fc.parameters())):
        return False
    return not (_hooked(fc1) or _hooked(act) or _hooked(fc2))


def _layer(fc):
    return dict(weight=fc.weight.data, bias=None if fc.bias is None else fc.bias.data, w_interval=fc.w_interval,
                a_interval=fc._positive_a_interval(), w_bit=fc.w_bit, a_bit=fc.a_bit, n_V=fc.n_V, n_H=fc.n_H, n_a=fc.n_a,
                postgelu=fc._postgelu)


def _fused_forward(self, x):
    if takes_fused_path(self, x):
        return engine.mlp_quant_forward(x=x, fc1=_layer(self.fc1), fc2=_layer(self.fc2))
    return self.__dict__[_ORIG](x)


def fuse_mlp(net):
    """Patch the forward of every fusable MLP container of `net`; returns their names.  Idempotent."""
    names = []
    for name, m in net.named_modules():
        if not fusable(m):
            continue
        if _ORIG not in m.__dict__:
            m.__dict__[_ORIG] = m.forward
            m.forward = types.MethodType(_fused_forward, m)
        names.append(name)
    return names


def _unfuse(net, attr):
    names = []
    for name, m in net.named_modules():
        orig = m.__dict__.pop(attr, None)
        if orig is None:
            continue
        m.__dict__.pop("forward", None)
        if not (getattr(orig, "__self__", None) is m and getattr(orig, "__func__", None) is getattr(type(m), "forward", None)):
            m.forward = orig          # the forward was an instance attribute before: put that one back
        names.append(name)
    return names


def unfuse_mlp(net):
    """Undo fuse_mlp: every patched container gets its original forward back; returns their names.  Idempotent."""
    return _unfuse(net, _ORIG)


# ---- the attention side: matmul1 -> * scale -> softmax -> matmul2 (engine.attn_quant_forward) ----------------------
# Same shape as the MLP functions, with a saved-forward attribute of its own: an Attention is no MLP container, so fuse_mlp and
# fuse_attention patch different modules and compose in any order.  WindowAttention (Swin) scales q BEFORE matmul1 and adds a
# position bias and a mask before the softmax: not this kernel's arithmetic, fuse_attention skips it.
_ORIG_ATTN = "_p4v_unfused_attn_forward"


def _inactive_dropout(drop):
    return isinstance(drop, nn.Identity) or (isinstance(drop, nn.Dropout) and (not drop.training or drop.p == 0))


def attention_fusable(m):
    """The static half of the decision: an Attention container whose forward `fuse_attention` patches."""
    return (isinstance(m, models.Attention) and isinstance(m.matmul1, PTQSLQuantMatMul) and isinstance(m.matmul2, PTQSLQuantMatMul)
            and _inactive_dropout(m.attn_drop))


def _matmul_ready(mm):
    return (getattr(mm, "calibrated", None) and mm.mode == "quant_forward" and mm.int8_forward and not engine.has_blocks(mm._blocks)
            and 2 <= mm.A_bit <= 8 and 2 <= mm.B_bit <= 8 and mm.A_interval is not None and mm.B_interval is not None
            and (not mm._sos or mm.split is not None))


def takes_fused_attention_path(m, x):
    """The per-call half: would the patched forward of `m` run the fused kernel chain on `x`?"""
    if not attention_fusable(m):
        return False
    m1, m2 = m.matmul1, m.matmul2
    if not (_matmul_ready(m1) and _matmul_ready(m2)) or m1._sos:
        return False
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 3 and x.dtype == torch.float32):
        return False
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in m.qkv.parameters())):
        return False
    return not (_hooked(m1) or _hooked(m2) or _hooked(m.attn_drop))


def _matmul_side(mm, H):
    side = dict(A_interval=mm.A_interval if mm._sos else mm._per_head(mm.A_interval, H, mm.crb_groups_A),
                B_interval=mm._per_head(mm.B_interval, H, mm.crb_groups_B), A_bit=mm.A_bit, B_bit=mm.B_bit, blocks=mm._blocks,
                sos=mm._sos)
    if mm._sos:
        side["split"] = mm.split
    return side


def _fused_attention_forward(self, x):
    if not takes_fused_attention_path(self, x):
        return self.__dict__[_ORIG_ATTN](x)
    # models.Attention.forward, with matmul1 ... matmul2 as one engine call
    B, N, C = x.shape
    H = self.num_heads
    qkv = self.qkv(x).reshape(B, N, 3, H, C // H).permute(2, 0, 3, 1, 4)
    if os.environ.get("P4V_QKV_CONTIGUOUS", "1") == "1":
        qkv = qkv.contiguous()
    q, k, v = qkv.unbind(0)
    kT = k.transpose(-2, -1)
    for mm, (a, b) in ((self.matmul1, (q, kT)), (self.matmul2, (torch.empty(B, H, N, N, device="meta"), v))):
        if mm.crb_rows_A is None or mm.crb_rows_B is None:
            mm._get_padding_parameters(a, b)          # (intervals loaded from elsewhere: as in quant_forward)
    out = engine.attn_quant_forward(q=q, kT=kT, v=v, scale=self.scale, qk=_matmul_side(self.matmul1, H), pv=_matmul_side(self.matmul2, H))
    return self.proj_drop(self.proj(out.transpose(1, 2).reshape(B, N, C)))


def fuse_attention(net):
    """Patch the forward of every fusable Attention container of `net`; returns their names.  Idempotent."""
    names = []
    for name, m in net.named_modules():
        if not attention_fusable(m):
            continue
        if _ORIG_ATTN not in m.__dict__:
            m.__dict__[_ORIG_ATTN] = m.forward
            m.forward = types.MethodType(_fused_attention_forward, m)
        names.append(name)
    return names


def unfuse_attention(net):
    """Undo fuse_attention: every patched container gets its original forward back; returns their names.  Idempotent."""
    return _unfuse(net, _ORIG_ATTN)
