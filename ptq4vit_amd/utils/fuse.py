"""Opt-in, network-level fusion of the quantised MLP forward: fc1 -> GELU -> fc2's activation quantiser -> fc2 with int8 in
between (engine.mlp_quant_forward / p4v_mlp_quant_forward).

The drop-in contract keeps every quant module doing what the reference's does; nothing here changes a module.  `fuse_mlp(net)`
patches the `forward` of the MLP *containers* -- every module with `fc1`, `act`, `fc2` where `act` is the exact (erf) nn.GELU
and fc1 / fc2 are this package's PTQSL Linear classes: models.Mlp, so ViT, DeiT and Swin alike -- and the patched forward decides
per call: the fused path only when both layers are calibrated, in quant_forward, on the int8 path and inside the engine's
envelope, the tensor is on the GPU, autograd is not recording and none of the three modules carries a forward (pre-)hook.  In
every other state (raw, the calibration modes, capture hooks, CPU tensors) it calls the original forward, so calibrators behave
exactly as on an unfused net.  Nothing calls `fuse_mlp` by default; `unfuse_mlp(net)` restores.
"""
import types

import torch
import torch.nn as nn

from .. import engine
from ..quant_layers.linear import PTQSLQuantLinear

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


def unfuse_mlp(net):
    """Undo fuse_mlp: every patched container gets its original forward back; returns their names.  Idempotent."""
    names = []
    for name, m in net.named_modules():
        orig = m.__dict__.pop(_ORIG, None)
        if orig is None:
            continue
        m.__dict__.pop("forward", None)
        if not (getattr(orig, "__self__", None) is m and getattr(orig, "__func__", None) is getattr(type(m), "forward", None)):
            m.forward = orig          # the forward was an instance attribute before: put that one back
        names.append(name)
    return names
