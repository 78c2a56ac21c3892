"""Opt-in, network-level fusion of the quantised MLP forward: fc1 -> GELU -> fc2's activation quantiser -> fc2 with int8 in
between (engine.mlp_quant_forward / p4v_mlp_quant_forward).

The drop-in contract keeps every quant module doing what the reference's does; nothing here changes a module.  `fuse_mlp(net)`
patches the `forward` of the MLP *containers* -- every module with `fc1`, `act`, `fc2` where `act` is the exact (erf) nn.GELU
and fc1 / fc2 are this package's PTQSL Linear classes: models.Mlp, so ViT, DeiT and Swin alike -- and the patched forward decides
per call: the fused path only when both layers are calibrated, in quant_forward, on the int8 path (the layers' own verdict and
engine keywords: _int8_ready / _int8_args, what their quant_forward uses) and inside the fused entry point's narrower
envelope, the tensor is on the GPU, autograd is not recording and none of the three modules carries a forward (pre-)hook.  In
every other state (raw, the calibration modes, capture hooks, CPU tensors) it calls the original forward, so calibrators behave
exactly as on an unfused net.  Nothing calls `fuse_mlp` by default; `unfuse_mlp(net)` restores.

`fuse_attention(net)` / `unfuse_attention(net)` / `takes_fused_attention_path(m, x)` are the same for the attention side: the
patched forward of a `models.Attention` repeats its forward -- the same qkv call, the same P4V_QKV_CONTIGUOUS branch, the same proj
-- and replaces matmul1 -> `* scale` -> softmax -> matmul2 by engine.attn_quant_forward (p4v_attn_quant_forward)
when both MatMuls are calibrated, in quant_forward, head-wise, on the int8 path and unhooked; otherwise the original forward.

`fuse_window_attention(net)` / `unfuse_window_attention(net)` / `takes_fused_window_attention_path(m, x, mask=None)` are the
same for Swin's `models.WindowAttention`, which fuse_attention leaves alone: the patched forward(x, mask=None) repeats the
module's -- qkv, `q * self.scale` in torch (matmul1 was calibrated on the scaled q), the bias gather / permute / contiguous, proj
-- and replaces matmul1 -> `+ bias` -> `+ mask` -> softmax -> matmul2 by engine.window_attn_quant_forward
(p4v_wattn_quant_forward) under fuse_attention's per-call conditions and one more: the mask is None or a
float32 [nW][N][N] tensor with B_ % nW == 0.  Each of the three fuse_* keeps its own saved forward: they compose in any order.

`fuse_qkv_attention(net)` / `takes_fused_qkv_attention_path(m, x)` take the qkv layer of a `models.Attention` into the chain
(engine.qkv_attn_quant_forward / p4v_qkv_attn_quant_forward): qkv's GEMM writes the int8 operand planes of
the two MatMuls.  It shares fuse_attention's saved forward -- the two do not stack, the later call decides which forward is
installed, unfuse_attention undoes either -- and its patched forward decides per call: the qkv-fused path when fuse_attention's
conditions hold and qkv is calibrated, in quant_forward, on the int8 path, unhooked, n_H = n_a = 1, no post-GELU layer, 3 * C
wide; otherwise fuse_attention's path where its conditions hold; otherwise the original forward.
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


def _live(q):
    """A quant module whose forward the patched container may bypass: calibrated, in the mode that forward would dispatch to
    quant_forward, and nobody listening on it."""
    return bool(getattr(q, "calibrated", None)) and q.mode == "quant_forward" and not _hooked(q)


def _recording(x, *modules):
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for m in modules for p in m.parameters()))


# Whether a module is on its int8 path, and with which engine keywords, the module says itself (_int8_ready / _int8_args of
# quant_layers/linear.py and matmul.py: what its own quant_forward uses).  Stated here, and only here, is what the fused entry
# points take LESS than the single ones (include/ptq4vit_hip.h):
#   p4v_mlp_quant_forward    n_H = n_a = 1 on both layers, fc1 no post-GELU layer
#   p4v_attn_quant_forward   no row / column sub-blocks, matmul1 no split-of-softmax operand; a float32 [B][N][C] input
#   p4v_wattn_quant_forward  the same; the mask None or float32 [nW][N][N], B_ % nW == 0
# (_layer / _matmul_side: the names under which the tests fetch those keywords for a direct engine call)
_layer, _matmul_side = (lambda fc: fc._int8_args()), (lambda mm, H: mm._int8_args(H))


def _mlp_args(m, x):
    """(fc1's, fc2's engine keywords) if the patched forward of `m` runs the fused chain on `x`, else None."""
    if not (fusable(m) and torch.is_tensor(x) and x.dim() >= 2):
        return None
    fc1, fc2 = m.fc1, m.fc2
    if not (_live(fc1) and _live(fc2)) or _hooked(m.act) or _recording(x, fc1, fc2):
        return None
    if x.shape[-1] != fc1.in_features or fc1.out_features != fc2.in_features:
        return None
    # (fc2 is asked with x: its input would lie where x lies, and records autograd only when _recording says so)
    if not (fc1._int8_ready(x) and fc2._int8_ready(x)):
        return None
    a1, a2 = fc1._int8_args(), fc2._int8_args()
    if a1["postgelu"] or any(a["n_H"] != 1 or a["n_a"] != 1 for a in (a1, a2)):
        return None
    return a1, a2


def takes_fused_path(m, x):
    """The per-call half: would the patched forward of `m` run the fused kernel chain on `x`?"""
    return _mlp_args(m, x) is not None


def _fused_forward(self, x):
    args = _mlp_args(self, x)
    if args is not None:
        return engine.mlp_quant_forward(x=x, fc1=args[0], fc2=args[1])
    return self.__dict__[_ORIG](x)


def _patch(net, predicate, attr, forward, replace=False):
    """`replace`: two patched forwards share `attr` -- a container that already carries one gets `forward` installed over it,
    its saved original stays."""
    names = []
    for name, m in net.named_modules():
        if not predicate(m):
            continue
        if attr not in m.__dict__:
            m.__dict__[attr] = m.forward
            m.forward = types.MethodType(forward, m)
        elif replace:
            m.forward = types.MethodType(forward, m)
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


def fuse_mlp(net):
    """Patch the forward of every fusable MLP container of `net`; returns their names.  Idempotent."""
    return _patch(net, fusable, _ORIG, _fused_forward)


def unfuse_mlp(net):
    """Undo fuse_mlp: every patched container gets its original forward back; returns their names.  Idempotent."""
    return _unfuse(net, _ORIG)


# ---- the attention side: matmul1 -> * scale -> softmax -> matmul2 (engine.attn_quant_forward) ----------------------
# Same shape as the MLP functions, with a saved-forward attribute of its own: an Attention is no MLP container, so fuse_mlp and
# fuse_attention patch different modules and compose in any order.  WindowAttention (Swin) scales q BEFORE matmul1 and adds a
# position bias and a mask before the softmax: not that kernel instance's arithmetic, fuse_attention skips it (it has
# fuse_window_attention, below).
_ORIG_ATTN = "_p4v_unfused_attn_forward"


def _inactive_dropout(drop):
    return isinstance(drop, nn.Identity) or (isinstance(drop, nn.Dropout) and (not drop.training or drop.p == 0))


def attention_fusable(m):
    """The static half of the decision: an Attention container whose forward `fuse_attention` patches."""
    return (isinstance(m, models.Attention) and isinstance(m.matmul1, PTQSLQuantMatMul) and isinstance(m.matmul2, PTQSLQuantMatMul)
            and _inactive_dropout(m.attn_drop))


def _attn_args(m, x, static=attention_fusable):
    """(matmul1's, matmul2's engine keywords) if the patched forward of `m` runs the fused chain on `x`, else None."""
    if not (static(m) and torch.is_tensor(x) and x.dim() == 3 and x.dtype == torch.float32):
        return None
    m1, m2 = m.matmul1, m.matmul2
    if not (_live(m1) and _live(m2)) or _hooked(m.attn_drop) or _recording(x, m.qkv):
        return None
    # the MatMuls are asked before qkv runs: stand-ins without rows for q / v (k^T: transposed) and the probabilities
    H, N = m.num_heads, x.shape[1]
    qv, p = x.new_empty((0, H, N, x.shape[2] // H)), x.new_empty((0, H, N, N))
    if not (m1._int8_ready(qv, qv.transpose(-2, -1)) and m2._int8_ready(p, qv)):
        return None
    qk, pv = m1._int8_args(H), m2._int8_args(H)
    if qk["sos"] or "blocks" in qk or "blocks" in pv:
        return None
    return qk, pv


def takes_fused_attention_path(m, x):
    """The per-call half: would the patched forward of `m` run the fused kernel chain on `x`?"""
    return _attn_args(m, x) is not None


def _fused_attention_forward(self, x):
    args = _attn_args(self, x)
    if args is None:
        return self.__dict__[_ORIG_ATTN](x)
    # models.Attention.forward, with matmul1 ... matmul2 as one engine call
    B, N, C = x.shape
    H = self.num_heads
    qkv = self.qkv(x).reshape(B, N, 3, H, C // H).permute(2, 0, 3, 1, 4)
    if os.environ.get("P4V_QKV_CONTIGUOUS", "1") == "1":
        qkv = qkv.contiguous()
    q, k, v = qkv.unbind(0)
    out = engine.attn_quant_forward(q=q, kT=k.transpose(-2, -1), v=v, scale=self.scale, qk=args[0], pv=args[1])
    return self.proj_drop(self.proj(out.transpose(1, 2).reshape(B, N, C)))


def fuse_attention(net):
    """Patch the forward of every fusable Attention container of `net`; returns their names.  Idempotent.  On a container
    fuse_qkv_attention patched it replaces that forward (the two share the saved forward: the later call decides)."""
    return _patch(net, attention_fusable, _ORIG_ATTN, _fused_attention_forward, replace=True)


def unfuse_attention(net):
    """Undo fuse_attention or fuse_qkv_attention: every patched container gets its original forward back; returns their names.
    Idempotent."""
    return _unfuse(net, _ORIG_ATTN)


# ---- qkv in front of the attention chain (engine.qkv_attn_quant_forward) -------------------------------------------
# The qkv layer's GEMM writes the int8 operand planes of the two MatMuls: p4v_qkv_attn_quant_forward takes, beyond
# p4v_attn_quant_forward's envelope, a qkv layer with n_H = n_a = 1 that is no post-GELU layer and whose out_features are 3 * C.
# Same saved-forward attribute as fuse_attention: the two patch the same containers and cannot stack.
def qkv_attention_fusable(m):
    """The static half of the decision: an Attention container whose forward `fuse_qkv_attention` patches."""
    return attention_fusable(m) and isinstance(m.qkv, PTQSLQuantLinear)


def _qkv_attn_args(m, x):
    """(qkv's, matmul1's, matmul2's engine keywords) if the patched forward of `m` runs the qkv-fused chain on `x`, else None."""
    if not qkv_attention_fusable(m):
        return None
    args = _attn_args(m, x)
    if args is None:
        return None
    qkv = m.qkv
    if not (_live(qkv) and qkv._int8_ready(x)) or x.shape[-1] != qkv.in_features or qkv.out_features != 3 * x.shape[-1]:
        return None
    lin = qkv._int8_args()
    if lin["postgelu"] or lin["n_H"] != 1 or lin["n_a"] != 1:
        return None
    return (lin,) + args


def takes_fused_qkv_attention_path(m, x):
    """The per-call half: would the patched forward of `m` run the qkv-fused kernel chain on `x`?"""
    return _qkv_attn_args(m, x) is not None


def _fused_qkv_attention_forward(self, x):
    args = _qkv_attn_args(self, x)
    if args is None:
        return _fused_attention_forward(self, x)      # (fuse_attention's path where its conditions hold, else the original)
    # models.Attention.forward, with qkv ... matmul2 as one engine call
    B, N, C = x.shape
    out = engine.qkv_attn_quant_forward(x=x, qkv=args[0], scale=self.scale, qk=args[1], pv=args[2])
    return self.proj_drop(self.proj(out.transpose(1, 2).reshape(B, N, C)))


def fuse_qkv_attention(net):
    """Patch the forward of every Attention container of `net` that fuse_attention would patch and whose qkv is a PTQSL Linear
    layer; returns their names.  Idempotent.  On a container fuse_attention patched it replaces that forward."""
    return _patch(net, qkv_attention_fusable, _ORIG_ATTN, _fused_qkv_attention_forward, replace=True)


# ---- window attention (Swin): matmul1 -> + bias -> + mask -> softmax -> matmul2 (engine.window_attn_quant_forward) ----
_ORIG_WATTN = "_p4v_unfused_wattn_forward"


def window_attention_fusable(m):
    """The static half of the decision: a WindowAttention container whose forward `fuse_window_attention` patches."""
    return (isinstance(m, models.WindowAttention) and isinstance(m.matmul1, PTQSLQuantMatMul) and isinstance(m.matmul2, PTQSLQuantMatMul)
            and _inactive_dropout(m.attn_drop))


def _wattn_args(m, x, mask):
    """_attn_args for a WindowAttention, with the condition on the mask: None, or float32 [nW][N][N] where x lies, B_ % nW == 0."""
    args = _attn_args(m, x, window_attention_fusable)
    if args is None or _hooked(m.softmax) or (torch.is_grad_enabled() and m.relative_position_bias_table.requires_grad):
        return None
    if mask is not None:
        N = x.shape[1]
        if not (torch.is_tensor(mask) and mask.dtype == torch.float32 and mask.device == x.device and not mask.requires_grad
                and mask.dim() == 3 and tuple(mask.shape[1:]) == (N, N) and mask.shape[0] >= 1 and x.shape[0] % mask.shape[0] == 0):
            return None
    return args


def takes_fused_window_attention_path(m, x, mask=None):
    """The per-call half: would the patched forward of `m` run the fused kernel chain on `x` (and `mask`)?"""
    return _wattn_args(m, x, mask) is not None


def _fused_window_attention_forward(self, x, mask=None):
    args = _wattn_args(self, x, mask)
    if args is None:
        return self.__dict__[_ORIG_WATTN](x, mask)
    # models.WindowAttention.forward, with matmul1 ... matmul2 as one engine call
    B_, N, C = x.shape
    H = self.num_heads
    qkv = self.qkv(x).reshape(B_, N, 3, H, C // H).permute(2, 0, 3, 1, 4)
    q, k, v = qkv.unbind(0)
    q = q * self.scale
    n = self.window_size[0] * self.window_size[1]
    bias = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(n, n, -1)
    out = engine.window_attn_quant_forward(q=q, kT=k.transpose(-2, -1), v=v, bias=bias.permute(2, 0, 1).contiguous(), mask=mask,
                                           qk=args[0], pv=args[1])
    return self.proj_drop(self.proj(out.transpose(1, 2).reshape(B_, N, C)))


def fuse_window_attention(net):
    """Patch the forward of every fusable WindowAttention container of `net`; returns their names.  Idempotent."""
    return _patch(net, window_attention_fusable, _ORIG_WATTN, _fused_window_attention_forward)


def unfuse_window_attention(net):
    """Undo fuse_window_attention: every patched container gets its original forward back; returns their names.  Idempotent."""
    return _unfuse(net, _ORIG_WATTN)
