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
`fuse_window_attention(net, one_kernel=True)` asks for the one-kernel window core (k_wattn_qkpv): same bits.

`fuse_qkv_attention(net)` / `takes_fused_qkv_attention_path(m, x)` take the qkv layer of a `models.Attention` into the chain
(engine.qkv_attn_quant_forward / p4v_qkv_attn_quant_forward): qkv's GEMM writes the int8 operand planes of
the two MatMuls.  It shares fuse_attention's saved forward -- the two do not stack, the later call decides which forward is
installed, unfuse_attention undoes either -- and its patched forward decides per call: the qkv-fused path when fuse_attention's
conditions hold and qkv is calibrated, in quant_forward, on the int8 path, unhooked, n_H = n_a = 1, no post-GELU layer, 3 * C
wide; otherwise fuse_attention's path where its conditions hold; otherwise the original forward.

`fuse_norm(net, residual=True, proj_plane=True)`: on blocks whose attention container asked for its one-kernel
core, proj travels into the container's core call (engine.attn_quant_forward / window_attn_quant_forward with proj=, residual=) and
the core's epilogue writes proj's int8 row plane -- no fp32 attention output, no head-merging transpose copy, no pack of it in
front of proj.  Without `residual`, or on a container that did not ask for one kernel, the flag changes nothing; the net returns
the same bits either way.
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
_ONE_KERNEL = "_p4v_attn_one_kernel"      # the patched container's choice: the attention core as one kernel


def _choose_kernel(net, names, one_kernel):
    for name, m in net.named_modules():
        if name in names:
            m.__dict__[_ONE_KERNEL] = bool(one_kernel)
    return names


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
    return _attention_tail(self, self.qkv(x), args)


def _attention_tail(self, qkv_out, args):
    """models.Attention.forward behind `self.qkv(x)`, with matmul1 ... matmul2 as one engine call (`qkv_out` [B][N][3 C])"""
    return self.proj_drop(self.proj(_attention_core(self, qkv_out, args)))


def _attention_core(self, qkv_out, args, proj=None, residual=None):
    """... up to proj's input [B][N][C]: proj is the caller's.  `proj` (its engine keywords, with the block's `residual`): the engine
    call runs proj behind the core and returns residual + proj's output (fuse_norm(proj_plane=True))"""
    B, N, C = qkv_out.shape[0], qkv_out.shape[1], qkv_out.shape[2] // 3
    H = self.num_heads
    qkv = qkv_out.reshape(B, N, 3, H, C // H).permute(2, 0, 3, 1, 4)
    if os.environ.get("P4V_QKV_CONTIGUOUS", "1") == "1":
        qkv = qkv.contiguous()
    q, k, v = qkv.unbind(0)
    one = self.__dict__.get(_ONE_KERNEL, False)
    if proj is not None:
        return engine.attn_quant_forward(q=q, kT=k.transpose(-2, -1), v=v, scale=self.scale, qk=args[0], pv=args[1], one_kernel=one, proj=proj,
                                         residual=residual)
    out = engine.attn_quant_forward(q=q, kT=k.transpose(-2, -1), v=v, scale=self.scale, qk=args[0], pv=args[1], one_kernel=one)
    return out.transpose(1, 2).reshape(B, N, C)


def fuse_attention(net, one_kernel=False):
    """Patch the forward of every fusable Attention container of `net`; returns their names.  Idempotent.  On a container
    fuse_qkv_attention patched it replaces that forward (the two share the saved forward: the later call decides).
    `one_kernel`: the patched containers ask the engine for the one-kernel attention core (stored on them; the later call
    decides here too).  It changes neither when the fused path is taken nor what it returns."""
    return _choose_kernel(net, _patch(net, attention_fusable, _ORIG_ATTN, _fused_attention_forward, replace=True), one_kernel)


def unfuse_attention(net):
    """Undo fuse_attention or fuse_qkv_attention: every patched container gets its original forward back; returns their names.
    Idempotent."""
    for m in net.modules():
        m.__dict__.pop(_ONE_KERNEL, None)
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
    out = engine.qkv_attn_quant_forward(x=x, qkv=args[0], scale=self.scale, qk=args[1], pv=args[2],
                                        one_kernel=self.__dict__.get(_ONE_KERNEL, False))
    return self.proj_drop(self.proj(out.transpose(1, 2).reshape(B, N, C)))


def fuse_qkv_attention(net, one_kernel=False):
    """Patch the forward of every Attention container of `net` that fuse_attention would patch and whose qkv is a PTQSL Linear
    layer; returns their names.  Idempotent.  On a container fuse_attention patched it replaces that forward.  `one_kernel`: as
    in fuse_attention."""
    return _choose_kernel(net, _patch(net, qkv_attention_fusable, _ORIG_ATTN, _fused_qkv_attention_forward, replace=True), one_kernel)


# ---- window attention (Swin): matmul1 -> + bias -> + mask -> softmax -> matmul2 (engine.window_attn_quant_forward) ----
_ORIG_WATTN = "_p4v_unfused_wattn_forward"
_WONE_KERNEL = "_p4v_wattn_one_kernel"    # the patched container's choice: the window core as one kernel


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
    return _window_attention_tail(self, self.qkv(x), args, mask)


def _window_attention_tail(self, qkv_out, args, mask):
    """models.WindowAttention.forward behind `self.qkv(x)`, with matmul1 ... matmul2 as one engine call (`qkv_out` [B_][N][3 C])"""
    return self.proj_drop(self.proj(_window_attention_core(self, qkv_out, args, mask)))


def _window_attention_core(self, qkv_out, args, mask, proj=None, residual=None, window=None):
    """... up to proj's input [B_][N][C]: proj is the caller's.  `proj` (its engine keywords, with the block's `residual` and the
    `window` map): the engine call runs proj behind the core and returns residual + proj's output in token order
    (fuse_norm(proj_plane=True))"""
    B_, N, C = qkv_out.shape[0], qkv_out.shape[1], qkv_out.shape[2] // 3
    H = self.num_heads
    qkv = qkv_out.reshape(B_, N, 3, H, C // H).permute(2, 0, 3, 1, 4)
    q, k, v = qkv.unbind(0)
    q = q * self.scale
    n = self.window_size[0] * self.window_size[1]
    bias = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(n, n, -1)
    one = self.__dict__.get(_WONE_KERNEL, False)
    if proj is not None:
        return engine.window_attn_quant_forward(q=q, kT=k.transpose(-2, -1), v=v, bias=bias.permute(2, 0, 1).contiguous(), mask=mask,
                                                qk=args[0], pv=args[1], one_kernel=one, proj=proj, residual=residual, window=window)
    out = engine.window_attn_quant_forward(q=q, kT=k.transpose(-2, -1), v=v, bias=bias.permute(2, 0, 1).contiguous(), mask=mask,
                                           qk=args[0], pv=args[1], one_kernel=one)
    return out.transpose(1, 2).reshape(B_, N, C)


def fuse_window_attention(net, one_kernel=False):
    """Patch the forward of every fusable WindowAttention container of `net`; returns their names.  Idempotent.  `one_kernel`:
    the patched containers ask the engine for the one-kernel window core (stored on them; the later call decides).  It changes
    neither when the fused path is taken nor what it returns."""
    names = _patch(net, window_attention_fusable, _ORIG_WATTN, _fused_window_attention_forward)
    for name, m in net.named_modules():
        if name in names:
            m.__dict__[_WONE_KERNEL] = bool(one_kernel)
    return names


def unfuse_window_attention(net):
    """Undo fuse_window_attention: every patched container gets its original forward back; returns their names.  Idempotent."""
    for m in net.modules():
        m.__dict__.pop(_WONE_KERNEL, None)
    return _unfuse(net, _ORIG_WATTN)


# ---- LayerNorm in front of qkv and of the MLP (engine.linear_quant_forward / mlp_quant_forward with ln=) -----------
# fuse_norm patches the BLOCKS (models.Block, models.SwinBlock): the patched forward repeats the block's own and decides per side
# and per call.  norm2 side: the MLP container carries fuse_mlp's patch and would take its fused path, norm2 is an affine
# nn.LayerNorm over the last dimension, unhooked, not recording, inside the kernel's envelope -> engine.mlp_quant_forward(ln=) on the
# residual stream.  norm1 side: the attention container carries fuse_window_attention's (Swin) / fuse_attention's (ViT) patch and
# would take its fused path, qkv is live on its int8 path with n_H = n_a = 1 and no post-GELU input -> engine.linear_quant_forward(ln=)
# writes qkv's output (Swin: in window order -- the roll and window_partition are the kernel's row map) and the container's
# fused forward goes on behind `self.qkv(x)`.  A ViT container patched by fuse_qkv_attention keeps norm1 in torch.  Every other
# state runs the side as the block's own forward does.  Its own saved-forward attribute: composes with the other fuse_* in any order.
_ORIG_NORM = "_p4v_unfused_norm_forward"
_RESIDUAL = "_p4v_fuse_residual"          # the patched block's choice: proj / fc2 add the residual in their GEMM epilogue
_PROJ_PLANE = "_p4v_fuse_proj_plane"      # ... and the one-kernel attention core writes proj's int8 row plane


def _proj_plane(block):
    """the patched block hands proj to its container's core call: the flag is set and the container asked for the one-kernel core"""
    one = _WONE_KERNEL if isinstance(block, models.SwinBlock) else _ONE_KERNEL
    return block.__dict__.get(_PROJ_PLANE, False) and block.attn.__dict__.get(one, False)


def norm_fusable(m):
    """The static half of the decision: a block whose forward `fuse_norm` patches."""
    return isinstance(m, (models.Block, models.SwinBlock))


def _norm_ok(norm, x):
    return (isinstance(norm, nn.LayerNorm) and norm.elementwise_affine and norm.bias is not None and torch.is_tensor(x) and x.is_cuda
            and x.dtype == torch.float32 and x.dim() == 3 and tuple(norm.normalized_shape) == (x.shape[-1],) and not _hooked(norm)
            and not _recording(x, norm) and x.shape[-1] % 4 == 0 and x.shape[-1] <= 2048)


def _ln_of(norm):
    return dict(weight=norm.weight, bias=norm.bias, eps=norm.eps)


def _installed(m):
    return getattr(m.__dict__.get("forward"), "__func__", None)


def _container_args(block, x):
    """(the attention container's input -- its shape is all that is asked about --, its (matmul1, matmul2) keywords) if the container
    carries our fused forward and would take it on the block's input `x`, else (None, None)."""
    attn = getattr(block, "attn", None)
    if attn is None or _hooked(attn) or not (torch.is_tensor(x) and x.dim() == 3):
        return None, None
    if isinstance(block, models.SwinBlock):
        (H, W), ws = block.input_resolution, block.window_size
        if _installed(attn) is not _fused_window_attention_forward or x.shape[1] != H * W or H % ws or W % ws or not 0 <= block.shift_size < ws:
            return None, None
        xin = x.reshape(-1, ws * ws, x.shape[2])
        return xin, _wattn_args(attn, xin, block.attn_mask)
    if _installed(attn) is not _fused_attention_forward:
        return None, None
    return x, _attn_args(attn, x)


def _proj_res_args(block, x):
    """(proj's engine keywords, the container's (matmul1, matmul2) keywords) if the patched forward of `block` lets proj add the
    residual on `x` (fuse_norm(net, residual=True)), else None: the container carries our fused forward and would
    take it; proj is live on its int8 path with n_H = n_a = 1, unhooked, no post-GELU layer, C -> C with C % 4 == 0; proj_drop is
    inactive and unhooked."""
    if not block.__dict__.get(_RESIDUAL, False) or not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32):
        return None
    xin, args = _container_args(block, x)
    if args is None:
        return None
    attn = block.attn
    proj, C = attn.proj, x.shape[-1]
    if not (isinstance(proj, PTQSLQuantLinear) and _live(proj) and proj._int8_ready(xin)) or _recording(x, proj):
        return None
    if not _inactive_dropout(attn.proj_drop) or _hooked(attn.proj_drop) or C % 4 or proj.in_features != C or proj.out_features != C:
        return None
    lin = proj._int8_args()
    if lin["postgelu"] or lin["n_H"] != 1 or lin["n_a"] != 1:
        return None
    return lin, args


def _norm1_args(block, x):
    """(qkv's engine keywords, the container's (matmul1, matmul2) keywords) if the patched forward of `block` fuses norm1 into
    qkv's quantiser on `x`, else None."""
    attn = getattr(block, "attn", None)
    if attn is None or not _norm_ok(block.norm1, x):
        return None
    xin, args = _container_args(block, x)
    qkv = attn.qkv
    if args is None or not (isinstance(qkv, PTQSLQuantLinear) and _live(qkv) and qkv._int8_ready(xin)):
        return None
    lin = qkv._int8_args()
    if lin["postgelu"] or lin["n_H"] != 1 or lin["n_a"] != 1 or qkv.in_features != x.shape[-1] or qkv.out_features != 3 * x.shape[-1]:
        return None
    return lin, args


def _norm2_args(block, x):
    """(fc1's, fc2's engine keywords) if the patched forward of `block` fuses norm2 into fc1's quantiser on `x`, else None."""
    mlp = getattr(block, "mlp", None)
    if mlp is None or _ORIG not in mlp.__dict__ or _hooked(mlp) or not _norm_ok(block.norm2, x):
        return None
    return _mlp_args(mlp, x)


def takes_fused_norm_path(block, x, side=None):
    """The per-call half: would the patched forward of `block` fuse the LayerNorm of `side` ("norm1" / "norm2"; None: of both
    sides) on `x`?"""
    if not norm_fusable(block):
        return False
    sides = {"norm1": _norm1_args, "norm2": _norm2_args}
    return all(sides[s](block, x) is not None for s in ([side] if side else sides))


def _mlp_side(self, x):
    """x + mlp(norm2(x)), the block's second half"""
    res = self.__dict__.get(_RESIDUAL, False) and x.shape[-1] % 4 == 0
    args = _norm2_args(self, x)
    if args is not None:
        if res:
            return engine.mlp_quant_forward(x=x, ln=_ln_of(self.norm2), fc1=args[0], fc2=args[1], residual=x.contiguous())
        return x + engine.mlp_quant_forward(x=x, ln=_ln_of(self.norm2), fc1=args[0], fc2=args[1])
    mlp = getattr(self, "mlp", None)
    if res and mlp is not None and _ORIG in mlp.__dict__ and not _hooked(mlp) and x.is_cuda and x.dtype == torch.float32:
        y = self.norm2(x)
        args = _mlp_args(mlp, y)
        if args is not None:
            return engine.mlp_quant_forward(x=y, fc1=args[0], fc2=args[1], residual=x.contiguous())
        return x + mlp(y)
    return x + self.mlp(self.norm2(x))


def _fused_norm_block_forward(self, x):
    # models.Block.forward
    a, p = _norm1_args(self, x), _proj_res_args(self, x)
    if p is not None:
        qkv = engine.linear_quant_forward(x=x, ln=_ln_of(self.norm1), **a[0]) if a is not None else self.attn.qkv(self.norm1(x))
        if _proj_plane(self):
            x = _attention_core(self.attn, qkv, p[1], proj=p[0], residual=x.contiguous())
        else:
            x = engine.linear_quant_forward(x=_attention_core(self.attn, qkv, p[1]), residual=x.contiguous(), **p[0])
    elif a is None:
        x = x + self.attn(self.norm1(x))
    else:
        x = x + _attention_tail(self.attn, engine.linear_quant_forward(x=x, ln=_ln_of(self.norm1), **a[0]), a[1])
    return _mlp_side(self, x)


def _fused_norm_swin_block_forward(self, x):
    # models.SwinBlock.forward
    H, W = self.input_resolution
    B, L, C = x.shape
    shortcut = x
    ws = self.window_size
    a, p = _norm1_args(self, x), _proj_res_args(self, x)
    if a is None:
        x = self.norm1(x).view(B, H, W, C)
        if self.shift_size > 0:
            x = torch.roll(x, shifts=(-self.shift_size, -self.shift_size), dims=(1, 2))
        xw = models.window_partition(x, ws).view(-1, ws * ws, C)
        qkv = self.attn.qkv(xw) if p is not None else None
    else:
        qkv = engine.linear_quant_forward(x=x, ln=_ln_of(self.norm1), window=(H, W, ws, self.shift_size), **a[0])
        qkv = qkv.view(-1, ws * ws, qkv.shape[-1])
    if p is not None:
        # proj scatters its rows through window_reverse + roll(+shift) and adds the shortcut: k_lin_res's row map
        if _proj_plane(self):
            x = _window_attention_core(self.attn, qkv, p[1], self.attn_mask, proj=p[0], residual=shortcut.contiguous(),
                                       window=(H, W, ws, self.shift_size))
            return _mlp_side(self, x)
        core = _window_attention_core(self.attn, qkv, p[1], self.attn_mask)
        x = engine.linear_quant_forward(x=core, residual=shortcut.contiguous(), window=(H, W, ws, self.shift_size), **p[0])
        return _mlp_side(self, x)
    if a is None:
        aw = self.attn(xw, mask=self.attn_mask).view(-1, ws, ws, C)
    else:
        aw = _window_attention_tail(self.attn, qkv, a[1], self.attn_mask).view(-1, ws, ws, C)
    x = models.window_reverse(aw, ws, H, W)
    if self.shift_size > 0:
        x = torch.roll(x, shifts=(self.shift_size, self.shift_size), dims=(1, 2))
    x = shortcut + x.view(B, H * W, C)
    return _mlp_side(self, x)


def fuse_norm(net, residual=False, proj_plane=False):
    """Patch the forward of every Block / SwinBlock of `net`; returns their names.  Idempotent.  What a side fuses is decided per
    call (see above): without fuse_mlp / fuse_window_attention / fuse_attention on the block's containers nothing changes.
    `residual`: the patched blocks also let proj and fc2 add the residual -- and, on Swin, proj scatter its rows through
    window_reverse and the back-roll -- in their GEMM epilogue (engine.linear_quant_forward / mlp_quant_forward with residual=,
    DESIGN.md s5.15), per side and per call, whether or not that side's LayerNorm fused: the attention side where the container
    carries our fused forward and would take it, proj is live on its int8 path with n_H = n_a = 1, unhooked, proj_drop inactive and
    C % 4 == 0; the MLP side where the fused MLP chain would run.  Every other state runs the side as before.  The flag is stored
    on the blocks (the later call decides) and changes no bit of what the net returns.
    `proj_plane` (with `residual`): where proj adds the residual AND the block's attention container asked for its one-kernel core
    (fuse_attention / fuse_window_attention with one_kernel=True), proj travels into the container's core call
    (engine.attn_quant_forward / window_attn_quant_forward with proj=, residual=): the core's epilogue writes proj's
    int8 row plane -- no fp32 attention output, no transpose copy, no pack of it.  Stored on the blocks like `residual`; the same bits."""
    names = _patch(net, lambda m: isinstance(m, models.SwinBlock), _ORIG_NORM, _fused_norm_swin_block_forward)
    names = sorted(names + _patch(net, lambda m: isinstance(m, models.Block), _ORIG_NORM, _fused_norm_block_forward))
    for name, m in net.named_modules():
        if name in names:
            m.__dict__[_RESIDUAL] = bool(residual)
            m.__dict__[_PROJ_PLANE] = bool(residual and proj_plane)
    return names


def unfuse_norm(net):
    """Undo fuse_norm: every patched block gets its original forward back; returns their names.  Idempotent."""
    for m in net.modules():
        m.__dict__.pop(_RESIDUAL, None)
        m.__dict__.pop(_PROJ_PLANE, None)
    return _unfuse(net, _ORIG_NORM)
