"""MatMul operands in the memory layouts a network hands them over in, for tests/test_matmul_layouts_cpu.py and
tests/test_hip_matmul_layouts.py.

`layouts(x, role)` returns {name: view} for a canonical [b][H][R][C] fp32 tensor `x`; `role` is "A" (the row operand
[b][H][M][K]), "B_qk" (k^T, [b][H][D][T]) or "B_sv" (v, [b][H][T][D]).  Every view

  * holds the values of `x` (torch.equal(view, x); `batch_broadcast` holds those of `canonical_of(x, name)`),
  * lies in the interior of ONE allocation of its own (`allocation(view)`), behind and in front of a margin of at least
    3 x the extent of the buffer the view is cut from,
  * is surrounded by NaN: every float of the allocation that is no element of the view -- the gaps between padded rows, the
    sibling q / k / v slices of a packed buffer, the margins -- is NaN.  A read through a wrong stride or past a row end lands
    in mapped memory and shows in the result.

The layouts (strides for x [b][H][R][C]):
  contiguous           dense, base 16-byte aligned
  transposed           the last two axes swapped in memory: strides (H R C, R C, 1, R).  The production layout of B_qk
                       (k.transpose(-2, -1) of a contiguous k) and its canonical one.
  packed_qkv_{0,1,2}   slice s of a [b][R][3][H][C] buffer permuted as Attention.forward does: (3 R H C, C, 3 H C, 1)
  packed_qkv_{s}_T     B_qk only: k^T of the packed k -- slice s of a [b][C][3][H][R] buffer, permuted, last axes transposed:
                       (3 C H R, R, 1, 3 H R)
  packed_qkv_offset1   the role's own slice (A: q = 0, B_qk: k^T = 1_T, B_sv: v = 2), the buffer starting one float into the
                       allocation: base 4-byte aligned only
  row_pad1, row_pad4   row stride C + 1 (rows unaligned) and C + 4 (rows aligned, not dense)
  offset1              dense, base one float off a 16-byte boundary
  head_major           stored [H][b][R][C]: stride[0] < stride[1]
  batch_broadcast      x[:1].expand(b, ...): stride[0] = 0
  window_packed        WindowAttention.forward: B_ = images * windows on the batch axis.  A is q * scale, an elementwise
                       result that keeps the memory order of the packed slice, [B_][R][H][C]: (R H C, C, H C, 1); B_qk and B_sv
                       are the k^T and v slices of the [B_][T][3][H][D] buffer.

`packed_qkv_views(q, k, v)` places q, k^T and v in ONE packed buffer, as the network hands a MatMul pair over.
"""
import math

import torch

ROLES = ("A", "B_qk", "B_sv")
MARGIN_FACTOR = 3
ROLE_SLOT = {"A": 0, "B_qk": 1, "B_sv": 2}


def _embed(shape, pick, lead=0, dtype=torch.float32):
    """`pick(buf)` of a dense buffer `buf` of `shape`, `lead` floats behind a 16-byte aligned position of a NaN-filled
    allocation with margins of MARGIN_FACTOR x the buffer on both sides (rounded up to 4 floats)."""
    n = math.prod(shape)
    margin = (MARGIN_FACTOR * n + 3) // 4 * 4
    alloc = torch.full((margin + lead + n + margin,), float("nan"), dtype=dtype)
    assert alloc.data_ptr() % 16 == 0, "the allocator hands out 16-byte aligned memory"
    return pick(alloc[margin + lead: margin + lead + n].view(shape))


def _filled(x, shape, pick, lead=0):
    view = _embed(shape, pick, lead, x.dtype)
    (view if view.stride(0) else view[:1]).copy_(x if view.stride(0) else x[:1])      # (a broadcast batch is stored once)
    return view


def _packed(s, transposed):
    if transposed:
        return lambda buf: buf[:, :, s].permute(0, 2, 1, 3).transpose(-2, -1)
    return lambda buf: buf[:, :, s].permute(0, 2, 1, 3)


def _packed_shape(x, transposed):
    b, H, R, C = x.shape
    return (b, C, 3, H, R) if transposed else (b, R, 3, H, C)


def layouts(x, role):
    """{name: view} of the canonical [b][H][R][C] tensor `x` (on the CPU; `to_device` moves a view with its allocation)."""
    assert role in ROLES and x.dim() == 4 and x.dtype == torch.float32 and x.device.type == "cpu"
    b, H, R, C = x.shape
    out = {}
    out["contiguous"] = _filled(x, (b, H, R, C), lambda buf: buf)
    out["transposed"] = _filled(x, (b, H, C, R), lambda buf: buf.transpose(-2, -1))
    for s in range(3):
        out[f"packed_qkv_{s}"] = _filled(x, _packed_shape(x, False), _packed(s, False))
        if role == "B_qk":
            out[f"packed_qkv_{s}_T"] = _filled(x, _packed_shape(x, True), _packed(s, True))
    own_T = role == "B_qk"
    out["packed_qkv_offset1"] = _filled(x, _packed_shape(x, own_T), _packed(ROLE_SLOT[role], own_T), lead=1)
    out["row_pad1"] = _filled(x, (b, H, R, C + 1), lambda buf: buf[..., :C])
    out["row_pad4"] = _filled(x, (b, H, R, C + 4), lambda buf: buf[..., :C])
    out["offset1"] = _filled(x, (b, H, R, C), lambda buf: buf, lead=1)
    out["head_major"] = _filled(x, (H, b, R, C), lambda buf: buf.permute(1, 0, 2, 3))
    out["batch_broadcast"] = _filled(x, (1, H, R, C), lambda buf: buf.expand(b, H, R, C))
    if role == "A":
        out["window_packed"] = _filled(x, (b, R, H, C), lambda buf: buf.permute(0, 2, 1, 3))
    else:
        out["window_packed"] = _filled(x, _packed_shape(x, own_T), _packed(ROLE_SLOT[role], own_T))
    return out


def canonical_name(role):
    return "transposed" if role == "B_qk" else "contiguous"


def canonical_of(x, name):
    """The tensor whose values the layout `name` of `x` holds: `x`, for batch_broadcast the materialised expansion of x[:1]."""
    return x[:1].expand_as(x).contiguous() if name == "batch_broadcast" else x


def packed_qkv_views(q, k, v, lead=0):
    """(q, k^T, v) as Attention.forward hands them to matmul1 / matmul2: views of ONE [b][T][3][H][D] buffer (q, k, v: [b][H][T][D]
    each, any of them None: that slice stays NaN and None is returned for it)."""
    ref = next(t for t in (q, k, v) if t is not None)
    b, H, T, D = ref.shape
    buf = _embed((b, T, 3, H, D), lambda buf: buf, lead, ref.dtype)
    views = []
    for s, t in enumerate((q, k, v)):
        if t is None:
            views.append(None)
            continue
        assert t.shape == ref.shape
        view = buf[:, :, s].permute(0, 2, 1, 3)
        view.copy_(t)
        views.append(view.transpose(-2, -1) if s == 1 else view)
    return tuple(views)


def allocation(view):
    """The whole allocation behind `view` as a flat tensor of its dtype."""
    return torch.empty(0, dtype=view.dtype, device=view.device).set_(view.untyped_storage())


def extent(view):
    """Floats between the first and the last element of `view`, both included."""
    return 1 + sum((n - 1) * s for n, s in zip(view.shape, view.stride()))


def element_mask(view):
    """bool [allocation]: True at the floats that are elements of `view`."""
    mask = torch.zeros(allocation(view).numel(), dtype=torch.bool, device=view.device)
    mask.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(True)
    return mask


def to_device(view, device, moved=None):
    """The same view of a copy of the WHOLE allocation on `device`: strides, offset within the allocation, NaN surroundings.
    `moved`: a dict shared by the calls for views of ONE allocation, which then stay views of one copy."""
    if view is None:
        return None
    key = view.untyped_storage().data_ptr()
    alloc = moved.get(key) if moved is not None else None
    if alloc is None:
        alloc = allocation(view).to(device, copy=True)
        if moved is not None:
            moved[key] = alloc
    assert alloc.data_ptr() % 16 == 0
    return alloc.as_strided(view.shape, view.stride(), view.storage_offset())


def base_alignment(view):
    """Largest power of two up to 16 that divides the address of the view's first element."""
    p = view.data_ptr()
    return next(a for a in (16, 8, 4, 2, 1) if p % a == 0)
