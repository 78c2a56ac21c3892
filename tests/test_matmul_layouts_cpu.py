"""The layout builders of tests/matmul_layouts.py (no GPU needed): every view holds the canonical values, has the strides and the
base alignment its name states -- a refactor cannot quietly turn a layout back into a dense one --, lies inside one allocation
behind its margins, and everything around it is NaN.  And the MatMul module classes on the CPU (fake-quant path): a packed
view gives the output of its copy."""
import pytest
import torch

from tests import matmul_layouts as ml

b, H, T, D = 2, 3, 49, 32
HD = H * D


def _x(role, shape=(b, H, T, D)):
    b_, H_, T_, D_ = shape
    g = torch.Generator().manual_seed(30 + ml.ROLES.index(role))
    return torch.randn((b_, H_, D_, T_) if role == "B_qk" else (b_, H_, T_, D_), generator=g)


# strides of x [b][H][R][C]; R, C = T, D for A and B_sv, = D, T for B_qk; (strides, base alignment in bytes)
def _expected(role):
    R, C = (D, T) if role == "B_qk" else (T, D)
    packed = (3 * R * H * C, C, 3 * H * C, 1)
    packed_T = (3 * C * H * R, R, 1, 3 * H * R)
    own = packed_T if role == "B_qk" else packed
    exp = {"contiguous": ((H * R * C, R * C, C, 1), 16),
           "transposed": ((H * R * C, R * C, 1, R), 16),
           "packed_qkv_0": (packed, 16), "packed_qkv_1": (packed, None), "packed_qkv_2": (packed, None),
           "packed_qkv_offset1": (own, 4),
           "row_pad1": ((H * R * (C + 1), R * (C + 1), C + 1, 1), 16),
           "row_pad4": ((H * R * (C + 4), R * (C + 4), C + 4, 1), 16),
           "offset1": ((H * R * C, R * C, C, 1), 4),
           "head_major": ((R * C, b * R * C, C, 1), 16),
           "batch_broadcast": ((0, R * C, C, 1), 16),
           "window_packed": ((R * H * C, C, H * C, 1) if role == "A" else own, None)}
    if role == "B_qk":
        exp.update({f"packed_qkv_{s}_T": (packed_T, 16 if s == 0 else None) for s in range(3)})
    return exp


@pytest.mark.parametrize("role", ml.ROLES)
def test_every_layout_states_its_strides_and_holds_the_canonical_values(role):
    x = _x(role)
    views = ml.layouts(x, role)
    exp = _expected(role)
    assert set(views) == set(exp)
    assert ml.canonical_name(role) in views
    for name, v in views.items():
        strides, align = exp[name]
        assert v.shape == x.shape and v.dtype == torch.float32
        assert torch.equal(v, ml.canonical_of(x, name)), f"{role} {name}: values differ"
        assert tuple(v.stride()) == strides, f"{role} {name}: strides {tuple(v.stride())}, stated {strides}"
        if align is not None:
            assert ml.base_alignment(v) == align, f"{role} {name}: base aligned to {ml.base_alignment(v)} bytes, stated {align}"
        assert ml.base_alignment(v) >= 4
    assert not torch.equal(views["batch_broadcast"], x), "the canonical tensor has different images"
    # a layout that is dense and aligned is one of the two the suite always ran
    dense = [n for n, v in views.items() if v.is_contiguous() and ml.base_alignment(v) == 16]
    assert dense == ["contiguous"], dense


def test_the_strides_the_issue_states():
    A = ml.layouts(_x("A"), "A")
    assert tuple(A["packed_qkv_0"].stride()) == (14112, 32, 288, 1)
    assert tuple(A["head_major"].stride()) == (1568, 3136, 32, 1)
    assert tuple(A["batch_broadcast"].stride()) == (0, 1568, 32, 1)
    assert tuple(A["row_pad1"].stride()) == (4851, 1617, 33, 1)
    kT = ml.layouts(_x("B_qk"), "B_qk")
    assert tuple(kT["packed_qkv_1_T"].stride()) == (14112, 32, 1, 288)
    assert tuple(kT["transposed"].stride()) == (4704, 1568, 1, 32)            # k.transpose(-2, -1) of a contiguous k


@pytest.mark.parametrize("role", ml.ROLES)
def test_everything_around_a_view_is_nan(role):
    x = _x(role)
    for name, v in ml.layouts(x, role).items():
        alloc, mask = ml.allocation(v), ml.element_mask(v)
        elements = x.numel() // (b if name == "batch_broadcast" else 1)
        assert int(mask.sum()) == elements, f"{role} {name}: the view addresses {int(mask.sum())} floats"
        assert int(torch.isnan(alloc).sum()) == alloc.numel() - elements, f"{role} {name}: NaN count"
        assert bool(torch.isnan(alloc[~mask]).all()) and not bool(torch.isnan(alloc[mask]).any())
        first = v.storage_offset()
        last = first + ml.extent(v) - 1
        margin = ml.MARGIN_FACTOR * ml.extent(v)
        assert first >= margin and alloc.numel() - 1 - last >= margin, f"{role} {name}: margins {first}, {alloc.numel() - 1 - last} < {margin}"


def test_a_view_moves_with_its_allocation():
    x = _x("B_qk")
    for name, v in ml.layouts(x, "B_qk").items():
        w = ml.to_device(v, "cpu")
        assert w.data_ptr() != v.data_ptr() and tuple(w.stride()) == tuple(v.stride()) and w.storage_offset() == v.storage_offset()
        assert torch.equal(w, v) and ml.allocation(w).numel() == ml.allocation(v).numel()
        assert ml.base_alignment(w) == ml.base_alignment(v), name
        assert torch.equal(ml.element_mask(w), ml.element_mask(v))


def test_q_kT_v_of_one_packed_buffer():
    g = torch.Generator().manual_seed(33)
    q, k, v = (torch.randn(b, H, T, D, generator=g) for _ in range(3))
    qv, kTv, vv = ml.packed_qkv_views(q, k, v)
    assert torch.equal(qv, q) and torch.equal(kTv, k.transpose(-2, -1)) and torch.equal(vv, v)
    assert tuple(qv.stride()) == tuple(vv.stride()) == (T * 3 * HD, D, 3 * HD, 1) and tuple(kTv.stride()) == (T * 3 * HD, D, 1, 3 * HD)
    assert qv.untyped_storage().data_ptr() == kTv.untyped_storage().data_ptr() == vv.untyped_storage().data_ptr()
    assert (kTv.storage_offset() - qv.storage_offset(), vv.storage_offset() - qv.storage_offset()) == (HD, 2 * HD)
    alloc = ml.allocation(qv)
    assert int(torch.isnan(alloc).sum()) == alloc.numel() - 3 * q.numel()
    qv, kTv, vv = ml.packed_qkv_views(q, k, None, lead=1)
    assert vv is None and ml.base_alignment(qv) == 4
    alloc = ml.allocation(qv)
    assert int(torch.isnan(alloc).sum()) == alloc.numel() - 2 * q.numel(), "the v slice of a q / k pair stays NaN"
    assert int((ml.element_mask(qv) | ml.element_mask(kTv)).sum()) == 2 * q.numel()


# ---- the module classes on the CPU: a packed view against its copy --------------------------------------------------------------
def _headwise(x, qmax):
    return (x.abs().amax(dim=(0, 2, 3)) / (qmax - 0.5)).view(1, -1, 1, 1, 1, 1, 1)


def _calibrated(cls, q, kT, p, v):
    """An instance of `cls` with intervals set as a search would leave them, and its operands (A, B)."""
    from ptq4vit_amd.quant_layers import matmul as mm
    sos = cls in (mm.SoSPTQSLQuantMatMul, mm.SoSPTQSLBatchingQuantMatMul)
    A, B = (p, v) if sos else (q, kT)
    if cls is mm.MinMaxQuantMatMul:
        m = cls()
    elif sos:
        m = cls(split=torch.tensor(2.0 ** -5), n_G_B=H)
    else:
        m = cls(n_G_A=H, n_G_B=H)
        m.A_interval = _headwise(A, m.A_qmax)
    if cls is not mm.MinMaxQuantMatMul:
        m.B_interval = _headwise(B, m.B_qmax)
        m.calibrated = True
    return m, sos


def _all_classes():
    from ptq4vit_amd.quant_layers import matmul as mm
    return [mm.MinMaxQuantMatMul, mm.PTQSLQuantMatMul, mm.SoSPTQSLQuantMatMul, mm.PTQSLBatchingQuantMatMul,
            mm.SoSPTQSLBatchingQuantMatMul]


@pytest.mark.parametrize("cls", _all_classes(), ids=lambda c: c.__name__)
def test_module_classes_give_a_packed_view_the_output_of_its_copy(cls):
    g = torch.Generator().manual_seed(34)
    S, Dh = 17, 8
    q, k, v = (torch.randn(b, H, S, Dh, generator=g) * f for f in (Dh ** -0.5, 1.0, 1.0))
    q = q * torch.tensor([0.5, 1.0, 2.0]).view(1, H, 1, 1)             # another interval per head: a wrong head shows
    p = torch.softmax(torch.randn(b, H, S, S, generator=g) * 3, -1)
    qv, kTv, vv = ml.packed_qkv_views(q, k, v)
    kT = k.transpose(-2, -1).contiguous()
    m, sos = _calibrated(cls, q, kT, p, v)
    views, copies = ((p, vv) if sos else (qv, kTv)), ((p, v) if sos else (q, kT))
    assert not views[1].is_contiguous() and copies[1].is_contiguous()
    before = ml.allocation(qv).clone()
    with torch.no_grad():
        if type(m).__name__ == "MinMaxQuantMatMul":
            got, want = m.calibration_step2(*views), m.calibration_step2(*copies)
        else:
            got, want = m.quant_forward(*views), m.quant_forward(*copies)
    assert got.shape == (b, H, S, (Dh if sos else S)) and bool(torch.isfinite(got).all()), "a NaN of the packed buffer was read"
    assert torch.equal(got, want), f"{cls.__name__}: max |diff| {float((got - want).abs().max())}"
    assert not torch.equal(got, copies[0] @ copies[1]), "the module quantised nothing"
    after = ml.allocation(qv)
    assert torch.equal(after.view(torch.int32), before.view(torch.int32)), "the module stored into its operands' buffer"
