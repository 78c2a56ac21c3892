"""GPU: fuse_norm on the tiny Swin and the mini ViT (utils/fuse.py) -- which sides take the fused LayerNorm path in
which state, that unfuse_norm restores the unfused logits bit for bit, that a second calibration of a fused net gives the same
intervals, and the wiring gate: the logits differ from the unfused fused-net's only through LayerNorm's summation order, so
|fused - unfused| / |unfused - raw fp32| <= 0.1 (a wrong row map or interval gives a ratio near 1; not a precision claim -- the
exact checks are tests/test_hip_fused_norm.py's).  With P4V_FUSED_NORM_OUT set the ratios go there."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests.fused_common import _Loader, _intervals, _wrapped_of, merge_margins
from tests.test_hip_fused_window_attention import tiny  # noqa: F401  (the calibrated tiny Swin, built as that file builds it)

pytestmark = pytest.mark.gpu
_MARGINS = {}


@pytest.fixture(scope="module")
def eng():
    from ptq4vit_amd import engine
    yield engine
    engine.release_workspace()
    merge_margins(os.environ.get("P4V_FUSED_NORM_OUT"), "net", _MARGINS, ["swin", "vit"])


@pytest.fixture(scope="module")
def mini():
    from ptq4vit_amd.configs import PTQ4ViT
    from ptq4vit_amd.utils import models, net_wrap
    from ptq4vit_amd.utils.quant_calib import HessianQuantCalibrator
    g = np.load("tests/golden/minivit_ptq4vit.npz", allow_pickle=False)
    net = models.get_net("vit_tiny_patch16_224", seed=0, device="cuda", **json.loads(str(g["model_kwargs"])))
    wrapped = net_wrap.wrap_modules_in_net(net, PTQ4ViT)
    images = torch.from_numpy(g["images"][:4]).cuda()
    HessianQuantCalibrator(net, wrapped, _Loader(images), sequential=False, batch_size=4).batching_quant_calib()
    return net, wrapped, images


def _fusers(which):
    from ptq4vit_amd.utils import fuse
    attn = (lambda n: fuse.fuse_window_attention(n, one_kernel=True)) if which == "swin" else fuse.fuse_attention
    unattn = fuse.unfuse_window_attention if which == "swin" else fuse.unfuse_attention
    return attn, unattn


def _count_ln_calls(eng, monkeypatch):
    """counts the calls of engine.linear_quant_forward / mlp_quant_forward that carry ln= from here on"""
    counts = {"linear_quant_forward": [], "mlp_quant_forward": []}
    for name, calls in counts.items():
        def counted(_orig=getattr(eng, name), _calls=calls, **kw):
            if kw.get("ln") is not None:
                _calls.append(1)
            return _orig(**kw)
        monkeypatch.setattr(eng, name, counted)
    return counts["linear_quant_forward"], counts["mlp_quant_forward"]


def _probe(net, block, images):
    """the tensor entering `block` on `images`"""
    seen = []
    h = block.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    net(images)
    h.remove()
    return seen[0]


@pytest.mark.parametrize("which", ["swin", "vit"])
def test_fuse_norm_paths_logits_and_restore(eng, which, request, monkeypatch):
    from ptq4vit_amd.utils import fuse, models
    net, wrapped, images = request.getfixturevalue("tiny" if which == "swin" else "mini")
    fuse_attn, unfuse_attn = _fusers(which)
    blocks = [n for n, m in net.named_modules() if isinstance(m, (models.Block, models.SwinBlock))]
    mods = dict(net.named_modules())
    takes = lambda x, side=None: [fuse.takes_fused_norm_path(mods[n], x, side) for n in blocks]
    try:
        with torch.no_grad():
            y_plain = net(images)
            for m in wrapped.values():
                m.mode = "raw"
            y_raw = net(images)
            for m in wrapped.values():
                m.mode = "quant_forward"
            fuse.fuse_mlp(net)
            fuse_attn(net)
            y_u = net(images)
            x0 = _probe(net, mods[blocks[0]], images)
            for order in (0, 1):                                # fuse_norm after the containers' patches, and before them
                if order:
                    fuse.unfuse_mlp(net); unfuse_attn(net)
                    assert fuse.fuse_norm(net) == sorted(blocks) and not any(takes(x0))
                    fuse.fuse_mlp(net); fuse_attn(net)
                assert fuse.fuse_norm(net) == sorted(blocks) and fuse.fuse_norm(net) == sorted(blocks)
                lin, mlp = _count_ln_calls(eng, monkeypatch)
                y_f = net(images)
                assert len(lin) == len(mlp) == len(blocks) and fuse.takes_fused_norm_path(mods[blocks[0]], x0)
                monkeypatch.undo()
                ratio = ((y_f - y_u).norm() / (y_u - y_raw).norm()).item()
                print(f"[fused norm net] {which}: |fused - unfused| / |unfused - raw| = {ratio:.4f}")
                _MARGINS.setdefault("logit_ratio", {})[which] = ratio
                assert ratio <= 0.1, ratio
                assert fuse.unfuse_norm(net) == sorted(blocks) and torch.equal(net(images), y_u)
            fuse.fuse_norm(net)
            b0 = mods[blocks[0]]
            # raw and calibration modes: nothing fused
            for mode in ("raw", "calibration_step1"):
                for m in wrapped.values():
                    m.mode = mode
                assert not fuse.takes_fused_norm_path(b0, x0, "norm1") and not fuse.takes_fused_norm_path(b0, x0, "norm2")
            for m in wrapped.values():
                m.mode = "quant_forward"
            # a hook on norm1: that side alone falls back
            h = b0.norm1.register_forward_hook(lambda mod, inp, out: None)
            assert not fuse.takes_fused_norm_path(b0, x0) and not fuse.takes_fused_norm_path(b0, x0, "norm1") and fuse.takes_fused_norm_path(b0, x0, "norm2")
            assert torch.isfinite(net(images)).all()
            h.remove()
            # an MLP container without fuse_mlp's patch: the norm2 side is not fused, the norm1 side still is
            fuse.unfuse_mlp(net)
            assert not fuse.takes_fused_norm_path(b0, x0) and not fuse.takes_fused_norm_path(b0, x0, "norm2") and fuse.takes_fused_norm_path(b0, x0, "norm1")
            lin, mlp = _count_ln_calls(eng, monkeypatch)
            net(images)
            assert len(lin) == len(blocks) and not mlp
            monkeypatch.undo()
            if which == "vit":                                  # fuse_qkv_attention keeps norm1 in torch; the logits still come
                fuse.fuse_qkv_attention(net)
                assert not fuse.takes_fused_norm_path(b0, x0, "norm1")
                assert torch.isfinite(net(images)).all()
    finally:
        for m in wrapped.values():
            m.mode = "quant_forward"
        fuse.unfuse_norm(net); fuse.unfuse_mlp(net); unfuse_attn(net)
    with torch.no_grad():
        assert torch.equal(net(images), y_plain) and not any("forward" in m.__dict__ for m in net.modules())


def test_second_calibration_of_a_fused_net_gives_the_same_intervals(eng, tiny, monkeypatch):  # noqa: F811
    from ptq4vit_amd.utils import fuse
    from ptq4vit_amd.utils.quant_calib import HessianQuantCalibrator
    net, wrapped, images = tiny
    net_u, net_f = copy.deepcopy(net), copy.deepcopy(net)
    wrapped_u, wrapped_f = _wrapped_of(net_u, wrapped), _wrapped_of(net_f, wrapped)
    fuse.fuse_mlp(net_f); fuse.fuse_window_attention(net_f, one_kernel=True); fuse.fuse_norm(net_f)
    HessianQuantCalibrator(net_u, wrapped_u, _Loader(images), sequential=False, batch_size=4).batching_quant_calib()
    HessianQuantCalibrator(net_f, wrapped_f, _Loader(images), sequential=False, batch_size=4).batching_quant_calib()
    iu, ifu = _intervals(wrapped_u), _intervals(wrapped_f)
    assert iu.keys() == ifu.keys() and all(torch.equal(iu[k], ifu[k]) for k in iu)
    _, calls = _count_ln_calls(eng, monkeypatch)
    with torch.no_grad():
        net_f(images)
    assert calls
