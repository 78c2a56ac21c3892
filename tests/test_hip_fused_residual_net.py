"""GPU: fuse_norm(net, residual=True) on the tiny Swin and the mini ViT (utils/fuse.py): the logits are
fuse_norm(net)'s bit for bit, every block makes two k_lin_res launches (proj and fc2), a hook on proj and the raw / calibration modes
fall back to the path without the fused residual, and unfuse_norm restores the unfused net."""
import pytest
import torch

from tests.test_hip_fused_norm_net import _fusers, mini  # noqa: F401  (the calibrated mini ViT, built as that file builds it)
from tests.test_hip_fused_window_attention import tiny  # noqa: F401  (the calibrated tiny Swin)

pytestmark = pytest.mark.gpu


def _kernels(eng, net, images):
    eng.stats_enable(True)
    try:
        eng.stats_reset()
        y = net(images)
        torch.cuda.synchronize()
        return y, [r["kernel"] for r in eng.stats_launches()]
    finally:
        eng.stats_enable(False)


@pytest.mark.parametrize("which", ["swin", "vit"])
def test_fused_residual_logits_launches_and_fallbacks(which, request):
    from ptq4vit_amd import engine as eng
    from ptq4vit_amd.utils import fuse, models
    net, wrapped, images = request.getfixturevalue("tiny" if which == "swin" else "mini")
    fuse_attn, unfuse_attn = _fusers(which)
    blocks = [m for m in net.modules() if isinstance(m, (models.Block, models.SwinBlock))]
    try:
        with torch.no_grad():
            y_plain = net(images)
            fuse.fuse_mlp(net); fuse_attn(net); fuse.fuse_norm(net)
            y_n, k_n = _kernels(eng, net, images)
            assert "k_lin_res" not in k_n
            fuse.fuse_norm(net, residual=True)                  # (the later call decides)
            y_r, k_r = _kernels(eng, net, images)
            assert torch.equal(y_r, y_n) and k_r.count("k_lin_res") == 2 * len(blocks), (k_r.count("k_lin_res"), len(blocks))
            # a hook on one proj: that block's attention side alone runs as before
            h = blocks[0].attn.proj.register_forward_hook(lambda mod, inp, out: None)
            y_h, k_h = _kernels(eng, net, images)
            h.remove()
            assert torch.equal(y_h, y_n) and k_h.count("k_lin_res") == 2 * len(blocks) - 1
            # raw and calibration modes: the original path
            for mode in ("raw", "calibration_step1"):
                for m in wrapped.values():
                    m.mode = mode
                assert "k_lin_res" not in _kernels(eng, net, images)[1]
            for m in wrapped.values():
                m.mode = "quant_forward"
            # the LayerNorm side unfused (a hook on norm2): fc2 still adds the residual
            h = blocks[0].norm2.register_forward_hook(lambda mod, inp, out: None)
            assert _kernels(eng, net, images)[1].count("k_lin_res") == 2 * len(blocks)
            h.remove()
            fuse.unfuse_norm(net)
            y_u, k_u = _kernels(eng, net, images)
            assert "k_lin_res" not in k_u and not any("_p4v_fuse_residual" in m.__dict__ for m in net.modules())
    finally:
        for m in wrapped.values():
            m.mode = "quant_forward"
        fuse.unfuse_norm(net); fuse.unfuse_mlp(net); unfuse_attn(net)
    with torch.no_grad():
        assert torch.equal(net(images), y_plain)
