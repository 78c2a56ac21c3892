"""GPU: fuse_norm(net, residual=True, proj_plane=True) on the tiny Swin and the mini ViT (utils/fuse.py): on the
one-kernel cores the logits are fuse_norm(net, residual=True)'s bit for bit, every block makes one plane-instance launch and no
launch of the core that writes fp32, containers that did not ask for one kernel run as before, and unfuse_norm restores the net."""
import pytest
import torch

from tests.test_hip_fused_norm_net import mini  # noqa: F401  (the calibrated mini ViT, built as that file builds it)
from tests.test_hip_fused_residual_net import _kernels
from tests.test_hip_fused_window_attention import tiny  # noqa: F401  (the calibrated tiny Swin)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which", ["swin", "vit"])
def test_proj_plane_logits_and_launches(which, request):
    from ptq4vit_amd import engine as eng
    from ptq4vit_amd.utils import fuse, models
    net, wrapped, images = request.getfixturevalue("tiny" if which == "swin" else "mini")
    fuse_attn, unfuse_attn = (fuse.fuse_window_attention, fuse.unfuse_window_attention) if which == "swin" else \
        (fuse.fuse_attention, fuse.unfuse_attention)
    blocks = [m for m in net.modules() if isinstance(m, (models.Block, models.SwinBlock))]
    core, inst = ("k_wattn_qkpv", "k_wattn_qkpv_plane") if which == "swin" else ("k_attn_qkpv", "k_attn_qkpv_plane")
    try:
        with torch.no_grad():
            y_plain = net(images)
            fuse.fuse_mlp(net); fuse_attn(net, one_kernel=True); fuse.fuse_norm(net, residual=True)
            y_r, k_r = _kernels(eng, net, images)
            assert k_r.count(core) == len(blocks) and inst not in k_r
            fuse.fuse_norm(net, residual=True, proj_plane=True)         # (the later call decides)
            y_p, k_p = _kernels(eng, net, images)
            assert torch.equal(y_p, y_r), "proj_plane changed the logits"
            assert k_p.count(inst) == len(blocks) and core not in k_p and k_p.count("k_lin_res") == 2 * len(blocks), k_p
            # a container that did not ask for one kernel, and no residual=: the flag changes nothing
            fuse_attn(net)
            y_2, k_2 = _kernels(eng, net, images)
            assert torch.equal(y_2, y_r) and inst not in k_2
            fuse_attn(net, one_kernel=True); fuse.fuse_norm(net, proj_plane=True)
            assert inst not in _kernels(eng, net, images)[1]
            fuse.unfuse_norm(net)
            assert not any("_p4v_fuse_proj_plane" in m.__dict__ for m in net.modules())
    finally:
        fuse.unfuse_norm(net); fuse.unfuse_mlp(net); unfuse_attn(net)
    with torch.no_grad():
        assert torch.equal(net(images), y_plain)
