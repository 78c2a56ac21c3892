"""Shared by tests/test_hip_fused_mlp.py and tests/test_hip_fused_attention.py: fp32 ulp distances, and the module-level helpers of
the mini-ViT tests (a one-batch loader, the wrapped modules of a copied net, their intervals, a counter on an engine call)."""
import torch


def _ordered(t):
    i = t.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulp_distance(a, b):
    return (_ordered(a) - _ordered(b)).abs()


class _Loader:
    def __init__(self, images):
        self.images, self.batch_size = images, images.shape[0]

    def __iter__(self):
        yield self.images, torch.zeros(self.images.shape[0], dtype=torch.long)


def _wrapped_of(net, names):
    mods = dict(net.named_modules())
    return {n: mods[n] for n in names}


def _intervals(wrapped):
    out = {}
    for n, m in wrapped.items():
        for a in ("w_interval", "a_interval", "A_interval", "B_interval", "split"):
            v = getattr(m, a, None)
            if v is not None:
                out[f"{n}.{a}"] = torch.as_tensor(v).detach().cpu().clone()
    return out


def _count_fused_calls(eng, monkeypatch, name):
    """counts the calls of engine.<name> (mlp_quant_forward / attn_quant_forward) from here on"""
    calls = []
    orig = getattr(eng, name)

    def counted(**kw):
        calls.append(1)
        return orig(**kw)
    monkeypatch.setattr(eng, name, counted)
    return calls
