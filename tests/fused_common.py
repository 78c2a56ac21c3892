"""Shared by tests/test_hip_fused_mlp.py and tests/test_hip_fused_attention.py: fp32 ulp distances, and the module-level helpers of
the mini-ViT tests (a one-batch loader, the wrapped modules of a copied net, their intervals, a counter on an engine call), and
the writer of the margins file."""
import torch


def _ordered(t):
    i = t.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulp_distance(a, b):
    return (_ordered(a) - _ordered(b)).abs()


def merge_margins(path, section, margins, ids):
    """Write the measured margins of one test file into the JSON file `path` (nothing when it is empty or unset), under the key
    `section` and next to what the file already holds: every {case id: value} table turned round into cases[id][table], the
    other entries as they are."""
    import json
    import os
    if not (margins and path):
        return
    path = os.path.abspath(path)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    old = {}
    if os.path.exists(path):
        with open(path) as fh:
            old = json.load(fh)
    sec = old.setdefault(section, {})
    for key, val in margins.items():
        if isinstance(val, dict) and val and set(val) <= set(ids):
            for cid, v in val.items():
                sec.setdefault("cases", {}).setdefault(cid, {})[key] = v
        else:
            sec[key] = val
    with open(path, "w") as fh:
        json.dump(old, fh, indent=1, sort_keys=True)
        fh.write("\n")


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
