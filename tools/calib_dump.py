"""GPU: what the calibrator (ptq4vit_amd/utils/quant_calib.py) does, as JSON -- to compare two checkouts of the Python side
on ONE library.  --tree DIR puts another checkout's root first on sys.path (default: this tree); the library is this tree's
(or P4V_LIB).  Only what every tree since round 6 has is read: the constructor, the six attribute knobs (`use_graph`,
`capture_lanes`, `search_streams`, `search_grouped`, `group_calls`, `shard_capture`), `timings["modules"]` / `["owned"]`,
`capture_mode`, `owner`, the engine's launch counters and pass-memo statistics, the `_p4v_*` keys of `net.__dict__`, and the
modules' intervals and caches.

Two networks (those of tests/test_hip_model.py: the mini ViT of tests/golden/minivit_ptq4vit.npz with its 8 images, the tiny
Swin of test_graph_capture_equals_eager_capture with 8 seeded images at 56 x 56), PTQ4ViT, batch_size=2, sequential=False;
per network the scenarios of `run()` in order.  Per scenario: capture_mode, modules / owned, which `_p4v_*` keys are set, graph
keys and lanes, launch counters, memo hits / misses, a sha256 over all intervals and splits in module order and -- where a direct
`_capture` of every module precedes the calibration -- one over every raw_input / raw_out / raw_grad.  No timings: two runs of the
same tree give the same file.

    python tools/calib_dump.py [--tree DIR] [--out FILE]
"""
import argparse
import contextlib
import hashlib
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=HERE)
ap.add_argument("--out", default=None)
args = ap.parse_args()
os.environ.setdefault("P4V_LIB", os.path.join(HERE, "ptq4vit_amd", "csrc", "libptq4vit_hip.so"))
sys.path.insert(0, os.path.abspath(args.tree))
import ptq4vit_amd  # noqa: E402
ptq4vit_amd.configure_runtime()
import numpy as np  # noqa: E402
import torch  # noqa: E402
from ptq4vit_amd import engine  # noqa: E402
from ptq4vit_amd.configs import BasePTQ, PTQ4ViT  # noqa: E402
from ptq4vit_amd.utils import models, net_wrap  # noqa: E402
from ptq4vit_amd.utils.quant_calib import HessianQuantCalibrator, QuantCalibrator  # noqa: E402

NET_KEYS = ("_p4v_capture_graphs", "_p4v_capture_shadow", "_p4v_calibrations", "_p4v_module_ms", "_p4v_cache_sizes")
INTERVALS = ("w_interval", "a_interval", "A_interval", "B_interval", "split")
DEV = torch.device("cuda:0")


class Loader:
    def __init__(self, x):
        self.x, self.batch_size = x, x.shape[0]

    def __iter__(self):
        yield self.x, None


class L2Config:
    """BasePTQ's modules under the L2_norm metric (no gradients needed)."""
    @staticmethod
    def get_module(kind, *a, **k):
        m = BasePTQ.get_module(kind, *a, **k)
        if hasattr(m, "metric"):
            m.metric = "L2_norm"
        return m


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def feed(h, v):
    if v is None:
        h.update(b"<none>")
    elif isinstance(v, (list, tuple)):
        h.update(b"[%d]" % len(v))
        for e in v:
            feed(h, e)
    else:
        a = torch.as_tensor(v).detach().contiguous().cpu().numpy()
        h.update(str((a.dtype, a.shape)).encode())
        h.update(a.tobytes())


def digest(wrapped, attrs):
    h = hashlib.sha256()
    for n, m in wrapped.items():
        h.update(n.encode())
        for a in attrs:
            feed(h, getattr(m, a, None))
    return h.hexdigest()


def calibrate(net, wrapped, x, capture=False, sequential=False, env=None, **attrs):
    """One scenario: a new calibrator on (net, wrapped, x), every module back in raw mode, `attrs` set after construction."""
    for m in wrapped.values():
        m.mode = "raw"
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        cal = HessianQuantCalibrator(net, wrapped, Loader(x), sequential=sequential, batch_size=2)
        for k, v in attrs.items():
            setattr(cal, k, v)
        row = {}
        with quiet():
            if capture:
                cal._capture(list(wrapped), cal._raw_pred_softmax(), True)
                torch.cuda.synchronize()
                row["captures"] = digest(wrapped, ("raw_input", "raw_out", "raw_grad"))
            engine.launch_counters(reset=True)
            engine.stats_reset()
            cal.batching_quant_calib()
            torch.cuda.synchronize()
        return dict(row, **snapshot(cal, net, wrapped))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def snapshot(cal, net, wrapped):
    graphs = net.__dict__.get("_p4v_capture_graphs") or {}
    counters, stats = engine.launch_counters(), engine.stats_get()
    return {"capture_mode": cal.capture_mode, "modules": cal.timings["modules"], "owned": cal.timings["owned"],
            "owner": sorted(set(cal.owner.values())),
            "net_keys": [k for k in NET_KEYS if net.__dict__.get(k)],
            "graph_keys": len(graphs), "lanes": sum(len(v) for v in graphs.values()),
            "launches": {k: counters[k] for k in ("asked", "issued", "rounds")},
            "memo": {k: int(stats[k]) for k in ("memo_hits", "memo_misses")},
            "intervals": digest(wrapped, INTERVALS)}


def run(make, x, mini):
    """`make(seed, config)` -> (net, wrapped)."""
    rows = {}
    net, wrapped = make(None, PTQ4ViT)
    rows["01_first"] = calibrate(net, wrapped, x, capture=True)
    rows["02_second"] = calibrate(net, wrapped, x, capture=True)
    rows["03_third"] = calibrate(net, wrapped, x)
    sizes = HessianQuantCalibrator(net, wrapped, Loader(x), batch_size=2)._estimate_cache_bytes(list(wrapped))
    rows["04_budget"] = calibrate(net, wrapped, x, cache_budget_bytes=int(sum(sizes.values()) / 3.5))
    rows["05_not_grouped"] = calibrate(net, wrapped, x, search_grouped=False)
    rows["06_one_stream"] = calibrate(net, wrapped, x, search_streams=1)
    rows["07_two_group_calls"] = calibrate(net, wrapped, x, group_calls=2)
    rows["08_no_graph"] = calibrate(net, wrapped, x, capture=True, use_graph=False)
    rows["09_one_lane"] = calibrate(net, wrapped, x, capture=True, capture_lanes=1)
    rows["10_four_images"] = calibrate(net, wrapped, x[:4], capture=True)
    HessianQuantCalibrator._ARCH.clear()
    for seed in (1, 2, 3):
        rows[f"11_fresh_seed{seed}"] = calibrate(*make(seed, PTQ4ViT), x, capture=True)
    net12, wrapped12 = make(4, PTQ4ViT)
    rows["12_no_arch_graphs_first"] = calibrate(net12, wrapped12, x, env={"P4V_ARCH_GRAPHS": "0"})
    rows["12_no_arch_graphs_second"] = calibrate(net12, wrapped12, x, env={"P4V_ARCH_GRAPHS": "0"})
    if mini:
        net13, wrapped13 = make(None, L2Config)
        with quiet():
            engine.launch_counters(reset=True)
            engine.stats_reset()
            QuantCalibrator(net13, wrapped13, Loader(x), sequential=False).batching_quant_calib()
            torch.cuda.synchronize()
        counters = engine.launch_counters()
        rows["13_quant_calibrator_l2"] = {"net_keys": [k for k in NET_KEYS if net13.__dict__.get(k)],
                                          "launches": {k: counters[k] for k in ("asked", "issued", "rounds")},
                                          "intervals": digest(wrapped13, INTERVALS)}
        rows["14_sequential"] = calibrate(net, wrapped, x, sequential=True)
    HessianQuantCalibrator._ARCH.clear()
    return rows


def main():
    g = np.load(os.path.join(HERE, "tests", "golden", "minivit_ptq4vit.npz"), allow_pickle=False)
    vit_kw = json.loads(str(g["model_kwargs"]))
    swin_kw = dict(img_size=56, embed_dim=24, depths=(2, 2), num_heads=(2, 4), num_classes=10)

    def maker(model, kw, seed0):
        def make(seed, config):
            net = models.get_net(model, seed=seed0 if seed is None else seed, device=DEV, **kw)
            with quiet():
                return net, net_wrap.wrap_modules_in_net(net, config)
        return make

    out = {"mini_vit": run(maker("vit_tiny_patch16_224", vit_kw, 0), torch.from_numpy(g["images"]).to(DEV), True),
           "tiny_swin": run(maker("swin_tiny_patch4_window7_224", swin_kw, 3),
                            torch.randn(8, 3, 56, 56, generator=torch.Generator().manual_seed(5)).to(DEV), False)}
    text = json.dumps(out, indent=1, sort_keys=True) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
