#!/usr/bin/env python
"""Throughput of the calibrated network's quant_forward (the top-1 evaluation loop of the
reference, example/test_vit.py:26-45) next to the raw fp32 forward.

    python tools/bench_forward.py --model vit_base_patch16_224 --batch 128
    python tools/bench_forward.py --model vit_base_patch16_224 --batch 128 --fused --json profiles/forward.json

--fused: the same network with its MLPs fused (utils/fuse.py::fuse_mlp) next to the unfused one, alternating in one process,
medians over --reps repetitions each, and the per-kernel device time of one forward of each kind: the engine's launch records
for the GEMMs (k_mlp_fc1, the fc2 sweep), torch's profiler for everything (k_pack*, torch's GELU).
--fused-attn: a further variant in the same alternation, the attention blocks fused (fuse_attention: k_attn_qk in place of
matmul1's sweep, torch's `* scale` and softmax and k_pack_dual; on a Swin net fuse_window_attention: the window instances of
k_attn_qk in place of matmul1's sweep, torch's `+ bias`, `+ mask` and softmax and k_pack_dual); with --fused it is MLPs +
attention, without it attention alone.
--fused-qkv: a fourth variant in the same alternation: fuse_qkv_attention in place of fuse_attention (k_qkv_heads in place of the
qkv sweep, the permute copy and the three k_pack1 of q, k^T and v), on top of the fused MLPs with --fused.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ptq4vit_amd import _lib, engine  # noqa: E402
from ptq4vit_amd.configs import PTQ4ViT  # noqa: E402
from ptq4vit_amd.utils import fuse, models, net_wrap  # noqa: E402
from ptq4vit_amd.utils.quant_calib import HessianQuantCalibrator  # noqa: E402


class Loader:
    def __init__(self, x):
        self.x = x

    def __iter__(self):
        yield self.x, torch.zeros(self.x.shape[0], dtype=torch.long, device=self.x.device)


def engine_records(net, x):
    """{kernel: [launches, ms]} of the engine's timed launches (the GEMMs) in one forward."""
    engine.stats_enable(True)
    engine.stats_reset()
    with torch.no_grad():
        net(x)
    torch.cuda.synchronize()
    engine.stats_get()                   # (drains the event pairs into the records)
    out = {}
    for r in engine.stats_launches():
        e = out.setdefault(r["kernel"], [0, 0.0])
        e[0] += 1
        e[1] += r["ms"]
    engine.stats_enable(False)
    engine.stats_reset()
    return out


def profiler_kernels(net, x):
    """{kernel name: [launches, ms]} of every GPU kernel of one forward (torch.profiler); None where it is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            with torch.no_grad():
                net(x)
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            dt = getattr(ev, "device_time", None)
            if dt is None:
                dt = getattr(ev, "cuda_time", 0.0)
            if str(getattr(ev, "device_type", "")).endswith("CUDA") and dt:
                e = out.setdefault(ev.name, [0, 0.0])
                e[0] += 1
                e[1] += dt / 1e3
        return out or None
    except Exception as exc:      # noqa: BLE001 -- a measurement aid: the timing above does not depend on it
        print(f"[bench_forward] torch.profiler not usable here: {exc}", file=sys.stderr)
        return None


def short(tab, keep=14):
    if tab is None:
        return None
    rows = sorted(tab.items(), key=lambda kv: -kv[1][1])[:keep]
    return [{"kernel": k[:120], "launches": n, "ms": round(ms, 4)} for k, (n, ms) in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="vit_base_patch16_224")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fused", action="store_true", help="also time the network with fused MLPs (utils/fuse.py), alternating")
    ap.add_argument("--fused-attn", action="store_true",
                    help="also time the network with fused attention (utils/fuse.py::fuse_attention and fuse_window_attention; with --fused: on top of the fused MLPs)")
    ap.add_argument("--fused-qkv", action="store_true",
                    help="also time the network with the qkv layer fused into the attention chain (utils/fuse.py::fuse_qkv_attention; with --fused: on top of the fused MLPs)")
    ap.add_argument("--json", default=None, help="write the result to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    net = models.get_net(a.model, seed=0, device=dev)
    wrapped = net_wrap.wrap_modules_in_net(net, PTQ4ViT)
    img = models.input_size(a.model)
    g = torch.Generator(device="cpu").manual_seed(0)
    calib = torch.randn(32, 3, img, img, generator=g).to(dev)
    HessianQuantCalibrator(net, wrapped, Loader(calib), sequential=False, batch_size=4).batching_quant_calib()
    x = torch.randn(a.batch, 3, img, img, generator=g).to(dev)

    def once():
        torch.cuda.synchronize()
        t = time.time()
        with torch.no_grad():
            y = net(x)
        torch.cuda.synchronize()
        return time.time() - t, y

    def timed(mode, reps):
        for m in wrapped.values():
            m.mode = mode
        once()
        ts = []
        for _ in range(reps):
            t, y = once()
            ts.append(t)
        return statistics.median(ts), y

    t_raw, y_raw = timed("raw", a.reps)
    t_q, y_q = timed("quant_forward", a.reps)
    print(f"{a.model} batch {a.batch}: raw fp32 {a.batch / t_raw:.0f} img/s ({t_raw * 1e3:.1f} ms), "
          f"quant_forward {a.batch / t_q:.0f} img/s ({t_q * 1e3:.1f} ms); "
          f"logit rel diff {((y_q - y_raw).norm() / y_raw.norm()).item():.3e}")
    res = {"model": a.model, "batch": a.batch, "reps": a.reps, "source_hash": _lib.source_hash(),
           "raw_fp32_ms": t_raw * 1e3, "quant_forward_ms": t_q * 1e3, "quant_vs_fp32": t_raw / t_q}
    if a.fused or a.fused_attn or a.fused_qkv:
        # the variants alternating, repetition by repetition, after one warm-up of each: (key, fuse the MLPs, fuse the attention --
        # "qkv": with the qkv layer)
        variants = [("unfused", False, False)]
        if a.fused:
            variants.append(("fused", True, False))
        if a.fused_attn:
            variants.append(("fused_attn", a.fused, True))
        if a.fused_qkv:
            variants.append(("fused_qkv", a.fused, "qkv"))

        def setup(mlp, attn):
            fuse.unfuse_mlp(net)
            fuse.unfuse_attention(net)
            fuse.unfuse_window_attention(net)
            fuse_attn = fuse.fuse_qkv_attention if attn == "qkv" else fuse.fuse_attention
            return (len(fuse.fuse_mlp(net)) if mlp else 0, len(fuse_attn(net)) + len(fuse.fuse_window_attention(net)) if attn else 0)

        ts = {key: [] for key, _, _ in variants}
        ys, counts = {}, {}
        for rep in range(a.reps + 1):
            for key, mlp, attn in variants:
                counts[key] = setup(mlp, attn)
                t, ys[key] = once()
                if rep:
                    ts[key].append(t)
        med = {key: statistics.median(v) for key, v in ts.items()}
        t_u = med["unfused"]
        res.update({"unfused_ms": t_u * 1e3, "unfused_ms_all": [t * 1e3 for t in ts["unfused"]]})
        for key, _, _ in variants[1:]:
            t_v, (n_mlp, n_attn) = med[key], counts[key]
            rel = ((ys[key] - ys["unfused"]).norm() / ys["unfused"].norm()).item()
            if key == "fused":
                print(f"  unfused {t_u * 1e3:.2f} ms, fused MLPs ({n_mlp}) {t_v * 1e3:.2f} ms: x{t_u / t_v:.3f}; "
                      f"fused vs fp32 x{t_raw / t_v:.2f}; logit rel diff fused vs unfused {rel:.3e}")
                res["fused_mlps"] = n_mlp
            elif key == "fused_qkv":
                base_key = "fused_attn" if a.fused_attn else "fused" if a.fused else "unfused"
                print(f"  fused qkv + attention ({n_attn}{' + MLPs' if a.fused else ''}) {t_v * 1e3:.2f} ms: x{med[base_key] / t_v:.3f} "
                      f"over {base_key} ({(med[base_key] - t_v) * 1e3:+.3f} ms), x{t_u / t_v:.3f} over unfused; logit rel diff vs unfused {rel:.3e}")
                res.update({"fused_qkv_attentions": n_attn, "fused_qkv_with_mlps": bool(a.fused), base_key + "_over_fused_qkv": med[base_key] / t_v,
                            base_key + "_minus_fused_qkv_ms": (med[base_key] - t_v) * 1e3})
            else:
                base_key = "fused" if a.fused else "unfused"
                print(f"  fused attention ({n_attn}{' + MLPs' if a.fused else ''}) {t_v * 1e3:.2f} ms: x{med[base_key] / t_v:.3f} "
                      f"over {base_key}, x{t_u / t_v:.3f} over unfused; vs fp32 x{t_raw / t_v:.2f}; logit rel diff vs unfused {rel:.3e}")
                res.update({"fused_attentions": n_attn, "fused_attn_with_mlps": bool(a.fused), base_key + "_over_fused_attn": med[base_key] / t_v})
            res.update({key + "_ms": t_v * 1e3, "unfused_over_" + key: t_u / t_v, key + "_vs_fp32": t_raw / t_v,
                        key + "_ms_all": [t * 1e3 for t in ts[key]], f"logit_rel_diff_{key}_vs_unfused": rel})
        # a digest of each variant's logit bytes: two libraries that compute the same thing give the same three
        res["logits_sha256"] = {key: hashlib.sha256(y.float().cpu().numpy().tobytes()).hexdigest()[:16] for key, y in ys.items()}
        kern = {}
        for key, mlp, attn in variants:
            setup(mlp, attn)
            kern[key] = {"engine_records": short(engine_records(net, x)), "profiler": short(profiler_kernels(net, x))}
            for row in kern[key]["profiler"] or kern[key]["engine_records"]:
                print(f"  [{key}] {row['ms']:9.3f} ms  {row['launches']:4d} x  {row['kernel'][:90]}")
        res["kernels_per_forward"] = kern
        setup(False, False)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
