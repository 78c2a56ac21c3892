"""Time the cosine Linear search with column / activation blocks against the same layer without blocks (GPU tool).

One ViT-B/224 qkv layer at 32 images (32 x 197 x 768 -> 2304, n_V = 3, cosine, the BasePTQ search settings, one round):
    blocks     n_H = 2, n_a = 2: k_pack_seg / k_sweep_seg<EPI_COS> / k_finish_cos, four block steps, no pruning
    unblocked  n_H = n_a = 1:    the register-stationary k_sweep6 with the cosine epilogues
alternating in one process; device events around every call, one warm-up call per variant, at least 0.5 s of timed work per
variant.  One further call per variant runs with the engine's launch timing on (not part of the timed work) for the sweep
kernels' own launch records.  Writes profiles/r14_linblk_cos.json.

    python tools/bench_linear_blocks.py [--out profiles/r14_linblk_cos.json] [--images 32]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_I8 = 5000.0        # TOP/s, dense int8 MFMA (bench.py's convention: 2 x the 2.5 PF bf16 dense spec)
SEARCH = dict(metric="cosine", eq_alpha=0.5, eq_beta=1.2, eq_n=100, search_round=1, w_bit=8, a_bit=8)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_linblk_cos.json"))
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    args = ap.parse_args(argv)
    import torch
    from ptq4vit_amd import _lib, engine
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    b, T, K, N, nV = args.images, 197, 768, 2304, 3
    w = torch.randn(N, K, generator=gen) * 0.05 * torch.linspace(0.5, 2.0, N).view(-1, 1)
    bias = torch.randn(N, generator=gen) * 0.1
    x = torch.randn(b, T, K, generator=gen)
    w, bias, x = w.to(dev), bias.to(dev), x.to(dev)
    out = torch.nn.functional.linear(x, w, bias)
    variants = {"blocks": (2, 2), "unblocked": (1, 1)}
    jobs = {vn: engine.linear_job(weight=w, bias=bias, x=x, out=out, grad=None, n_V=nV, n_H=nH, n_a=nA, **SEARCH)
            for vn, (nH, nA) in variants.items()}
    times = {vn: [] for vn in variants}
    for vn in variants:                                              # warm-up
        engine.run_job(jobs[vn])
    torch.cuda.synchronize()
    while min(sum(t) for t in times.values()) < args.min_seconds * 1e3 or min(len(t) for t in times.values()) < 3:
        for vn in variants:                                          # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            engine.run_job(jobs[vn])
            e1.record()
            e1.synchronize()
            times[vn].append(e0.elapsed_time(e1))
    result = {"source_hash": _lib.source_hash(), "batch_tokens_K_N": [b, T, K, N], "n_V": nV, "search": SEARCH,
              "peak_int8_tops": PEAK_I8}
    for vn, (nH, nA) in variants.items():                            # the sweep kernels' own launch records (launch timing on)
        engine.stats_reset()
        engine.stats_enable(True)
        try:
            engine.run_job(jobs[vn])
            torch.cuda.synchronize()
            recs = engine.stats_launches()
        finally:
            engine.stats_enable(False)
        by = {}
        for r in recs:
            d = by.setdefault(r["kernel"], {"launches": 0, "ms": 0.0, "alg_ops": 0.0})
            d["launches"] += 1
            d["ms"] += r["ms"]
            d["alg_ops"] += r["alg_ops"]
        t = sorted(times[vn])
        result[vn] = {"n_H": nH, "n_a": nA, "calls": len(t), "median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1],
                      "sweep_kernels": by}
        if vn == "blocks":
            result[vn]["k_sweep_seg_launches"] = [r for r in recs if r["kernel"] == "k_sweep_seg"]
        for d in by.values():
            d["achieved_tops"] = d["alg_ops"] / (d["ms"] * 1e-3) / 1e12 if d["ms"] > 0 else None
    result["ratio_blocks_over_unblocked"] = result["blocks"]["median_ms"] / result["unblocked"]["median_ms"]
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(f"[bench_linear_blocks] wrote {args.out}")


if __name__ == "__main__":
    main()
