"""Time the fused MatMul search with row / column sub-blocks against the head-wise search (GPU tool).

The ViT-B/224 attention shapes at 32 images (hessian metric, the PTQ4ViT search settings):
    q.k^T    32 x 12 x 197 x 64 x 197
    attn.v   32 x 12 x 197 x 197 x 64, split-of-softmax on A
each head-wise and with all four block counts = 2, alternating in one process; device events around every call, one warm-up
call per variant, at least 0.5 s of timed work per variant.  One further call per variant runs with the engine's launch timing
on (not part of the timed work) for the sweep kernels' own time.  Writes profiles/r10_matmul_blocks.json.

    python tools/bench_matmul_blocks.py [--out profiles/r10_matmul_blocks.json] [--images 32]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_I8 = 5000.0        # TOP/s, dense int8 MFMA (bench.py's convention: 2 x the 2.5 PF bf16 dense spec)
SEARCH = dict(metric="hessian", eq_alpha=0.01, eq_beta=1.2, eq_n=100, search_round=3, A_bit=8, B_bit=8)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_matmul_blocks.json"))
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    args = ap.parse_args(argv)
    import torch
    import __graft_entry__ as g
    g.build()
    from ptq4vit_amd import _lib, engine
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    b, H, T, hd = args.images, 12, 197, 64
    shapes = []
    q = torch.randn(b, H, T, hd, generator=gen)
    k = torch.randn(b, H, T, hd, generator=gen)
    v = torch.randn(b, H, T, hd, generator=gen)
    probs = torch.softmax(q @ k.transpose(-2, -1) / hd ** 0.5 * 3.0, dim=-1)
    shapes.append(("qk", q, k.transpose(-2, -1), False))                 # B handed over as a transposed view, as the models do
    shapes.append(("attn_v", probs, v, True))
    result = {"source_hash": _lib.source_hash(), "images": b, "search": SEARCH, "peak_int8_tops": PEAK_I8, "shapes": {}}
    for name, A, B, sos in shapes:
        A, B = A.to(dev), B.to(dev)
        out = (A @ B).contiguous()
        grad = (torch.randn(out.shape, generator=gen) * 1e-3).to(dev)
        M, K, N = A.shape[2], A.shape[3], B.shape[3]
        variants = {"headwise": (1, 1, 1, 1), "blocks2": (1, 1, 2, 2) if sos else (2, 2, 2, 2)}
        jobs = {vn: engine.matmul_job(A=A, B=B, out=out, grad=grad, sos=sos, blocks=blk, **SEARCH) for vn, blk in variants.items()}
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
        sweeps = {}
        for vn in variants:                                              # the sweep kernels' own time (launch timing on)
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
                d = by.setdefault(r["kernel"], {"launches": 0, "ms": 0.0})
                d["launches"] += 1
                d["ms"] += r["ms"]
            sweeps[vn] = by
        entry = {"batch_heads_M_K_N": [b, H, M, K, N], "sos": sos, "blocks": variants["blocks2"]}
        for vn in variants:
            t = sorted(times[vn])
            entry[vn] = {"calls": len(t), "median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "sweep_kernels": sweeps[vn]}
        blk = variants["blocks2"]
        steps = (1 if sos else blk[0] * blk[1]) + blk[2] * blk[3]
        block_steps = steps - (1 if sos else 0)                          # the split search is the head-wise engine's pass
        seg = sweeps["blocks2"].get("k_sweep_seg", {"ms": 0.0, "launches": 0})
        macs = float(SEARCH["search_round"]) * block_steps * SEARCH["eq_n"] * b * H * M * K * N * (2 if sos else 1)
        entry["ratio_blocks_over_headwise"] = entry["blocks2"]["median_ms"] / entry["headwise"]["median_ms"]
        entry["k_sweep_seg"] = {"ms": seg["ms"], "launches": seg["launches"], "algorithmic_macs": macs,
                                "achieved_tops": 2.0 * macs / (seg["ms"] * 1e-3) / 1e12 if seg["ms"] > 0 else None}
        if seg["ms"] > 0:
            entry["k_sweep_seg"]["share_of_int8_peak"] = entry["k_sweep_seg"]["achieved_tops"] / PEAK_I8
            entry["k_sweep_seg"]["share_of_call"] = seg["ms"] / entry["blocks2"]["median_ms"]
        result["shapes"][name] = entry
        print(json.dumps({name: entry}), flush=True)
        del jobs
        engine.release_workspace()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(f"[bench_matmul_blocks] wrote {args.out}")


if __name__ == "__main__":
    main()
