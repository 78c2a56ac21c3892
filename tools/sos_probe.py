"""Timing probe of k_sos_split on the ViT-B attn.v shape (32 images x 12 heads, 197 x 197 x 64): python tools/sos_probe.py [out.json]

One sweep over all rows with 1..6 and 20 candidates in the range, per instance (tuning key 12: 13 the previous kernel, 14 the
resident instance, 15 the light instance), and the 16-row slice sweep of stage A (13 the previous kernel, 0 the paired
instance), timed by the engine's launch records (HIP events around the kernel).  The table decides SOS_LIGHT_MAX in
csrc/p4v_api.hip: the largest candidate count at which the light instance still beats the resident one."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ptq4vit_amd import engine

g = torch.Generator().manual_seed(0)
b, H, S, D = 32, 12, 197, 64


def operands(M):
    A = torch.softmax(torch.randn(b, H, M, S, generator=g) * 3, -1).cuda()
    B = torch.randn(b, H, S, D, generator=g).cuda()
    out = A @ B
    return dict(A=A, B=B, out=out, grad=(torch.randn(out.shape, generator=g) * 1e-3).cuda(), A_bit=8, metric="hessian")


def time_sweep(ops, tv, crange, known, reps=5):
    engine.debug_tuning(12, tv)
    engine.debug_sos_sweep(**ops, crange=crange, known_cands=known)
    engine.stats_reset(); engine.stats_enable(True)
    for _ in range(reps):
        engine.debug_sos_sweep(**ops, crange=crange, known_cands=known)
    torch.cuda.synchronize()
    recs = [r["ms"] * 1e3 for r in engine.stats_launches() if r["kernel"] == "k_sos_split"]
    engine.stats_enable(False); engine.debug_tuning(12, 0)
    assert len(recs) == reps, recs
    return round(min(recs), 1), round(sorted(recs)[len(recs) // 2], 1)


table = {"shape": [b, H, S, S, D], "unit": "us per launch: [min, median] of 5", "all_rows": [], "slice16": {}}
full = operands(S)
for n in (1, 2, 3, 4, 5, 6, 20):
    row = {"candidates": n}
    for tv, name in ((13, "previous"), (14, "resident"), (15, "light")):
        row[name] = time_sweep(full, tv, (4, 4 + n) if n < 20 else (0, 20), n)
    table["all_rows"].append(row)
    print(row, flush=True)
sl = operands(16)
for tv, name in ((13, "previous"), (0, "paired")):
    table["slice16"][name] = time_sweep(sl, tv, None, -1)
print(table["slice16"], flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(table, f, indent=1)
