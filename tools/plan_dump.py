"""What the host side plans, as JSON -- to compare two builds of the library (P4V_LIB selects the one to load).

Without a GPU: the four *_workspace_bytes entry points over a grid of descriptors that reaches every sweep kernel family (the
small shapes of tests/sweep_plan_cases.py, the layers of ViT-B / DeiT-T / Swin-T at the sizes tests/test_hip_production_path.py
calibrates them; metrics, blocks, pruning on / off, fp32 planes -- the sizes do not depend on the bit width).  Then the dry runs of
the forward side: the Linear, MatMul and sub-block grids again with `reserved` bit 2 (the sizes of *_quant_forward alone; the
small shapes and the ViT-B layers), p4v_mlp_workspace_bytes over a small grid of fused MLP forwards and p4v_attn_workspace_bytes
over one of fused attention forwards (3 / 12 heads, 50 / 197 / 577 keys, plain / split-of-softmax p.v, 8 / 4 bit).
--gpu: also the cases of tests/sweep_plan_cases.py, pruning off and on: launch records (kernel, stage, grid_x, grid_z) in order,
p4v_launch_counters, p4v_prune_counters, and the raw bytes of the returned intervals, score tables and selections (as hex where
they are at most 16 bytes, as a sha256 prefix otherwise); then the three-round cases of tests/search_round_cases.py in each of
their modes, with the pass memo's (hits, misses) as well, and the cases of tests/pruned_pass_cases.py in theirs; last one
fused MLP and one fused attention forward (the launch record of the producer kernel, then those of the consumer's sweep); after them
the metric grid of tests/metric_grid_cases.py: the twelve shapes again, each in its own pruning setting, under the four difference
metrics the rows above do not run, with the generators' raw_grad and then with none (rows marked "grad": "none").  No timings: two
runs of the same code give the same file.

--base FILE: an earlier dump of this tool.  Where this run's workspace section and its first GPU rows equal FILE's, they are not
written again: the output names FILE, its sha256 and the number of rows found equal, and lists the rows after them.  Anything
that differs from FILE is written in full.

    python tools/plan_dump.py [--gpu] [--base FILE] [--out FILE]
"""
import argparse
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ptq4vit_amd import _lib  # noqa: E402

HESSIAN, COSINE, L2 = _lib.METRICS["hessian"], _lib.METRICS["cosine"], _lib.METRICS["L2_norm"]


def linear_descs():
    # (batch, tokens, K, N, n_V): the small cases; ViT-B x 32, DeiT-T x 16, Swin-T x 16 (blocks, patch merging, heads)
    shapes = [(2, 64, 192, 128, 1), (2, 64, 128, 128, 1), (2, 64, 1024, 64, 1), (2, 64, 1088, 64, 1), (2, 64, 192, 120, 3), (10, 65, 192, 96, 1)]
    for b, T, D in ((32, 197, 768), (16, 197, 192)):
        shapes += [(b, T, D, 3 * D, 3), (b, T, D, D, 1), (b, T, D, 4 * D, 1), (b, T, 4 * D, D, 1), (b, 1, D, 1000, 1)]
    for T, D in ((3136, 96), (784, 192), (196, 384), (49, 768)):
        shapes += [(16, T, D, 3 * D, 3), (16, T, D, D, 1), (16, T, D, 4 * D, 1), (16, T, 4 * D, D, 1)]
        if D < 768:
            shapes.append((16, T // 4, 4 * D, 2 * D, 1))
    shapes.append((16, 1, 768, 1000, 1))
    shapes += [(16, 128, 64, 96, 3), (21, 197, 64, 64, 1)]      # the smallest that plan a second tier / the quarter slice
    for (b, T, K, N, nV), metric, bits, reserved in itertools.product(shapes, (HESSIAN, COSINE, L2), (8,), (0, 8, 1)):
        for postgelu in ((0, 1) if K >= N and K >= 768 else (0,)):
            yield _lib.LinearDesc(b, T, K, N, nV, 1, 1, bits, bits, metric, 100, 3, postgelu, 0, 1, reserved)
    for (b, T, K, N, nV), metric in itertools.product(shapes[:6] + shapes[6:9], (HESSIAN, COSINE)):      # column / activation blocks
        if N % 2 == 0 and K % 2 == 0:
            yield _lib.LinearDesc(b, T, K, N, nV, 2, 2, 8, 8, metric, 100, 3, 0, 0, 1, 0)


def _mm(b, H, M, K, N, bits, metric, sos, reserved, out=None):
    d = out if out is not None else _lib.MatMulDesc()
    d.batch, d.heads, d.M, d.K, d.N = b, H, M, K, N
    for i, s in enumerate((H * M * K, M * K, K, 1)):
        d.a_stride[i] = s
    # q.k^T reads k transposed ([b][H][N][K] in memory), attn.v reads v as it lies
    for i, s in enumerate((H * N * K, N * K, 1, K) if not sos else (H * K * N, K * N, N, 1)):
        d.b_stride[i] = s
    d.A_bit, d.B_bit, d.metric, d.eq_n, d.search_round, d.sos, d.init_layerwise, d.reserved = bits, bits, metric, 100, 3, sos, 0, reserved
    return d


def matmul_shapes():
    # (batch, heads, tokens, head_dim): the small cases, ViT-B x 32, DeiT-T x 16, the four stages of Swin-T x 16 (windows of 49)
    return [(2, 2, 49, 64), (2, 2, 120, 64), (32, 12, 197, 64), (16, 3, 197, 64), (16 * 64, 3, 49, 32), (16 * 16, 6, 49, 32),
            (16 * 4, 12, 49, 32), (16, 24, 49, 32)]


def matmul_descs():
    for (b, H, T, D), metric, bits, reserved in itertools.product(matmul_shapes(), (HESSIAN, COSINE), (8,), (0, 8)):
        yield _mm(b, H, T, D, T, bits, metric, 0, reserved)
        yield _mm(b, H, T, T, D, bits, metric, 1, reserved)
        yield _mm(b, H, T, T, D, bits, metric, 0, reserved)


def matmul_blocks_descs():
    for (b, H, T, D), blocks in itertools.product(matmul_shapes()[:4], ((2, 2, 2, 3), (1, 2, 3, 1), (1, 1, 2, 2), (1, 1, 1, 1))):
        for sos in (0, 1):
            bd = _lib.MatMulBlocksDesc()
            _mm(b, H, T, T if sos else D, D if sos else T, 8, HESSIAN, sos, 0, out=bd.mm)
            bd.n_V_A, bd.n_H_A, bd.n_V_B, bd.n_H_B = ((1, 1) + blocks[2:]) if sos else blocks
            yield bd


def conv_descs():
    # (batch, channels, height, width, out channels, kernel = stride): the small case, the patch embeddings of ViT-B, DeiT-T, Swin-T
    shapes = [(2, 3, 32, 32, 16, 16), (32, 3, 224, 224, 768, 16), (16, 3, 224, 224, 192, 16), (16, 3, 224, 224, 96, 4)]
    for (b, ic, h, w, oc, k), metric, a_bit, cw, reserved in itertools.product(shapes, (HESSIAN, COSINE), (32, 8), (1, 0), (0, 8)):
        yield _lib.ConvDesc(b, ic, h, w, oc, k, k, k, k, 0, 0, 1, 1, 8, a_bit, metric, 100, 3, cw, 0, 1, reserved)


FWD = _lib.RESERVED_FORWARD_ONLY


def linear_forward_descs():
    # the small cases and the ViT-B x 32 layers (post-GELU where fc2 is); int8 planes, fp32 planes (bit 0), column / activation blocks
    shapes = [(2, 64, 192, 128, 1), (2, 64, 128, 128, 1), (2, 64, 1024, 64, 1), (2, 64, 1088, 64, 1), (2, 64, 192, 120, 3), (10, 65, 192, 96, 1),
              (32, 197, 768, 2304, 3), (32, 197, 768, 768, 1), (32, 197, 768, 3072, 1), (32, 197, 3072, 768, 1), (32, 1, 768, 1000, 1)]
    for (b, T, K, N, nV), reserved in itertools.product(shapes, (FWD, FWD | 1)):
        for postgelu in ((0, 1) if K >= N and K >= 768 else (0,)):
            yield _lib.LinearDesc(b, T, K, N, nV, 1, 1, 8, 8, HESSIAN, 100, 3, postgelu, 0, 1, reserved)
    for (b, T, K, N, nV), metric in itertools.product(shapes[:6], (HESSIAN, COSINE)):
        yield _lib.LinearDesc(b, T, K, N, nV, 2, 2, 8, 8, metric, 100, 3, 0, 0, 1, FWD)


def matmul_forward_descs():
    for (b, H, T, D), metric in itertools.product(matmul_shapes()[:3], (HESSIAN, COSINE)):
        yield _mm(b, H, T, D, T, 8, metric, 0, FWD)
        yield _mm(b, H, T, T, D, 8, metric, 1, FWD)
        yield _mm(b, H, T, T, D, 8, metric, 0, FWD)


def matmul_blocks_forward_descs():
    for bd in matmul_blocks_descs():
        bd.mm.reserved = FWD
        yield bd


def mlp_descs():
    # (batch, tokens, in, hidden): rows x in x hidden of 128 x 64 x 256, 130 x 192 x 768, ViT-B x 32; fc2 plain / post-GELU twin; n_V on fc1
    for (b, T, K, Hd), twin, nV in itertools.product(((2, 64, 64, 256), (10, 13, 192, 768), (32, 197, 768, 3072)), (0, 1), (1, 3)):
        d = _lib.MlpDesc()
        d.fc1 = _lib.LinearDesc(b, T, K, Hd, nV, 1, 1, 8, 8, HESSIAN, 100, 3, 0, 0, 1, 0)
        d.fc2 = _lib.LinearDesc(b, T, Hd, K, 1, 1, 1, 8, 8, HESSIAN, 100, 3, twin, 0, 1, 0)
        yield d


def attn_descs():
    # batch 2, head_dim 64, tokens = keys
    for H, T, sos, bits in itertools.product((3, 12), (50, 197, 577), (0, 1), (8, 4)):
        d = _lib.AttnDesc()
        _mm(2, H, T, 64, T, bits, L2, 0, FWD, out=d.qk)
        _mm(2, H, T, T, 64, bits, L2, sos, FWD, out=d.pv)
        d.scale, d.reserved = 0.125, 0
        yield d


def workspace_plan(lib):
    """per entry point: the number of descriptors, a digest of their bytes (which grid this was) and the sizes in grid order"""
    plan = {}
    for fn, descs in (("p4v_linear_workspace_bytes", linear_descs()), ("p4v_matmul_workspace_bytes", matmul_descs()),
                      ("p4v_matmul_blocks_workspace_bytes", matmul_blocks_descs()), ("p4v_conv_workspace_bytes", conv_descs()),
                      ("p4v_linear_workspace_bytes:forward", linear_forward_descs()), ("p4v_matmul_workspace_bytes:forward", matmul_forward_descs()),
                      ("p4v_matmul_blocks_workspace_bytes:forward", matmul_blocks_forward_descs()), ("p4v_mlp_workspace_bytes", mlp_descs()),
                      ("p4v_attn_workspace_bytes", attn_descs())):
        h, sizes = hashlib.sha256(), []
        for d in descs:
            h.update(bytes(d))
            sizes.append(int(getattr(lib, fn.split(":")[0])(C.byref(d))))
        plan[fn] = {"descriptors": len(sizes), "grid_sha256": h.hexdigest()[:16], "bytes": sizes}
    return plan


def _raw(t):
    """shape and digest of a result tensor's bytes; the bytes themselves (hex) where they are few: the intervals"""
    b = t.detach().cpu().contiguous().numpy().tobytes()
    return "x".join(str(n) for n in t.shape) + ":" + (b.hex() if len(b) <= 16 else hashlib.sha256(b).hexdigest()[:16])


def _runs(recs):
    """launch records in order, equal neighbours folded: [kernel, stage, grid_x, grid_z, count]"""
    out = []
    for r in recs:
        if out and out[-1][:4] == list(r):
            out[-1][4] += 1
        else:
            out.append(list(r) + [1])
    return out


def _fused_mlp(eng, prune):
    """130 rows x 192 x 768, n_V = 3 on fc1, fc2 the post-GELU twin"""
    import torch
    g = torch.Generator().manual_seed(21)
    x = torch.randn(10, 13, 192, generator=g).cuda()
    layer = lambda n, k, n_V, iv, **kw: dict(weight=(torch.randn(n, k, generator=g) * 0.05).cuda(), bias=(torch.randn(n, generator=g) * 0.1).cuda(),
                                             w_interval=torch.full((n_V,), 0.002), a_interval=torch.tensor([iv]), w_bit=8, a_bit=8, n_V=n_V, **kw)
    return [eng.mlp_quant_forward(x=x, fc1=layer(768, 192, 3, 0.03), fc2=layer(192, 768, 1, 0.02, postgelu=True))]


def _fused_attn(eng, prune):
    """2 x 3 heads, 50 queries and keys, head_dim 64, p.v split-of-softmax"""
    import torch
    g = torch.Generator().manual_seed(22)
    q, k, v = (torch.randn(2, 3, 50, 64, generator=g).cuda() for _ in range(3))
    iv = lambda val, n=3: torch.full((n,), val)
    return [eng.attn_quant_forward(q=q, kT=k.transpose(-2, -1), v=v, scale=0.125, qk=dict(A_interval=iv(0.03), B_interval=iv(0.03), A_bit=8, B_bit=8),
                                   pv=dict(A_interval=iv(0.01 / 127, 1), B_interval=iv(0.03), A_bit=8, B_bit=8, sos=True, split=iv(0.01, 1)))]


def gpu_plan():
    from ptq4vit_amd import engine
    from tests.sweep_plan_cases import CASES, run_case
    rows = []
    for (name, run, _), prune in itertools.product(CASES, (False, True)):
        res, recs, launches, pruned = run_case(engine, run, prune)
        rows.append({"case": name, "prune": int(prune), "records": _runs(recs),
                     "launch_counters": [launches[k] for k in ("asked", "issued", "rounds", "groups")],
                     "prune_counters": [pruned[k] for k in ("staged", "staged_no_survivors", "kept_full_sweep", "not_eligible")],
                     "results": [_raw(t) for t in res]})
        engine.release_workspace()
    from tests.search_round_cases import CASES as ROUND_CASES, MODES, run_case as run_rounds
    for (name, run), mode in itertools.product(ROUND_CASES, MODES):
        r = run_rounds(engine, run, mode)
        rows.append({"case": name, "mode": mode, "records": _runs(r["records"]),
                     "launch_counters": [r["launch_counters"][k] for k in ("asked", "issued", "rounds", "groups")],
                     "prune_counters": [r["prune_counters"][k] for k in ("staged", "staged_no_survivors", "kept_full_sweep", "not_eligible")],
                     "memo": list(r["memo"]), "results": [_raw(t) for t in r["intervals"] + r["tables"]]})
        engine.release_workspace()
    from tests.pruned_pass_cases import CASES as PRUNED_CASES, modes_of
    for name, run in PRUNED_CASES:
        for mode in modes_of(name):
            r = run_rounds(engine, run, mode)
            rows.append({"case": name, "mode": mode, "records": _runs(r["records"]),
                         "launch_counters": [r["launch_counters"][k] for k in ("asked", "issued", "rounds", "groups")],
                         "prune_counters": [r["prune_counters"][k] for k in ("staged", "staged_no_survivors", "kept_full_sweep", "not_eligible")],
                         "memo": list(r["memo"]), "results": [_raw(t) for t in r["intervals"] + r["tables"]]})
            engine.release_workspace()
    for name, run in (("fused_mlp_130x192x768_twin", _fused_mlp), ("fused_attn_2x3x50x64_sos", _fused_attn)):
        res, recs, launches, _ = run_case(engine, run, False)
        rows.append({"case": name, "records": _runs(recs), "launch_counters": [launches[k] for k in ("asked", "issued", "rounds", "groups")],
                     "results": [_raw(t) for t in res]})
        engine.release_workspace()
    from tests.metric_grid_cases import CASES as METRIC_CASES
    for name, metric, run, pruned in METRIC_CASES:
        res, recs, launches, counters = run_case(engine, run, pruned)
        rows.append({"case": name, "metric": metric, "prune": int(pruned), "records": _runs(recs),
                     "launch_counters": [launches[k] for k in ("asked", "issued", "rounds", "groups")],
                     "prune_counters": [counters[k] for k in ("staged", "staged_no_survivors", "kept_full_sweep", "not_eligible")],
                     "memo": list(launches["memo"]), "results": [_raw(t) for t in res]})
        engine.release_workspace()
    # ... and once more without a raw_grad: none of these metrics reads it, so every row must repeat the one above
    for name, metric, run, pruned in METRIC_CASES:
        res, recs, launches, counters = run_case(engine, run, pruned, grad="none")
        rows.append({"case": name, "metric": metric, "grad": "none", "prune": int(pruned), "records": _runs(recs),
                     "launch_counters": [launches[k] for k in ("asked", "issued", "rounds", "groups")],
                     "prune_counters": [counters[k] for k in ("staged", "staged_no_survivors", "kept_full_sweep", "not_eligible")],
                     "memo": list(launches["memo"]), "results": [_raw(t) for t in res]})
        engine.release_workspace()
    return rows


def _against_base(doc, path):
    """doc with what equals the earlier dump `path` replaced by a reference to it (see --base)"""
    base = json.load(open(path))
    ref = {"file": os.path.basename(path), "sha256": hashlib.sha256(open(path, "rb").read()).hexdigest()[:16], "workspace_equal": doc["workspace"] == {k: v for k, v in base.items() if k not in ("gpu", "base")}}
    rows, old = doc.get("gpu", []), base.get("gpu", [])
    if rows[:len(old)] == old:
        ref["gpu_rows_equal"] = len(old)
        rows = rows[len(old):]
    return {"base": ref, "workspace": {} if ref["workspace_equal"] else doc["workspace"], "gpu": rows}


def _lines(doc):
    """compact JSON, one entry point / one case per line, the size lists wrapped"""
    out = ["{"]
    if "base" in doc:
        out.append(' "base": %s,' % json.dumps(doc["base"]))
    for fn, e in doc["workspace"].items():
        sizes = e["bytes"]
        out.append(' "%s": {"descriptors": %d, "grid_sha256": "%s", "bytes": [' % (fn, e["descriptors"], e["grid_sha256"]))
        out += ["  " + ", ".join(str(n) for n in sizes[i:i + 16]) + ("," if i + 16 < len(sizes) else "") for i in range(0, len(sizes), 16)]
        out.append(" ]},")
    rows = doc.get("gpu", [])
    out.append(' "gpu": [')
    out += ["  " + json.dumps(r) + ("," if i + 1 < len(rows) else "") for i, r in enumerate(rows)]
    out += [" ]", "}"]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gpu", action="store_true", help="also run the small cases on cuda:0")
    ap.add_argument("--base", default=None, help="an earlier dump: what equals it is referred to, not written again")
    ap.add_argument("--out", default=None, help="write the JSON here instead of stdout")
    a = ap.parse_args()
    doc = {"workspace": workspace_plan(_lib.load())}
    if a.gpu:
        doc["gpu"] = gpu_plan()
    text = _lines(_against_base(doc, a.base) if a.base else doc)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
