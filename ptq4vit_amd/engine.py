"""Glue between torch tensors and the C ABI: pointers, stream, workspace, candidate tables.

Nothing here computes: every calibration number comes out of libptq4vit_hip.so.
"""
import ctypes as C

import torch

from . import _lib

_workspace = {}
_mult_cache = {}


def _require_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"ptq4vit_amd: {what} must live on the GPU (got {t.device}); the calibration path has no CPU fallback")


def device_of(*tensors):
    for t in tensors:
        if t is not None and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("ptq4vit_amd: no GPU visible -- the HIP calibration engine needs an MI355X (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def to_dev(t, dev):
    """fp32 tensor on `dev` (the reference keeps caches on the host and re-uploads per search call)."""
    if t is None:
        return None
    return t.detach().to(device=dev, dtype=torch.float32)


def workspace(dev, nbytes, slot=0):
    """Scratch for one calibration call; one buffer per (device, stream, member of a group) so that searches running on
    different streams, and the members of a p4v_calibrate_group call, never share scratch."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream, slot)
    ws = _workspace.get(key)
    if ws is None or ws.numel() < nbytes:
        _workspace.pop(key, None)
        ws = None           # (the old buffer goes back to torch's pool BEFORE the new one is taken from it)
        pad = (1 << 20) if slot == "arena" else int(nbytes * 0.05) + (1 << 20)    # an arena is sized by its caller's budget
        ws = torch.empty(int(nbytes) + pad, dtype=torch.uint8, device=dev)
        _workspace[key] = ws
    return ws


def release_workspace():
    _workspace.clear()


def workspace_bytes(dev=None):
    """Bytes of scratch buffers the engine keeps alive between calls (per device, stream and group member)."""
    return sum(ws.numel() for (d, _s, _slot), ws in _workspace.items() if dev is None or d == dev)


def workspace_held(dev, slot=0):
    """Size of the scratch buffer already kept for (current stream of `dev`, `slot`); 0 if none."""
    ws = _workspace.get((dev, torch.cuda.current_stream(dev).cuda_stream, slot))
    return 0 if ws is None else ws.numel()


_side_streams = {}


def side_streams(dev, n):
    """`n` persistent side streams of `dev` (the calibrator searches several modules at a time).  Persistent because
    the scratch buffers are keyed by stream: fresh streams per calibration would strand one scratch buffer each."""
    lst = _side_streams.setdefault(dev, [])
    while len(lst) < n:
        lst.append(torch.cuda.Stream(device=dev))
    return lst[:n]


def candidate_multipliers(eq_alpha, eq_beta, eq_n, dev):
    """Reference quant_layers/linear.py:544: python-float grid rounded to fp32 (eq_n+1 entries)."""
    key = (float(eq_alpha), float(eq_beta), int(eq_n), str(dev))
    t = _mult_cache.get(key)
    if t is None:
        t = torch.tensor([eq_alpha + i * (eq_beta - eq_alpha) / eq_n for i in range(eq_n + 1)],
                         dtype=torch.float32).to(dev)
        _mult_cache[key] = t
    return t


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream_ptr(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def metric_id(name):
    if name not in _lib.METRICS:
        raise NotImplementedError(f"metric {name} not implemented!")
    return _lib.METRICS[name]


class Job:
    """One prepared p4v_*_calibrate call: descriptor, device tensors (kept alive until the results are taken), outputs,
    workspace size.  `run_job` makes the call; `calibrate_group` makes the calls of many jobs as ONE p4v_calibrate_group."""
    __slots__ = ("kind", "name", "desc", "inputs", "mult", "outputs", "need", "dev", "scores", "best")

    def __init__(self, kind, name, desc, inputs, mult, outputs, need, dev, scores=None, best=None):
        self.kind, self.name, self.desc, self.inputs, self.mult = kind, name, desc, inputs, mult
        self.outputs, self.need, self.dev, self.scores, self.best = outputs, need, dev, scores, best


def _need(fn, desc, what):
    need = fn(C.byref(desc))
    if need == 0:
        _lib.check(-1 if not _lib.load().p4v_last_error() else -2, what)
    return need


def run_job(job):
    """The single-module call (p4v_linear_calibrate / p4v_matmul_calibrate / p4v_conv_calibrate) on the current stream."""
    lib = _lib.load()
    ws = workspace(job.dev, job.need)
    with torch.cuda.device(job.dev):
        rc = getattr(lib, job.name)(C.byref(job.desc), *[ptr(t) for t in job.inputs], ptr(job.mult), *[ptr(t) for t in job.outputs],
                                    ptr(job.scores), ptr(job.best), ptr(ws), ws.numel(), stream_ptr(job.dev))
    _lib.check(rc, job.name)
    return job


def calibrate_group(jobs, inputs_ready=None):
    """calibration_step2 of all `jobs` in ONE p4v_calibrate_group call on the current stream: the members search in lock
    step, every kernel launch of the same kind is issued once for all of them.  Results bit-identical to run_job on each.
    `inputs_ready`: a torch.cuda.Event recorded behind the capture passes that fill the jobs' captured tensors -- the call
    starts at once with the work that needs none of them (weight abs-max, candidate tables, the candidate planes of the
    weights) and makes its stream wait for the event where the first captured tensor is read.  None: the tensors are ready."""
    jobs = list(jobs)
    if not jobs:
        return jobs
    lib = _lib.load()
    dev = jobs[0].dev
    arr = (_lib.GroupJob * len(jobs))()
    # ONE arena per (device, stream) for the scratch of all members, carved by offset: the call's scratch is exactly the sum of
    # the members' needs whatever mixture the previous calls on this stream held (a buffer per member slot, each grown to the
    # largest member it ever saw, added up to more than the budget of a 128-image configuration and fragmented torch's pool).
    offs, total = [], 0
    for job in jobs:
        offs.append(total)
        total += (int(job.need) + 4095) & ~4095
    arena = workspace(dev, total, slot="arena")
    base = arena.data_ptr()
    keep = [arena]
    for i, job in enumerate(jobs):
        if job.dev != dev:
            raise ValueError("calibrate_group: every member must live on the same device")
        if job.scores is not None:
            raise ValueError("calibrate_group: score tables are only returned by the single-module calls")
        g = arr[i]
        g.kind, g.status, g.desc = job.kind, 0, C.cast(C.pointer(job.desc), C.c_void_p)
        ins = list(job.inputs) + [None] * (5 - len(job.inputs))
        for k in range(5):
            g.inp[k] = ins[k].data_ptr() if ins[k] is not None else None
        g.mult = job.mult.data_ptr()
        outs = list(job.outputs) + [None] * (3 - len(job.outputs))
        for k in range(3):
            g.out[k] = outs[k].data_ptr() if outs[k] is not None else None
        g.workspace, g.workspace_bytes = base + offs[i], int(job.need)
    with torch.cuda.device(dev):
        ev = C.c_void_p(inputs_ready.cuda_event) if inputs_ready is not None else C.c_void_p(0)
        rc = lib.p4v_calibrate_group(arr, len(jobs), stream_ptr(dev), ev)
    _lib.check(rc, "p4v_calibrate_group")
    del keep
    return jobs


def launch_counters(reset=False):
    """Process-wide launch counters (p4v_launch_counters): launches the calibration path asked for, launches issued to the
    GPU (a grouped launch counts once), issue rounds of the groups, group calls."""
    out = (C.c_int64 * 4)()
    _lib.check(_lib.load().p4v_launch_counters(out, int(bool(reset))), "p4v_launch_counters")
    return dict(zip(("asked", "issued", "rounds", "groups"), (int(v) for v in out)))


def linear_job(*, weight, bias, x, out, grad, w_bit, a_bit, metric, eq_alpha, eq_beta, eq_n, search_round,
               n_V, n_H, n_a, init_layerwise=False, postgelu=False, want_scores=False, force_f32=False, memoize=True,
               prune=True):
    lib = _lib.load()
    dev = device_of(x, weight)
    weight, bias, x, out, grad = (to_dev(t, dev) for t in (weight, bias, x, out, grad))
    x = x.contiguous(); out = out.contiguous(); weight = weight.contiguous()
    grad = grad.contiguous() if grad is not None else None
    batch = x.shape[0]
    K = x.shape[-1]
    tokens = x.numel() // (batch * K)
    N = weight.shape[0]
    d = _lib.LinearDesc(batch, tokens, K, N, n_V, n_H, n_a, w_bit, a_bit, metric_id(metric), eq_n, search_round,
                        int(postgelu), int(init_layerwise), int(bias is not None),
                        (_lib.RESERVED_FP32_PLANES if force_f32 else 0) | (0 if memoize else _lib.RESERVED_NO_MEMO) |
                        (0 if prune else _lib.RESERVED_NO_PRUNE))
    need = _need(lib.p4v_linear_workspace_bytes, d, "p4v_linear_workspace_bytes")
    mult = candidate_multipliers(eq_alpha, eq_beta, eq_n, dev)
    w_iv = torch.empty(n_V * n_H, dtype=torch.float32, device=dev)
    a_iv = torch.empty(n_a, dtype=torch.float32, device=dev)
    scores = torch.zeros(search_round, 2, eq_n, n_V, dtype=torch.float32, device=dev) if want_scores else None
    best = torch.zeros(search_round, 2, n_V, dtype=torch.int32, device=dev) if want_scores else None
    return Job(_lib.JOB_LINEAR, "p4v_linear_calibrate", d, (weight, bias, x, out, grad), mult, (w_iv, a_iv), need, dev, scores, best)


def linear_calibrate(**kw):
    """Run calibration_step2 of a (post-GELU) Linear on the GPU.  Returns (w_interval[n_V*n_H], a_interval[n_a], scores, best)."""
    job = run_job(linear_job(**kw))
    return job.outputs[0], job.outputs[1], job.scores, job.best


def linear_quant_forward(*, weight, bias, x, w_interval, a_interval, w_bit, a_bit, n_V, n_H, n_a, postgelu=False):
    """quant_forward of a calibrated (post-GELU) Linear as one int8 MFMA GEMM (p4v_linear_quant_forward)."""
    lib = _lib.load()
    dev = device_of(x, weight)
    weight, bias, x = (to_dev(t, dev) for t in (weight, bias, x))
    x = x.contiguous(); weight = weight.contiguous()
    batch, K = x.shape[0], x.shape[-1]
    tokens = x.numel() // (batch * K)
    N = weight.shape[0]
    d = _lib.LinearDesc(batch, tokens, K, N, n_V, n_H, n_a, w_bit, a_bit, metric_id("L2_norm"), 1, 1,
                        int(postgelu), 0, int(bias is not None), _lib.RESERVED_FORWARD_ONLY)
    need = lib.p4v_linear_workspace_bytes(C.byref(d))
    if need == 0:
        _lib.check(-2, "p4v_linear_workspace_bytes")
    ws = workspace(dev, need)
    w_iv = to_dev(w_interval, dev).reshape(-1).contiguous()
    a_iv = to_dev(a_interval, dev).reshape(-1).contiguous()
    out = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.p4v_linear_quant_forward(C.byref(d), ptr(weight), ptr(bias), ptr(x), ptr(w_iv), ptr(a_iv), ptr(out),
                                          ptr(ws), ws.numel(), stream_ptr(dev))
    _lib.check(rc, "p4v_linear_quant_forward")
    return out


def _mlp_layer_desc(batch, tokens, layer):
    w = layer["weight"]
    return _lib.LinearDesc(batch, tokens, w.shape[1], w.shape[0], layer["n_V"], layer.get("n_H", 1), layer.get("n_a", 1),
                           layer["w_bit"], layer["a_bit"], metric_id("L2_norm"), 1, 1, int(bool(layer.get("postgelu", False))), 0,
                           int(layer.get("bias") is not None), _lib.RESERVED_FORWARD_ONLY)


def _fused_forward(kind, d, tensors, dev, res, want_planes, z=None):
    """The tail of the fused forwards (`kind`: mlp / attn / wattn): p4v_<kind>_workspace_bytes, the workspace, the checked call
    p4v_<kind>_quant_forward(d, *tensors, workspace, its size, stream) -- wattn: `tensors` maps the members of its
    p4v_wattn_tensors record, in which the workspace and its size travel too.  Returns the tuple `res` -- its one member alone --,
    with `want_planes` followed by the int8 plane(s) p4v_debug_<kind>_planes (wattn: attn's) locates in the workspace:
    [rows][cols] each, or `z` of [rows / z][cols]."""
    lib = _lib.load()
    ws = workspace(dev, _need(getattr(lib, f"p4v_{kind}_workspace_bytes"), d, f"p4v_{kind}_workspace_bytes"))
    with torch.cuda.device(dev):
        if kind == "wattn":
            rec = _lib.WattnTensors(**{n: ptr(t) for n, t in tensors.items()}, ws=ptr(ws), ws_bytes=ws.numel())
            rc = lib.p4v_wattn_quant_forward(C.byref(d), C.byref(rec), stream_ptr(dev))
        else:
            rc = getattr(lib, f"p4v_{kind}_quant_forward")(C.byref(d), *[ptr(t) for t in tensors], ptr(ws), ws.numel(), stream_ptr(dev))
    _lib.check(rc, f"p4v_{kind}_quant_forward")
    if want_planes:
        info = (C.c_uint64 * 5)()
        kind = "attn" if kind == "wattn" else kind
        _lib.check(getattr(lib, f"p4v_debug_{kind}_planes")(info), f"p4v_debug_{kind}_planes")
        off1, off2, rows, cols, twin = (int(v) for v in info)
        shape = (rows, cols) if z is None else (z, rows // z, cols)
        take = lambda off: ws[off:off + rows * cols].view(torch.int8).reshape(shape).clone()
        res += ((take(off1), take(off2)) if twin else (take(off1),),)
    return res[0] if len(res) == 1 else res


def mlp_quant_forward(*, x, fc1, fc2, want_hidden=False, want_planes=False):
    """fc2(GELU(fc1(x))) of two calibrated Linear layers in quant_forward, fused (p4v_mlp_quant_forward): fc1's int8 GEMM ends
    in the exact GELU and fc2's activation quantiser and writes fc2's int8 plane(s); no fp32 hidden tensor in between.
    `fc1` / `fc2`: dicts with weight, bias (or None), w_interval, a_interval (fc2: the positive range), w_bit, a_bit, n_V and
    optionally n_H, n_a, postgelu (fc2: the post-GELU twin).  Returns out, or (out, hidden) with `want_hidden` -- the fp32 GELU
    output the planes were quantised from --, with `want_planes` also the padded int8 plane(s) as the call left them in its
    workspace (a tuple of one or two [rows_padded][cols_padded] tensors; for the tests)."""
    dev = device_of(x, fc1["weight"])
    x = to_dev(x, dev).contiguous()
    batch, K = x.shape[0], x.shape[-1]
    tokens = x.numel() // (batch * K)
    t = {}
    for name, layer in (("fc1", fc1), ("fc2", fc2)):
        t[name] = (to_dev(layer["weight"], dev).contiguous(), to_dev(layer.get("bias"), dev),
                   to_dev(layer["w_interval"], dev).reshape(-1).contiguous(), to_dev(layer["a_interval"], dev).reshape(-1).contiguous())
    d = _lib.MlpDesc(_mlp_layer_desc(batch, tokens, fc1), _mlp_layer_desc(batch, tokens, fc2))
    hidden_n, out_n = fc1["weight"].shape[0], fc2["weight"].shape[0]
    out = torch.empty(x.shape[:-1] + (out_n,), dtype=torch.float32, device=dev)
    hidden = torch.empty(x.shape[:-1] + (hidden_n,), dtype=torch.float32, device=dev) if want_hidden else None
    (w1, b1, w1_iv, a1_iv), (w2, b2, w2_iv, a2_iv) = t["fc1"], t["fc2"]
    return _fused_forward("mlp", d, (w1, b1, w2, b2, x, w1_iv, a1_iv, w2_iv, a2_iv, out, hidden), dev,
                          (out, hidden) if want_hidden else (out,), want_planes)


def _attn_matmul_desc(d, A_shape, A_stride, B, side, what, who="attn_quant_forward"):
    """One p4v_matmul_desc of a p4v_attn_desc / p4v_wattn_desc; `side`: the dict engine.attn_quant_forward takes per MatMul."""
    if has_blocks(side.get("blocks")):
        raise NotImplementedError(f"{who}: {what} has row / column sub-blocks (the fused forward is head-wise)")
    d.batch, d.heads, d.M, d.K, d.N = A_shape[0], A_shape[1], A_shape[2], A_shape[3], B.shape[3]
    for i in range(4):
        d.a_stride[i] = A_stride[i]
        d.b_stride[i] = B.stride(i)
    d.A_bit, d.B_bit, d.metric, d.eq_n, d.search_round = side["A_bit"], side["B_bit"], metric_id("L2_norm"), 1, 1
    d.sos, d.init_layerwise, d.reserved = int(bool(side.get("sos", False))), 0, _lib.RESERVED_FORWARD_ONLY


def _attn_call(who, q, kT, v, qk, pv, want_probs, desc):
    """What attn_quant_forward and window_attn_quant_forward share: the operands on the device, the two p4v_matmul_desc of
    `desc`, the checked interval tensors, the outputs.  Returns (dev, q, kT, v, (qk_A, qk_B, pv_A, pv_B, split), out, probs)."""
    dev = device_of(q, kT, v)
    q, kT, v = to_dev(q, dev), to_dev(kT, dev), to_dev(v, dev)
    b, H, M, _ = q.shape
    N, Dv = kT.shape[3], v.shape[3]
    if qk.get("sos", False):
        raise NotImplementedError(f"{who}: q k^T is no split-of-softmax operand (sos belongs on p v)")
    _attn_matmul_desc(desc.qk, q.shape, q.stride(), kT, qk, "q k^T", who)
    _attn_matmul_desc(desc.pv, (b, H, M, v.shape[2]), (H * M * v.shape[2], M * v.shape[2], v.shape[2], 1), v, pv, "p v", who)
    sos = bool(pv.get("sos", False))
    flat = lambda t: to_dev(t, dev).reshape(-1).contiguous()
    qk_A, qk_B, pv_A, pv_B = flat(qk["A_interval"]), flat(qk["B_interval"]), flat(pv["A_interval"]), flat(pv["B_interval"])
    if qk_A.numel() != H or qk_B.numel() != H or pv_B.numel() != H or pv_A.numel() != (1 if sos else H):
        raise ValueError(f"{who}: interval tensors must hold one value per head (the split-of-softmax A: one)")
    sp = flat(pv["split"]) if sos else None
    out = torch.empty(b, H, M, Dv, dtype=torch.float32, device=dev)
    probs = torch.empty(b, H, M, N, dtype=torch.float32, device=dev) if want_probs else None
    return dev, q, kT, v, (qk_A, qk_B, pv_A, pv_B, sp), out, probs


def attn_quant_forward(*, q, kT, v, scale, qk, pv, want_probs=False, want_planes=False):
    """matmul2(softmax(matmul1(q, kT) * scale, -1), v) of the two calibrated MatMuls of an attention block in quant_forward,
    fused (p4v_attn_quant_forward): matmul1's int8 GEMM keeps the scores in registers, takes the softmax and matmul2's A
    quantiser and writes matmul2's int8 plane(s); no fp32 score or probability tensor in between.
    q [B][H][M][D], kT [B][H][D][N], v [B][H][N][Dv]: read through their strides (views are not copied).  `qk` / `pv`: dicts
    with A_interval, B_interval ([heads] each; the split-of-softmax pv: its scalar A_interval), A_bit, B_bit, optionally
    blocks (anything but (1, 1, 1, 1) is refused), and for `pv` sos, split.  Returns out [B][H][M][Dv], or (out, probs) with
    `want_probs` -- the fp32 probabilities the planes were quantised from --, with `want_planes` also the padded int8
    plane(s) as the call left them in its workspace (a tuple of one or two [B*H][rows_padded][cols_padded] tensors; for the
    tests)."""
    d = _lib.AttnDesc()
    dev, q, kT, v, (qk_A, qk_B, pv_A, pv_B, sp), out, probs = _attn_call("attn_quant_forward", q, kT, v, qk, pv, want_probs, d)
    d.scale, d.reserved = float(scale), 0
    return _fused_forward("attn", d, (q, kT, v, qk_A, qk_B, pv_A, pv_B, sp, out, probs), dev, (out, probs) if want_probs else (out,),
                          want_planes, z=q.shape[0] * q.shape[1])


def window_attn_quant_forward(*, q, kT, v, bias, mask=None, qk, pv, want_probs=False, want_planes=False):
    """matmul2(softmax(matmul1(q, kT) + bias (+ mask), -1), v) of the two calibrated MatMuls of a window attention block
    (models.WindowAttention) in quant_forward, fused (p4v_wattn_quant_forward): attn_quant_forward's chain with the window
    arithmetic between matmul1 and the softmax.  `q` arrives ALREADY SCALED, as the module hands it to matmul1.
    q [B_][H][N][D], kT [B_][H][D][N], v [B_][H][N][Dv] (B_ = images * windows, windows innermost; views are not copied); bias
    [H][N][N]; mask None or [nW][N][N] with B_ % nW == 0, added to window (b_ % nW) of every image and head; -inf entries
    behave as in torch.  Checks, `qk` / `pv`, want_probs, want_planes and the returned values: as attn_quant_forward."""
    d = _lib.WattnDesc()
    dev, q, kT, v, (qk_A, qk_B, pv_A, pv_B, sp), out, probs = _attn_call("window_attn_quant_forward", q, kT, v, qk, pv, want_probs, d)
    b, H, M, _ = q.shape
    N = kT.shape[3]
    bias = to_dev(bias, dev).contiguous()
    if tuple(bias.shape) != (H, M, N):
        raise ValueError(f"window_attn_quant_forward: bias {tuple(bias.shape)} is not [heads][M][N] = {(H, M, N)}")
    if mask is not None:
        mask = to_dev(mask, dev).contiguous()
        if mask.dim() != 3 or tuple(mask.shape[1:]) != (M, N):
            raise ValueError(f"window_attn_quant_forward: mask {tuple(mask.shape)} is not [windows][M][N] = [*]{(M, N)}")
    d.n_windows, d.has_mask = (1 if mask is None else mask.shape[0]), int(mask is not None)
    tensors = dict(q=q, kT=kT, v=v, bias=bias, mask=mask, qk_A_interval=qk_A, qk_B_interval=qk_B, pv_A_interval=pv_A, pv_B_interval=pv_B,
                   split=sp, out=out, probs=probs)
    return _fused_forward("wattn", d, tensors, dev, (out, probs) if want_probs else (out,), want_planes, z=b * H)


def qkv_attn_quant_forward(*, x, qkv, scale, qk, pv, want_qkv=False, want_probs=False, want_planes=False):
    """matmul2(softmax(matmul1(q, kT) * scale, -1), v) with q, kT, v the head slices of qkv(x), all three modules calibrated and
    in quant_forward, fused (p4v_qkv_attn_quant_forward): the qkv layer's int8 GEMM quantises its output with the quantisers of
    the MatMul operands and writes their int8 planes; no fp32 qkv tensor, no permute copy and no pack of q, kT, v in between.
    x [B][N][in_features]; `qkv`: a Linear dict as in mlp_quant_forward (weight [3 * H * D][in_features]); `qk` / `pv`: as in
    attn_quant_forward -- the head count is the length of qk's A_interval.  Returns out [B][H][N][D]; then, as asked for, the
    fp32 qkv tensor [B][N][3 * H * D] the planes were quantised from (`want_qkv`), the probabilities [B][H][N][N]
    (`want_probs`) and the padded int8 planes as the call left them in its workspace (`want_planes`; for the tests): a tuple
    (Q [B*H][Mp][K1p], Kt [B*H][Np][K1p], V [B*H][NpB][Kp], P1[, P2] [B*H][Mp][Kp])."""
    who = "qkv_attn_quant_forward"
    lib = _lib.load()
    dev = device_of(x, qkv["weight"])
    x = to_dev(x, dev).contiguous()
    if x.dim() != 3:
        raise ValueError(f"{who}: x {tuple(x.shape)} is not [batch][tokens][in_features]")
    B, N, _ = x.shape
    w = to_dev(qkv["weight"], dev).contiguous()
    bias = to_dev(qkv.get("bias"), dev)
    flat = lambda t: to_dev(t, dev).reshape(-1).contiguous()
    qk_A, qk_B, pv_A, pv_B = flat(qk["A_interval"]), flat(qk["B_interval"]), flat(pv["A_interval"]), flat(pv["B_interval"])
    H = qk_A.numel()
    sos = bool(pv.get("sos", False))
    if qk.get("sos", False):
        raise NotImplementedError(f"{who}: q k^T is no split-of-softmax operand (sos belongs on p v)")
    if qk_B.numel() != H or pv_B.numel() != H or pv_A.numel() != (1 if sos else H):
        raise ValueError(f"{who}: interval tensors must hold one value per head (the split-of-softmax A: one)")
    if w.shape[0] % (3 * H):
        raise ValueError(f"{who}: qkv's out_features = {w.shape[0]} is not 3 x {H} heads x head_dim")
    D = w.shape[0] // (3 * H)
    d = _lib.QkvAttnDesc()
    d.qkv = _mlp_layer_desc(B, N, qkv)
    # (the operand strides are not read: no fp32 q, kT, v exists; filled as the contiguous tensors would have them)
    q_shape, kT_shape, v_shape = (B, H, N, D), (B, H, D, N), (B, H, N, D)
    cont = lambda s: (s[1] * s[2] * s[3], s[2] * s[3], s[3], 1)
    like = lambda s: torch.empty(s, device="meta")
    _attn_matmul_desc(d.qk, q_shape, cont(q_shape), like(kT_shape), qk, "q k^T", who)
    _attn_matmul_desc(d.pv, (B, H, N, N), cont((B, H, N, N)), like(v_shape), pv, "p v", who)
    d.scale, d.reserved = float(scale), 0
    sp = flat(pv["split"]) if sos else None
    out = torch.empty(B, H, N, D, dtype=torch.float32, device=dev)
    qkv_out = torch.empty(B, N, w.shape[0], dtype=torch.float32, device=dev) if want_qkv else None
    probs = torch.empty(B, H, N, N, dtype=torch.float32, device=dev) if want_probs else None
    ws = workspace(dev, _need(lib.p4v_qkv_attn_workspace_bytes, d, "p4v_qkv_attn_workspace_bytes"))
    tensors = dict(x=x, w=w, bias=bias, w_interval=flat(qkv["w_interval"]), a_interval=flat(qkv["a_interval"]), qk_A_interval=qk_A,
                   qk_B_interval=qk_B, pv_A_interval=pv_A, pv_B_interval=pv_B, split=sp, out=out, qkv_out=qkv_out, probs=probs)
    with torch.cuda.device(dev):
        rec = _lib.QkvAttnTensors(**{n: ptr(t) for n, t in tensors.items()}, ws=ptr(ws), ws_bytes=ws.numel())
        rc = lib.p4v_qkv_attn_quant_forward(C.byref(d), C.byref(rec), stream_ptr(dev))
    _lib.check(rc, "p4v_qkv_attn_quant_forward")
    res = (out,) + ((qkv_out,) if want_qkv else ()) + ((probs,) if want_probs else ())
    if want_planes:
        info = (C.c_uint64 * 9)()
        _lib.check(lib.p4v_debug_qkv_planes(info), "p4v_debug_qkv_planes")
        off_q, off_k, off_v, Z, rows_q, rows_k, ld_qk, rows_v, ld_v = (int(v) for v in info)
        take = lambda off, rows, ld: ws[off:off + Z * rows * ld].view(torch.int8).reshape(Z, rows, ld).clone()
        planes = (take(off_q, rows_q, ld_qk), take(off_k, rows_k, ld_qk), take(off_v, rows_v, ld_v))
        info = (C.c_uint64 * 5)()
        _lib.check(lib.p4v_debug_attn_planes(info), "p4v_debug_attn_planes")
        off1, off2, rows, cols, twin = (int(v) for v in info)
        planes += tuple(take(off, rows // Z, cols) for off in ((off1, off2) if twin else (off1,)))
        res += (planes,)
    return res[0] if len(res) == 1 else res


def matmul_quant_forward(*, A, B, A_interval, B_interval, split, A_bit, B_bit, sos=False):
    """quant_forward of a calibrated MatMul (head-wise intervals; optional split-of-softmax twin on A)."""
    lib = _lib.load()
    dev = device_of(A, B)
    A, B = to_dev(A, dev), to_dev(B, dev)
    b, H, M, K = A.shape
    N = B.shape[3]
    d = _lib.MatMulDesc()
    d.batch, d.heads, d.M, d.K, d.N = b, H, M, K, N
    for i in range(4):
        d.a_stride[i] = A.stride(i)
        d.b_stride[i] = B.stride(i)
    d.A_bit, d.B_bit, d.metric, d.eq_n, d.search_round = A_bit, B_bit, metric_id("L2_norm"), 1, 1
    d.sos, d.init_layerwise, d.reserved = int(sos), 0, _lib.RESERVED_FORWARD_ONLY
    need = lib.p4v_matmul_workspace_bytes(C.byref(d))
    if need == 0:
        _lib.check(-2, "p4v_matmul_workspace_bytes")
    ws = workspace(dev, need)
    A_iv = to_dev(A_interval, dev).reshape(-1).contiguous()
    B_iv = to_dev(B_interval, dev).reshape(-1).contiguous()
    sp = to_dev(split, dev).reshape(-1).contiguous() if sos else None
    out = torch.empty(b, H, M, N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.p4v_matmul_quant_forward(C.byref(d), ptr(A), ptr(B), ptr(A_iv), ptr(B_iv), ptr(sp), ptr(out),
                                          ptr(ws), ws.numel(), stream_ptr(dev))
    _lib.check(rc, "p4v_matmul_quant_forward")
    return out


def has_blocks(blocks):
    """`blocks` = (n_V_A, n_H_A, n_V_B, n_H_B) of a MatMul: does any operand have row / column sub-blocks?"""
    return blocks is not None and tuple(int(n) for n in blocks) != (1, 1, 1, 1)


def _matmul_desc(A, B, A_bit, B_bit, metric, eq_n, search_round, sos, init_layerwise, reserved, blocks=None, wrap=False):
    """p4v_matmul_desc of the operands -- wrapped in a p4v_matmul_blocks_desc when `blocks` has a count above 1 or `wrap` is
    set (returns the descriptor to pass and its p4v_matmul_desc part)."""
    bd = _lib.MatMulBlocksDesc() if (wrap or has_blocks(blocks)) else None
    d = bd.mm if bd is not None else _lib.MatMulDesc()
    b, H, M, K = A.shape
    d.batch, d.heads, d.M, d.K, d.N = b, H, M, K, B.shape[3]
    for i in range(4):
        d.a_stride[i] = A.stride(i)
        d.b_stride[i] = B.stride(i)
    d.A_bit, d.B_bit, d.metric, d.eq_n, d.search_round = A_bit, B_bit, metric_id(metric), eq_n, search_round
    d.sos, d.init_layerwise, d.reserved = int(sos), int(init_layerwise), int(reserved)
    if bd is not None:
        bd.n_V_A, bd.n_H_A, bd.n_V_B, bd.n_H_B = (int(n) for n in blocks)
    return (bd if bd is not None else d), d


def matmul_blocks_quant_forward(*, A, B, A_interval, B_interval, split, A_bit, B_bit, blocks, sos=False):
    """quant_forward of a calibrated MatMul with row / column sub-blocks (p4v_matmul_blocks_quant_forward): intervals
    [heads][n_V][n_H] per operand (the split-of-softmax A: its scalar interval and the split), `blocks` = (n_V_A, n_H_A, n_V_B,
    n_H_B).  An int8 MFMA GEMM per K segment, one fp32 rescale per segment."""
    lib = _lib.load()
    dev = device_of(A, B)
    A, B = to_dev(A, dev), to_dev(B, dev)
    bd, d = _matmul_desc(A, B, A_bit, B_bit, "L2_norm", 1, 1, sos, 0, _lib.RESERVED_FORWARD_ONLY, blocks, wrap=True)
    b, H, M, _ = A.shape
    need = _need(lib.p4v_matmul_blocks_workspace_bytes, bd, "p4v_matmul_blocks_workspace_bytes")
    ws = workspace(dev, need)
    A_iv = to_dev(A_interval, dev).reshape(-1).contiguous()
    B_iv = to_dev(B_interval, dev).reshape(-1).contiguous()
    if A_iv.numel() != (1 if sos else H * bd.n_V_A * bd.n_H_A) or B_iv.numel() != H * bd.n_V_B * bd.n_H_B:
        raise ValueError("matmul_blocks_quant_forward: interval tensors must hold [heads][n_V][n_H] values")
    sp = to_dev(split, dev).reshape(-1).contiguous() if sos else None
    out = torch.empty(b, H, M, d.N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.p4v_matmul_blocks_quant_forward(C.byref(bd), ptr(A), ptr(B), ptr(A_iv), ptr(B_iv), ptr(sp), ptr(out),
                                                 ptr(ws), ws.numel(), stream_ptr(dev))
    _lib.check(rc, "p4v_matmul_blocks_quant_forward")
    return out


def matmul_job(*, A, B, out, grad, A_bit, B_bit, metric, eq_alpha, eq_beta, eq_n, search_round,
               sos=False, init_layerwise=False, want_scores=False, prune=True, blocks=None):
    lib = _lib.load()
    dev = device_of(A, B)
    A, B, out, grad = (to_dev(t, dev) for t in (A, B, out, grad))
    out = out.contiguous()
    grad = grad.contiguous() if grad is not None else None
    b, H, M, K = A.shape
    N = B.shape[3]
    if has_blocks(blocks):
        # row / column sub-blocks: p4v_matmul_blocks_calibrate; intervals [heads][n_V][n_H], one score table per block step
        bd, _ = _matmul_desc(A, B, A_bit, B_bit, metric, eq_n, search_round, sos, init_layerwise, 0, blocks)
        need = _need(lib.p4v_matmul_blocks_workspace_bytes, bd, "p4v_matmul_blocks_workspace_bytes")
        mult = candidate_multipliers(eq_alpha, eq_beta, eq_n, dev)
        nA, nB = (1 if sos else H * bd.n_V_A * bd.n_H_A), H * bd.n_V_B * bd.n_H_B
        steps = (1 if sos else bd.n_V_A * bd.n_H_A) + bd.n_V_B * bd.n_H_B
        A_iv = torch.empty(nA, dtype=torch.float32, device=dev)
        B_iv = torch.empty(nB, dtype=torch.float32, device=dev)
        split = torch.empty(1, dtype=torch.float32, device=dev) if sos else None
        scores = torch.zeros(search_round, steps, eq_n, H, dtype=torch.float32, device=dev) if want_scores else None
        best = torch.zeros(search_round, steps, H, dtype=torch.int32, device=dev) if want_scores else None
        return Job(_lib.JOB_MATMUL_BLOCKS, "p4v_matmul_blocks_calibrate", bd, (A, B, out, grad), mult, (A_iv, B_iv, split), need,
                   dev, scores, best)
    d = _lib.MatMulDesc()
    d.batch, d.heads, d.M, d.K, d.N = b, H, M, K, N
    for i in range(4):
        d.a_stride[i] = A.stride(i)
        d.b_stride[i] = B.stride(i)
    d.A_bit, d.B_bit, d.metric, d.eq_n, d.search_round = A_bit, B_bit, metric_id(metric), eq_n, search_round
    d.sos, d.init_layerwise, d.reserved = int(sos), int(init_layerwise), (0 if prune else _lib.RESERVED_NO_PRUNE)
    need = _need(lib.p4v_matmul_workspace_bytes, d, "p4v_matmul_workspace_bytes")
    mult = candidate_multipliers(eq_alpha, eq_beta, eq_n, dev)
    A_iv = torch.empty(1 if sos else H, dtype=torch.float32, device=dev)
    B_iv = torch.empty(H, dtype=torch.float32, device=dev)
    split = torch.empty(1, dtype=torch.float32, device=dev) if sos else None
    scores = torch.zeros(search_round, 2, eq_n, H, dtype=torch.float32, device=dev) if want_scores else None
    best = torch.zeros(search_round, 2, H, dtype=torch.int32, device=dev) if want_scores else None
    return Job(_lib.JOB_MATMUL, "p4v_matmul_calibrate", d, (A, B, out, grad), mult, (A_iv, B_iv, split), need, dev, scores, best)


def matmul_calibrate(**kw):
    """Run calibration_step2 of a MatMul (head-wise; optional split-of-softmax on A) on the GPU."""
    job = run_job(matmul_job(**kw))
    return job.outputs[0], job.outputs[1], job.outputs[2], job.scores, job.best


def conv_job(*, weight, bias, x, out, grad, stride, padding, dilation, w_bit, a_bit, metric, eq_alpha, eq_beta,
             eq_n, search_round, channelwise=True, init_layerwise=False, want_scores=False, prune=True):
    lib = _lib.load()
    dev = device_of(x, weight)
    weight, bias, x, out, grad = (to_dev(t, dev) for t in (weight, bias, x, out, grad))
    weight = weight.contiguous(); x = x.contiguous(); out = out.contiguous()
    grad = grad.contiguous() if grad is not None else None
    b, ic, H, W = x.shape
    oc, _, kh, kw = weight.shape
    d = _lib.ConvDesc(b, ic, H, W, oc, kh, kw, stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1],
                      w_bit, a_bit, metric_id(metric), eq_n, search_round, int(channelwise), int(init_layerwise),
                      int(bias is not None), 0 if prune else _lib.RESERVED_NO_PRUNE)
    need = _need(lib.p4v_conv_workspace_bytes, d, "p4v_conv_workspace_bytes")
    mult = candidate_multipliers(eq_alpha, eq_beta, eq_n, dev)
    nw = oc if channelwise else 1
    w_iv = torch.empty(nw, dtype=torch.float32, device=dev)
    a_iv = torch.empty(1, dtype=torch.float32, device=dev)
    scores = torch.zeros(search_round, 2, eq_n, nw, dtype=torch.float32, device=dev) if want_scores else None
    best = torch.zeros(search_round, 2, nw, dtype=torch.int32, device=dev) if want_scores else None
    return Job(_lib.JOB_CONV, "p4v_conv_calibrate", d, (weight, bias, x, out, grad), mult, (w_iv, a_iv), need, dev, scores, best)


def conv_calibrate(**kw):
    """Run calibration_step2 of the patch-embedding Conv2d on the GPU (prune=False: no exact candidate pruning)."""
    job = run_job(conv_job(**kw))
    return job.outputs[0], job.outputs[1], job.scores, job.best


# ----------------------------------------------------------------------------------------------------------------
# Granular passes: one part of calibration_step2 per call (C ABI p4v_amax_init_* / p4v_*_search_*), for callers that
# drive the alternation themselves like the reference's _initialize_intervals / _search_best_*_interval methods.
# ----------------------------------------------------------------------------------------------------------------
def _flat(t, dev, rows=None):
    t = to_dev(t, dev).contiguous()
    return t.reshape(rows, -1) if rows is not None else t.reshape(-1)


class _Stepper:
    """Tensors + descriptor + scratch of one module, shared by the granular calls on it."""

    def _call(self, name, *args):
        with torch.cuda.device(self.dev):
            rc = getattr(self.lib, name)(C.byref(self.d), *[ptr(a) for a in args], ptr(self.ws), self.ws.numel(),
                                         stream_ptr(self.dev))
        _lib.check(rc, name)

    def _tables(self, want, blocks, eq_n=None):
        eq_n = self.d.eq_n if eq_n is None else eq_n
        if not want:
            return None, None
        return (torch.zeros(eq_n, blocks, dtype=torch.float32, device=self.dev),
                torch.zeros(blocks, dtype=torch.int32, device=self.dev))


class LinearStepper(_Stepper):
    def __init__(self, *, weight, bias, x, out, grad, w_bit, a_bit, metric, eq_n, n_V, n_H, n_a, init_layerwise=False,
                 postgelu=False, force_f32=False):
        self.lib = _lib.load()
        self.dev = dev = device_of(x, weight)
        self.weight, self.bias, self.x, self.out, self.grad = (
            (to_dev(t, dev).contiguous() if t is not None else None) for t in (weight, bias, x, out, grad))
        batch, K = self.x.shape[0], self.x.shape[-1]
        self.blocks_w, self.blocks_a, self.n_V = n_V * n_H, n_a, n_V
        self.d = _lib.LinearDesc(batch, self.x.numel() // (batch * K), K, self.weight.shape[0], n_V, n_H, n_a, w_bit, a_bit,
                                 metric_id(metric), eq_n, 1, int(postgelu), int(init_layerwise), int(bias is not None),
                                 int(force_f32))
        need = self.lib.p4v_linear_workspace_bytes(C.byref(self.d))
        if need == 0:
            _lib.check(-2, "p4v_linear_workspace_bytes")
        self.ws = workspace(dev, need)

    def init_intervals(self):
        w_iv = torch.empty(self.blocks_w, dtype=torch.float32, device=self.dev)
        a_iv = torch.empty(self.blocks_a, dtype=torch.float32, device=self.dev)
        self._call("p4v_amax_init_linear", self.weight, self.x, w_iv, a_iv)
        return w_iv, a_iv

    def _call_block(self, block, name, *args):
        """One granular search call; `block`: the step of that column / activation block alone (desc.reserved bits 8..11), whose
        score table the call then returns -- None: every block in turn, the tables of block 0."""
        base = self.d.reserved
        self.d.reserved = base | _lib.reserved_block(block)
        try:
            self._call(name, *args)
        finally:
            self.d.reserved = base

    def search_w(self, w_cands, w_interval, a_interval, want_scores=False, block=None):
        """Returns (new w_interval [n_V*n_H], scores [eq_n][n_V] | None, best [n_V] | None)."""
        w_iv = _flat(w_interval, self.dev).clone()
        scores, best = self._tables(want_scores, self.n_V)
        self._call_block(block, "p4v_linear_search_w", self.weight, self.bias, self.x, self.out, self.grad,
                         _flat(w_cands, self.dev, self.d.eq_n + 1), w_iv, _flat(a_interval, self.dev), scores, best)
        return w_iv, scores, best

    def search_a(self, a_cands, w_interval, a_interval, want_scores=False, block=None):
        a_iv = _flat(a_interval, self.dev).clone()
        scores, best = self._tables(want_scores, self.n_V)
        self._call_block(block, "p4v_linear_search_a", self.weight, self.bias, self.x, self.out, self.grad,
                         _flat(a_cands, self.dev, self.d.eq_n + 1), _flat(w_interval, self.dev), a_iv, scores, best)
        return a_iv, scores, best


class MatMulStepper(_Stepper):
    def __init__(self, *, A, B, out, grad, A_bit, B_bit, metric, eq_n, sos=False, init_layerwise=False, blocks=None):
        self.lib = _lib.load()
        self.dev = dev = device_of(A, B)
        self.A, self.B = to_dev(A, dev), to_dev(B, dev)
        self.out = to_dev(out, dev).contiguous() if out is not None else None
        self.grad = to_dev(grad, dev).contiguous() if grad is not None else None
        self.H, self.sos = self.A.shape[1], bool(sos)
        # `d`: the p4v_matmul_desc of the head-wise entry points; `bd`: with row / column sub-blocks, the descriptor around it
        self.blocks = tuple(int(n) for n in blocks) if has_blocks(blocks) else None
        desc, self.d = _matmul_desc(self.A, self.B, A_bit, B_bit, metric, eq_n, 1, sos, init_layerwise, 0, self.blocks)
        self.bd = desc if self.blocks else None
        if self.blocks:
            need = _need(self.lib.p4v_matmul_blocks_workspace_bytes, desc, "p4v_matmul_blocks_workspace_bytes")
        else:
            need = self.lib.p4v_matmul_workspace_bytes(C.byref(self.d))
            if need == 0:
                _lib.check(-2, "p4v_matmul_workspace_bytes")
        self.ws = workspace(dev, need)

    def _call_blocks(self, name, lead, *args):
        with torch.cuda.device(self.dev):
            rc = getattr(self.lib, name)(C.byref(self.bd), *lead, *[ptr(a) for a in args], ptr(self.ws), self.ws.numel(),
                                         stream_ptr(self.dev))
        _lib.check(rc, name)

    def init_intervals(self):
        """(A_interval [heads] -- None for the split-of-softmax class, whose split search sets it -- , B_interval [heads]);
        with row / column sub-blocks [heads * n_V * n_H] each."""
        nA, nB = (self.H * self.blocks[0] * self.blocks[1], self.H * self.blocks[2] * self.blocks[3]) if self.blocks else (self.H, self.H)
        A_iv = torch.empty(nA, dtype=torch.float32, device=self.dev)
        B_iv = torch.empty(nB, dtype=torch.float32, device=self.dev)
        if self.blocks:
            self._call_blocks("p4v_amax_init_matmul_blocks", (), self.A, self.B, A_iv, B_iv)
        else:
            self._call("p4v_amax_init_matmul", self.A, self.B, A_iv, B_iv)
        return (None if self.sos else A_iv), B_iv

    def search_block(self, operand, v, h, cands, A_interval, B_interval, split=None, want_scores=False):
        """ONE block step (p4v_matmul_blocks_search): `operand` "A" / "B", block (v, h), `cands` [eq_n+1][heads] that block's
        candidates per head, both interval tensors [heads * n_V * n_H] as they enter the step.  Returns (the searched tensor
        with block (v, h) of every head replaced, scores [eq_n][heads] | None, best [heads] | None)."""
        A_iv, B_iv = _flat(A_interval, self.dev).clone(), _flat(B_interval, self.dev).clone()
        scores, best = self._tables(want_scores, self.H)
        self._call_blocks("p4v_matmul_blocks_search", (0 if operand == "A" else 1, int(v), int(h)), self.A, self.B, self.out,
                          self.grad, _flat(cands, self.dev, self.d.eq_n + 1), A_iv, B_iv,
                          (_flat(split, self.dev) if self.sos else None), scores, best)
        return (A_iv if operand == "A" else B_iv), scores, best

    def search_A(self, A_cands, A_interval, B_interval, want_scores=False):
        A_iv = _flat(A_interval, self.dev).clone()
        scores, best = self._tables(want_scores, self.H)
        self._call("p4v_matmul_search_A", self.A, self.B, self.out, self.grad, _flat(A_cands, self.dev, self.d.eq_n + 1),
                   A_iv, _flat(B_interval, self.dev), scores, best)
        return A_iv, scores, best

    def search_split(self, want_scores=False):
        """SoS: (split [1], A_interval [1] = split/(qmax-1), scores [20][1] | None, best [1] | None)."""
        split = torch.empty(1, dtype=torch.float32, device=self.dev)
        A_iv = torch.empty(1, dtype=torch.float32, device=self.dev)
        scores = best = None
        if want_scores:
            if self.d.eq_n < 20:
                raise ValueError("the split score table has 20 rows: eq_n >= 20 needed to return it")
            scores, best = self._tables(True, self.H)
        self._call("p4v_sos_search_split", self.A, self.B, self.out, self.grad, split, A_iv, scores, best)
        return split, A_iv, (scores[:20, :1] if scores is not None else None), (best[:1] if best is not None else None)

    def search_B(self, B_cands, A_interval, B_interval, split=None, want_scores=False):
        B_iv = _flat(B_interval, self.dev).clone()
        scores, best = self._tables(want_scores, self.H)
        self._call("p4v_matmul_search_B", self.A, self.B, self.out, self.grad, _flat(B_cands, self.dev, self.d.eq_n + 1),
                   _flat(A_interval, self.dev), (_flat(split, self.dev) if self.sos else None), B_iv, scores, best)
        return B_iv, scores, best


class ConvStepper(_Stepper):
    def __init__(self, *, weight, bias, x, out, grad, stride, padding, dilation, w_bit, a_bit, metric, eq_n,
                 channelwise=True, init_layerwise=False):
        self.lib = _lib.load()
        self.dev = dev = device_of(x, weight)
        self.weight, self.bias, self.x, self.out, self.grad = (
            (to_dev(t, dev).contiguous() if t is not None else None) for t in (weight, bias, x, out, grad))
        b, ic, H, W = self.x.shape
        oc, _, kh, kw = self.weight.shape
        self.nw, self.channelwise = (oc if channelwise else 1), bool(channelwise)
        self.d = _lib.ConvDesc(b, ic, H, W, oc, kh, kw, stride[0], stride[1], padding[0], padding[1], dilation[0],
                               dilation[1], w_bit, a_bit, metric_id(metric), eq_n, 1, int(channelwise),
                               int(init_layerwise), int(bias is not None), 0)
        need = self.lib.p4v_conv_workspace_bytes(C.byref(self.d))
        if need == 0:
            _lib.check(-2, "p4v_conv_workspace_bytes")
        self.ws = workspace(dev, need)

    def init_intervals(self):
        w_iv = torch.empty(self.nw, dtype=torch.float32, device=self.dev)
        a_iv = torch.empty(1, dtype=torch.float32, device=self.dev)
        self._call("p4v_amax_init_conv", self.weight, self.x, w_iv, a_iv)
        return w_iv, a_iv

    def search_w(self, w_cands, w_interval, a_interval, want_scores=False):
        w_iv = _flat(w_interval, self.dev).clone()
        scores, best = self._tables(want_scores, self.nw)
        name = "p4v_conv_search_w_channelwise" if self.channelwise else "p4v_conv_search_w_layerwise"
        self._call(name, self.weight, self.bias, self.x, self.out, self.grad, _flat(w_cands, self.dev, self.d.eq_n + 1),
                   w_iv, _flat(a_interval, self.dev), scores, best)
        return w_iv, scores, best

    def search_a(self, a_cands, w_interval, a_interval, want_scores=False):
        a_iv = _flat(a_interval, self.dev).clone()
        scores, best = self._tables(want_scores, self.nw)
        self._call("p4v_conv_search_a", self.weight, self.bias, self.x, self.out, self.grad,
                   _flat(a_cands, self.dev, self.d.eq_n + 1), _flat(w_interval, self.dev), a_iv, scores, best)
        return a_iv, scores, best


def score_argmax_gather(scores, cands):
    """(interval [blocks], best [blocks]): first-maximum argmax over the candidate axis, NaN counts as the maximum."""
    lib = _lib.load()
    _require_cuda(scores, "scores")
    dev = scores.device
    scores = scores.float().contiguous()
    eq_n, blocks = scores.shape
    cands = to_dev(cands, dev).contiguous().reshape(-1, blocks)
    if cands.shape[0] < eq_n:
        raise ValueError("candidate table shorter than the score table")
    iv = torch.empty(blocks, dtype=torch.float32, device=dev)
    best = torch.empty(blocks, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.p4v_score_argmax_gather(ptr(scores), eq_n, blocks, ptr(cands), ptr(iv), ptr(best), stream_ptr(dev))
    _lib.check(rc, "p4v_score_argmax_gather")
    return iv, best


def quantize_i8(x2d, scales, rows_per_scale, lo, hi):
    """int8 grid indices clamp(rint(x/s), lo, hi) of a 2-D fp32 tensor (K padded to 64 with zeros)."""
    lib = _lib.load()
    _require_cuda(x2d, "x")
    x2d = x2d.contiguous().float()
    rows, cols = x2d.shape
    colsp = (cols + 63) // 64 * 64
    q = torch.empty(rows, colsp, dtype=torch.int8, device=x2d.device)
    scales = scales.to(x2d.device, torch.float32).contiguous()
    rc = lib.p4v_quantize_i8(ptr(x2d), rows, cols, colsp, ptr(scales), rows_per_scale, lo, hi, ptr(q), stream_ptr(x2d.device))
    _lib.check(rc, "p4v_quantize_i8")
    return q[:, :cols]


def pack_plane_i8(x2d, *, mode="sym", scales=None, rows_per_scale=1, lo=-128, hi=127, qmax=128, const_scale=0.0):
    """ONE int8 operand plane exactly as the candidate sweeps consume it (p4v_pack_plane_i8): mode "sym"
    (clamp(rint(x/s), lo, hi); `scales=None` uses `const_scale`, the post-GELU negative range), "sos_hi" / "sos_lo"
    (split-of-softmax ranges, `scales` = the split), "twin" (both post-GELU ranges in one plane: `scales` = the positive
    interval, `const_scale` the negative one, lo < 0 < hi).  Returns the [rows][cols] int8 plane (padding stripped)."""
    lib = _lib.load()
    _require_cuda(x2d, "x")
    x2d = x2d.contiguous().float()
    rows, cols = x2d.shape
    colsp = (cols + 63) // 64 * 64
    q = torch.empty(rows, colsp, dtype=torch.int8, device=x2d.device)
    d = _lib.PlaneDesc(rows, cols, colsp, int(rows_per_scale),
                       {"sym": _lib.PLANE_SYM, "sos_hi": _lib.PLANE_SOS_HI, "sos_lo": _lib.PLANE_SOS_LO, "twin": _lib.PLANE_TWIN}[mode],
                       int(lo), int(hi), int(qmax), float(const_scale), 0)
    sc = scales.to(x2d.device, torch.float32).reshape(-1).contiguous() if scales is not None else None
    with torch.cuda.device(x2d.device):
        rc = lib.p4v_pack_plane_i8(C.byref(d), ptr(x2d), ptr(sc), ptr(q), stream_ptr(x2d.device))
    _lib.check(rc, "p4v_pack_plane_i8")
    return q[:, :cols], q


def fake_quant(x2d, scales, rows_per_scale, lo, hi):
    """clamp(rint(x / s), lo, hi) * s of a 2-D fp32 tensor, s = scales[row // rows_per_scale] (p4v_fake_quant)."""
    lib = _lib.load()
    _require_cuda(x2d, "x")
    x2d = x2d.contiguous().float()
    rows, cols = x2d.shape
    y = torch.empty_like(x2d)
    scales = scales.to(x2d.device, torch.float32).reshape(-1).contiguous()
    with torch.cuda.device(x2d.device):
        rc = lib.p4v_fake_quant(ptr(x2d), rows, cols, ptr(scales), int(rows_per_scale), int(lo), int(hi), ptr(y),
                                stream_ptr(x2d.device))
    _lib.check(rc, "p4v_fake_quant")
    return y


def _pad4(seq, fill):
    seq = list(seq)
    return [fill] * (4 - len(seq)) + seq


def export_quantize(src, *, mode, scale1, scale1_stride, scale1_div, lo1=0, hi1=0, scale2=None, scale2_stride=(0, 0, 0, 0),
                    scale2_div=(1, 1, 1, 1), scale2_const=0.0, lo2=0, hi2=0, qmax=128, dims=None, src_stride=None):
    """Integer image of `src` on the GPU (p4v_export_quantize).  `src` is viewed as the 4-D tensor `dims` through the
    element strides `src_stride` (default: src's own shape / strides, left-padded to 4-D).  Returns a contiguous device
    tensor of `dims`: int8 (sym_i8), float32 (sym_f32) or uint8 (gelu_u8 / sos_u8)."""
    lib = _lib.load()
    _require_cuda(src, "export source")
    dev = src.device
    src = src.detach()
    if src.dtype != torch.float32:
        if src_stride is not None and not src.is_contiguous():
            # the caller's strides describe `src` as it is; `.float()` of a non-dense view has other strides
            raise TypeError("export_quantize: explicit src_stride needs a float32 source (convert before deriving the strides)")
        src = src.float()
    if dims is None:
        dims, src_stride = _pad4(src.shape, 1), _pad4(src.stride(), 0)
    code = {"sym_i8": _lib.EXPORT_SYM_I8, "sym_f32": _lib.EXPORT_SYM_F32, "gelu_u8": _lib.EXPORT_GELU_U8,
            "sos_u8": _lib.EXPORT_SOS_U8}[mode]
    out = torch.empty(tuple(dims), dtype={"sym_i8": torch.int8, "sym_f32": torch.float32}.get(mode, torch.uint8), device=dev)
    d = _lib.ExportDesc()
    for i in range(4):
        d.dims[i], d.src_stride[i] = int(dims[i]), int(src_stride[i])
        d.scale1_stride[i], d.scale1_div[i] = int(scale1_stride[i]), int(scale1_div[i])
        d.scale2_stride[i], d.scale2_div[i] = int(scale2_stride[i]), int(scale2_div[i])
    d.scale2_const = float(scale2_const)
    d.mode, d.lo1, d.hi1, d.lo2, d.hi2, d.qmax, d.reserved = code, int(lo1), int(hi1), int(lo2), int(hi2), int(qmax), 0
    s1 = to_dev(torch.as_tensor(scale1), dev).reshape(-1).contiguous()
    s2 = to_dev(torch.as_tensor(scale2), dev).reshape(-1).contiguous() if scale2 is not None else None
    with torch.cuda.device(dev):
        rc = lib.p4v_export_quantize(C.byref(d), ptr(src), ptr(s1), ptr(s2), ptr(out), stream_ptr(dev))
    _lib.check(rc, "p4v_export_quantize")
    return out


def multi_copy(table, n, index, max_bytes, dev):
    """One launch: for each of the `n` {src, dst base, bytes} triples of the device int64 `table`, copy `bytes` from src
    to dst base + index * bytes (p4v_multi_copy: the capture pass appends a sub-batch to every cache at once)."""
    lib = _lib.load()
    with torch.cuda.device(dev):
        rc = lib.p4v_multi_copy(ptr(table), int(n), int(index), int(max_bytes), stream_ptr(dev))
    _lib.check(rc, "p4v_multi_copy")


def stats_enable(flag):
    """Launch timing of the sweep kernels on the CALLING thread (bench.py roofline)."""
    _lib.load().p4v_stats_enable(int(bool(flag)))


def debug_variant(variant=0, force_generic=False):
    """Kernel A/B switches (tests, tools/bench_layer.py); 0 in production."""
    _lib.check(_lib.load().p4v_debug_set_variant(int(variant), int(bool(force_generic))), "p4v_debug_set_variant")


def debug_tuning(key, value):
    _lib.check(_lib.load().p4v_debug_set_tuning(int(key), int(value)), "p4v_debug_set_tuning")


def debug_arena_gap(nbytes=0):
    """Bytes the arena leaves unused behind every allocation (p4v_debug_set_arena_gap; a multiple of 256, 0 = off).  The sizing
    queries include the gaps: build the job AFTER setting it.  For the tests of the workspace contract."""
    _lib.check(_lib.load().p4v_debug_set_arena_gap(int(nbytes)), "p4v_debug_set_arena_gap")


def debug_arena_ranges():
    """[(begin, end)] byte ranges of the workspace that the allocations of the calling thread's last single-module call covered
    (p4v_debug_arena_ranges), merged and ascending.  Recorded only while the arena gap is on."""
    lib = _lib.load()
    n = lib.p4v_debug_arena_ranges(None, 0)
    buf = (C.c_uint64 * max(2, 2 * n))()
    n = min(n, lib.p4v_debug_arena_ranges(buf, n))
    return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(n)]


def debug_bound_totals(start=False):
    """start=True: keep the stage-B1 totals (the bound) of this thread's pruned passes from now on.  Otherwise stop and return
    the ones kept, in pass order (p4v_debug_bound_totals) -- for tests that compare two stage-B1 kernels."""
    lib = _lib.load()
    if start:
        _lib.check(lib.p4v_debug_bound_totals(None, 0, None), "p4v_debug_bound_totals")
        return None
    n = C.c_int64(0)
    _lib.check(lib.p4v_debug_bound_totals(None, 0, C.byref(n)), "p4v_debug_bound_totals")
    buf = (C.c_float * max(1, n.value))()
    _lib.check(lib.p4v_debug_bound_totals(buf, n.value, C.byref(n)), "p4v_debug_bound_totals")
    return [float(v) for v in buf[:n.value]]


def debug_prune_tables(start=False):
    """start=True: keep the stage tables of this thread's pruned passes from now on.  Otherwise stop and return one dict per
    staged pass, in pass order (p4v_debug_prune_tables; include/ptq4vit_hip_debug.h lists the record): the flags, the ranges
    r1 / r2 / r3 as (lo, hi), best [nj], rblk2 / rblk3 [nj][2] (int32 tensors) and the tables SA, SB, SA2, S2 (fp32 CPU
    tensors [rows][nj]; None where the pass did not run the stage).  What a pass did not write is -1."""
    lib = _lib.load()
    if start:
        _lib.check(lib.p4v_debug_prune_tables(None, 0, None), "p4v_debug_prune_tables")
        return None
    n = C.c_int64(0)
    _lib.check(lib.p4v_debug_prune_tables(None, 0, C.byref(n)), "p4v_debug_prune_tables")
    buf = (C.c_int32 * max(1, n.value))()
    _lib.check(lib.p4v_debug_prune_tables(buf, n.value, C.byref(n)), "p4v_debug_prune_tables")
    words = torch.frombuffer(buf, dtype=torch.int32)[:n.value].clone()
    recs, at = [], 0
    while at < n.value:
        h = [int(v) for v in words[at:at + 24]]
        size, eq_n, nj, sb_rows = h[0], h[4], h[5], h[12]
        assert size >= 24 and at + size <= n.value, "p4v_debug_prune_tables: broken record"
        body = words[at + 24:at + size]
        pos = 0

        def take(count, shape, as_float=False):
            nonlocal pos
            part = body[pos:pos + count].clone()
            pos += count
            return (part.view(torch.float32) if as_float else part).reshape(shape)
        rec = dict(split_search=bool(h[1]), round=h[2], side=h[3], eq_n=eq_n, nj=nj, virt=bool(h[6]), hull_selects=bool(h[7]),
                   b1_bound=bool(h[8]), tier2=bool(h[9]), host_read=bool(h[10]),
                   margin=float(words[at + 11:at + 12].clone().view(torch.float32)), r1=(h[16], h[17]), r2=(h[18], h[19]),
                   r3=(h[20], h[21]), slice_rows=h[22], slice2_rows=h[23], has_rblk=bool(h[15]))
        rec["best"] = take(nj, (nj,))
        rec["rblk2"] = take(2 * nj, (nj, 2))
        rec["rblk3"] = take(2 * nj, (nj, 2))
        rec["SA"] = take(eq_n * nj, (eq_n, nj), True)
        rec["SB"] = take(sb_rows * nj, (sb_rows, nj), True)
        rec["SA2"] = take(eq_n * nj, (eq_n, nj), True) if h[13] else None
        rec["S2"] = take(eq_n * nj, (eq_n, nj), True) if h[14] else None
        assert pos == size - 24, "p4v_debug_prune_tables: broken record"
        recs.append(rec)
        at += size
    return recs


def debug_prune_decide(SA, T, cands, *, virt, honour_blk, host_reads, SA2=None):
    """The decision chain of a pruned pass (k_prune_pick, k_prune_hull, k_merge_*, k_select through the pass's own launchers;
    p4v_debug_prune_decide) on the stage-A scores `SA` [C][nj], the full totals `T` [C][nj] that stand in for the sweeps of stages
    B1 / B2, the optional second-tier scores `SA2` and the candidate table `cands` [C + 1][nj], all fp32 on the device.
    Returns a dict of CPU values: r1, r2, r3 as (lo, hi), rblk2 / rblk3 [nj][2], best [nj], interval [nj], best_out [nj],
    hull_selects, tier2, exit (0: merge and k_select; 1 / 2: no stage B2 after the first / second hull).  For the tests."""
    f32 = lambda t: None if t is None else t.contiguous().float()
    SA, T, cands, SA2 = f32(SA), f32(T), f32(cands), f32(SA2)
    n_c, nj = (int(v) for v in T.shape) if T is not None and T.dim() == 2 else (0, 0)
    dev = T.device if T is not None else torch.device("cuda", torch.cuda.current_device())
    i32 = lambda n: torch.zeros(max(1, n), dtype=torch.int32, device=dev)
    ranges, rblk, best, best_out = i32(6), i32(4 * nj), i32(nj), i32(nj)
    interval = torch.full((max(1, nj),), float("nan"), dtype=torch.float32, device=dev)
    info = (C.c_int32 * 3)()
    with torch.cuda.device(dev):
        rc = _lib.load().p4v_debug_prune_decide(ptr(SA), ptr(SA2), ptr(T), ptr(cands), n_c, nj, int(bool(virt)), int(bool(honour_blk)),
                                                int(bool(host_reads)), ptr(ranges), ptr(rblk), ptr(best), ptr(interval),
                                                ptr(best_out), info, stream_ptr(dev))
    _lib.check(rc, "p4v_debug_prune_decide")
    r = [int(v) for v in ranges.cpu()]
    rb = rblk.cpu().reshape(2, nj, 2)
    return dict(r1=(r[0], r[1]), r2=(r[2], r[3]), r3=(r[4], r[5]), rblk2=rb[0], rblk3=rb[1], best=best.cpu(), interval=interval.cpu(),
                best_out=best_out.cpu(), hull_selects=bool(info[0]), tier2=bool(info[1]), exit=int(info[2]))


def debug_topk_rows(mass, k):
    """Row selection of the exact pruning (k_topk_rows) on `mass` [segs, n] fp32: int32 [segs, k], the segment-local indices
    of the k heaviest entries in ascending order (ties: lowest indices).  For the tests."""
    assert mass.is_cuda and mass.dtype == torch.float32 and mass.dim() == 2 and mass.is_contiguous()
    segs, n = mass.shape
    out = torch.empty(segs, int(k), dtype=torch.int32, device=mass.device)
    with torch.cuda.device(mass.device):
        rc = _lib.load().p4v_debug_topk_rows(ptr(mass), segs, n, int(k), ptr(out), stream_ptr(mass.device))
    _lib.check(rc, "p4v_debug_topk_rows")
    return out


def debug_pack_dual(x2d, *, sos, scale, lo, hi, qmax, const_scale=0.0):
    """Both int8 planes of a twin row operand from one launch (k_pack_dual): `sos` False the post-GELU pair ([0, hi] on
    `scale`, [lo, 0] on `const_scale`), True the split-of-softmax pair (split `scale`).  Returns the two [rows][cols] planes
    (padding stripped) and the padded ones.  For the tests."""
    x2d = x2d.contiguous().float()
    rows, cols = x2d.shape
    colsp = (cols + 63) // 64 * 64
    q1 = torch.empty(rows, colsp, dtype=torch.int8, device=x2d.device)
    q2 = torch.empty_like(q1)
    sc = torch.tensor([float(scale)], dtype=torch.float32, device=x2d.device)
    with torch.cuda.device(x2d.device):
        rc = _lib.load().p4v_debug_pack_dual(ptr(x2d), rows, cols, colsp, int(bool(sos)), int(lo), int(hi), int(qmax), ptr(sc),
                                             float(const_scale), ptr(q1), ptr(q2), stream_ptr(x2d.device))
    _lib.check(rc, "p4v_debug_pack_dual")
    return q1[:, :cols], q2[:, :cols], q1, q2


def debug_pack_cands(x2d, scales, *, layout, lo, hi, rows_padded=None, crange=None, done=None, live_max=-1, general=False,
                     out=None):
    """The candidate planes of `x2d` [rows][cols] on the scales `scales` [C] as the search packs them (k_pack, k_pack1 for a
    single plane; p4v_debug_pack_cands): layout 0 [C][rows_padded][cols_padded], 1 [rows_padded][C][cols_padded], 2 candidate
    pairs interleaved per 64-byte k-tile, 3 one plane in MFMA-fragment order.  `crange` (int32 [2] on the device) / `done`
    (uint8 [C]) / `live_max` as in the header; `out`: the destination (flat int8, left as it is where nothing is packed).  Returns
    the flat int8 buffer.  For the tests."""
    x2d = x2d.contiguous().float()
    scales = scales.contiguous().float()
    rows, cols = x2d.shape
    n = scales.numel()
    colsp = (cols + 63) // 64 * 64
    rowsp = rows if rows_padded is None else int(rows_padded)
    size = rowsp * colsp * (1 if layout == 3 else (n + 1) // 2 * 2 if layout == 2 else n)
    if out is None:
        out = torch.zeros(size, dtype=torch.int8, device=x2d.device)
    assert out.dtype == torch.int8 and out.is_contiguous() and out.numel() >= size
    with torch.cuda.device(x2d.device):
        rc = _lib.load().p4v_debug_pack_cands(ptr(x2d), rows, cols, rowsp, colsp, int(layout), int(lo), int(hi), ptr(scales), n,
                                              ptr(crange) if crange is not None else None,
                                              ptr(done) if done is not None else None, int(live_max), int(bool(general)),
                                              ptr(out), stream_ptr(x2d.device))
    _lib.check(rc, "p4v_debug_pack_cands")
    return out


def debug_gather_im2col(x, idx, *, kernel_size, stride, padding, dilation):
    """Rows `idx` (int32 [k], each in [0, b * fh * fw)) of the im2col matrix of the conv input `x` [b][ic][H][W] as the pruned
    passes gather them (k_gather_im2col; p4v_debug_gather_im2col): fp32 [k][ic * kh * kw].  For the tests."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and idx.is_cuda and idx.dtype == torch.int32 and idx.dim() == 1
    x, idx = x.contiguous(), idx.contiguous()
    b, ic, H, W = x.shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel_size, stride, padding, dilation
    fh, fw = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    if fh > 0 and fw > 0:
        assert idx.numel() > 0 and int(idx.min()) >= 0 and int(idx.max()) < b * fh * fw, "row index outside the im2col matrix"
    out = torch.full((idx.numel(), ic * kh * kw), float("nan"), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().p4v_debug_gather_im2col(b, ic, H, W, kh, kw, sh, sw, ph, pw, dh, dw, ptr(x), ptr(idx), idx.numel(), ptr(out),
                                                 stream_ptr(x.device))
    _lib.check(rc, "p4v_debug_gather_im2col")
    return out


def debug_prep_epi6(o, wt, bias, *, o_ss, o_ts, sr, tr, bias_on_t, wt_mode, transposed):
    """k_sweep6's epilogue operands in fragment order (k_prep_epi6) from the flat fp32 tensors `o`, `wt` (or None), `bias`:
    a flat fp32 tensor of ceil(sr / 256) * ceil(tr / 64) * 256 * 64 * 2 values.  For the tests."""
    n = -(-sr // 256) * -(-tr // 64) * 256 * 64 * 2
    e = torch.full((n,), float("nan"), dtype=torch.float32, device=o.device)
    with torch.cuda.device(o.device):
        rc = _lib.load().p4v_debug_prep_epi6(ptr(o), ptr(wt) if wt is not None else None, ptr(bias), int(o_ss), int(o_ts),
                                             int(sr), int(tr), int(bias_on_t), int(wt_mode), int(transposed), ptr(e),
                                             stream_ptr(o.device))
    _lib.check(rc, "p4v_debug_prep_epi6")
    return e

def debug_sos_sweep(*, A, B, out, grad, A_bit, metric, crange=None, known_cands=-1, n_cands=20):
    """ONE sweep of the split-of-softmax split search (k_sos_split + k_finish; p4v_debug_sos_sweep) over the first `n_cands`
    splits of A [b][H][M][K] against the raw B [b][H][K][N] (any strides): the [n_cands] score table, -inf outside `crange`
    = (lo, hi) (None: no range).  `known_cands`: what the sweep is told about the number of candidates in the range; it
    selects the kernel instance, never the result.  For the tests and tools/sos_probe.py."""
    lib = _lib.load()
    dev = device_of(A, B)
    A, B = to_dev(A, dev), to_dev(B, dev)
    out = to_dev(out, dev).contiguous()
    grad = to_dev(grad, dev).contiguous() if grad is not None else None
    d = _matmul_desc(A, B, A_bit, 8, metric, 100, 1, True, 0, 0)[1]
    ws = workspace(dev, _need(lib.p4v_matmul_workspace_bytes, d, "p4v_matmul_workspace_bytes"))
    scores = torch.full((int(n_cands),), float("nan"), dtype=torch.float32, device=dev)
    lo, hi = (-1, -1) if crange is None else (int(crange[0]), int(crange[1]))
    with torch.cuda.device(dev):
        rc = lib.p4v_debug_sos_sweep(C.byref(d), ptr(A), ptr(B), ptr(out), ptr(grad), int(n_cands), lo, hi, int(known_cands),
                                     ptr(scores), ptr(ws), ws.numel(), stream_ptr(dev))
    _lib.check(rc, "p4v_debug_sos_sweep")
    return scores


def stats_reset():
    _lib.load().p4v_stats_reset()


def stats_get():
    s = _lib.KernelStats()
    _lib.check(_lib.load().p4v_stats_get(C.byref(s)), "p4v_stats_get")
    return {k: getattr(s, k) for k, _ in _lib.KernelStats._fields_}


def prune_counters(reset=False):
    """Process-wide counters of the exact candidate pruning since the last reset (p4v_prune_counters): how many search
    passes ran in three stages, how many of those had no survivors besides the bound's candidates, how many eligible passes
    kept the full sweep, how many were never eligible (score tables, cosine, fp32 planes, pruning switched off)."""
    out = (C.c_int64 * 4)()
    _lib.check(_lib.load().p4v_prune_counters(out, int(bool(reset))), "p4v_prune_counters")
    return dict(zip(("staged", "staged_no_survivors", "kept_full_sweep", "not_eligible"), (int(v) for v in out)))


def stats_launches():
    """Every sweep launch the calling thread enqueued with timing enabled since the last stats_reset(), in launch order:
    [{"kernel", "stage", "grid_x", "grid_z", "ms", "ops", "alg_ops", "alg_bytes"}] (p4v_stats_launches)."""
    lib = _lib.load()
    n = C.c_int64(0)
    _lib.check(lib.p4v_stats_launches(None, 0, C.byref(n)), "p4v_stats_launches")
    buf = (_lib.LaunchRecord * max(1, n.value))()
    _lib.check(lib.p4v_stats_launches(buf, n.value, C.byref(n)), "p4v_stats_launches")
    return [{"kernel": _lib.LAUNCH_KINDS.get(r.kind, str(r.kind)), "stage": _lib.LAUNCH_STAGES.get(r.stage, str(r.stage)),
             "grid_x": r.grid_x, "grid_z": r.grid_z, "ms": r.ms, "ops": r.ops, "alg_ops": r.alg_ops, "alg_bytes": r.alg_bytes}
            for r in buf[:n.value]]
