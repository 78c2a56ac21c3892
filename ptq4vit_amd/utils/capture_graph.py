"""The capture passes of a Hessian calibration served from HIP graphs: everything between "a graph may be used" and "the
caches are filled".  The calibrator (utils/quant_calib.py) keeps the hooks, `_capture` and the eager passes.

With batch_size=4 (the reference's setting) the eager pass is bound by launch overhead, not by the GPU (~130 ms of Python /
dispatcher time for ~70 ms of kernels on ViT-B, tools/prof_capture.py).  All modules run in "raw" mode during a non-sequential
capture, so every sub-batch executes the same kernel sequence: it is recorded once (hooks included -- they see the graph's static
tensors) and replayed per sub-batch; after each replay the hooked tensors are copied into their slice of the preallocated caches
(the copy torch.cat would have done).

State on the network: `net.__dict__["_p4v_capture_graphs"]` maps `graph_key` to the list of `Lane`s (one geometry at a time: a
graph pins its activations' memory; the same list object is replayed by the capture of a second group of modules and by every
later calibration), `net.__dict__["_p4v_capture_shadow"]` is the `ArchRecord` those lanes belong to when they are the
architecture's.
"""
import copy
import sys
import time
from collections import namedtuple

import torch

from ..quant_layers.matmul import MinMaxQuantMatMul

CACHES = ("raw_input", "raw_out", "raw_grad")


# One instantiated graph of the sub-batch pass with its own static tensors.  `inv_n` is read by every replay: it must live as long
# as the graph.  `statics`: module -> ([static input(s), output(, output gradient)], has a gradient).  `recipes` (used on lane 0
# only): tuple(names) -> Recipe.  `is_block`: tuple(names) -> the recipe's flags checked against THIS lane's statics.
Lane = namedtuple("Lane", "graph static_in static_tgt inv_n statics recipes is_block")
# What does not change between calibrations of one network is kept with the graph instance: the layout of every cache (shape +
# strides: _cache_like) and which pieces are one dense block (_same_dense_block) -- ~3 ms of Python per calibration, during which
# the GPU had nothing to do.
Recipe = namedtuple("Recipe", "n_sub layout is_block")


class ArchRecord:
    """An architecture in this process: how many network objects of it were seen and, once built, the shadow -- a private copy of
    the network (own parameter storage), its wrapped modules and the lanes recorded on it."""

    def __init__(self):
        self.seen, self.nets = 0, set()
        self.net = self.mods = self.lanes = None
        self.unavailable = False      # the network cannot be copied, or graph capture failed on the copy


def forget_caches(m):
    """Step 2 deletes the caches (reference linear.py:554); the hooks expect them to exist."""
    m.raw_input = m.raw_out = None
    if hasattr(m, "metric"):
        m.raw_grad = None


def _cache_like(t, n_sub):
    """Cache for `n_sub` sub-batch pieces shaped like `t`, concatenated on dim 0 -- with t's memory layout when t is a dense
    permutation whose batch dim is outermost in memory (e.g. the k.transpose(-2, -1) view the attention passes to matmul1):
    sub-batch i is then ONE contiguous block of the cache, and the consumer reads the view in place as before."""
    shape = (n_sub * t.shape[0],) + tuple(t.shape[1:])
    if t.is_contiguous() or t.dim() < 2:
        return torch.empty(shape, dtype=t.dtype, device=t.device)
    order = sorted(range(t.dim()), key=lambda k: (-t.stride(k), k))           # outermost -> innermost in memory
    dense, expect = order[0] == 0, 1
    for k in reversed(order):
        dense &= t.stride(k) == expect
        expect *= t.shape[k]
    if not dense:
        return torch.empty(shape, dtype=t.dtype, device=t.device)
    strides, acc = [0] * t.dim(), 1
    for k in reversed(order):
        strides[k] = acc
        acc *= shape[k]
    return torch.empty_strided(shape, strides, dtype=t.dtype, device=t.device)


def _same_dense_block(cache, t):
    """True when piece i of `cache` (rows [i*t.shape[0], (i+1)*t.shape[0])) and `t` are the same dense memory block layout,
    i.e. a flat copy of t's storage block is the copy of the piece."""
    if t.element_size() != 4 or cache.dtype != t.dtype:
        return False
    if tuple(cache.stride()[1:]) != tuple(t.stride()[1:]) or cache.stride(0) != t.stride(0):
        return False
    # dense: the block spans exactly numel elements
    span = 1 + sum((t.shape[k] - 1) * t.stride(k) for k in range(t.dim()))
    return span == t.numel() and t.stride(0) == max(t.stride())


def graph_wanted(opts, n_sub, calibrations):
    """May a graph be RECORDED for this capture (one that is already cached is replayed unless `use_graph` is False)?
    `use_graph` = True / False forces the choice; otherwise from 24 sub-batches on (recording + instantiating costs about five
    eager passes) or when this network has been calibrated before (from the second calibration on the graph is kept)."""
    if opts.use_graph is False:
        return False
    return bool(opts.use_graph or n_sub >= 24 or calibrations > 0)


def graph_key(cal, dev, bs, inp):
    """What a recorded pass depends on: sub-batch geometry and the storage of every parameter (the graph replays
    kernels on those addresses).  Quantisation settings do not enter: during a non-sequential capture every wrapped
    module runs its RAW forward, so the same graph serves W8A8, W6A6, ... calibrations of one network -- the grid the
    reference's experiment driver walks (example/test_all.py:83-103)."""
    return (str(dev), int(bs), tuple(inp.shape[1:]), str(inp.dtype), tuple(cal.wrapped_modules),
            tuple(getattr(m, "mode", "raw") for m in cal.wrapped_modules.values()),     # all "raw", see capture_passes
            tuple(p.data_ptr() for p in cal.net.parameters()))


# ---- ... or with the ARCHITECTURE (round 6): a fresh network object replays the graph recorded for its architecture --------
# What the reference's driver times is a NEW network object calibrated once (example/test_all.py:24-34), and a process walks
# many of them (example/test_all.py:83-103: every bit setting re-creates the network).  A graph recorded on one network's
# parameter storage is useless for the next one -- but the kernel sequence of the raw sub-batch pass depends on the
# architecture only.  So the graph is recorded on a private copy of the network (the "shadow", own parameter storage, kept
# per architecture for the life of the process); a fresh network copies its parameters and buffers into the shadow's storage
# (one fused D2D copy, ~0.35 GB for ViT-B: 0.2 ms) and replays: the same kernels on the same values as its own eager pass --
# the captured tensors are bit-identical (tests/test_hip_model.py) -- without the ~110 ms of Python / dispatcher time of eight
# eager passes.  Built at the SECOND sighting of an architecture (a process that calibrates one network once never pays for
# it); P4V_ARCH_GRAPHS=0 switches it off, `use_graph` = True builds at the first.
ARCH = {}            # architecture key -> ArchRecord


def arch_key(cal, dev, bs, inp):
    sig = tuple((n, tuple(p.shape), str(p.dtype)) for n, p in cal.net.named_parameters()) + \
        tuple((n, tuple(b.shape), str(b.dtype)) for n, b in cal.net.named_buffers())
    kinds = tuple((n, type(m).__name__) for n, m in cal.wrapped_modules.items())
    return (str(dev), int(bs), tuple(inp.shape[1:]), str(inp.dtype), type(cal.net).__name__, sig, kinds)


def arch_shadow(cal, opts, dev, bs, inp, build):
    """The record of this network's architecture with this network's parameter VALUES in its shadow, or None."""
    if not opts.arch_graphs:
        return None
    rec = ARCH.setdefault(arch_key(cal, dev, bs, inp), ArchRecord())
    if id(cal.net) not in rec.nets:
        rec.nets.add(id(cal.net))
        rec.seen += 1
    if rec.unavailable:
        return None
    if rec.net is None:
        if not (build or rec.seen >= 2):
            return None
        try:
            with torch.no_grad():   # one call: the module objects are shared between the two copies
                net2, mods2 = copy.deepcopy((cal.net, dict(cal.wrapped_modules)))
        except Exception as e:  # noqa: BLE001 - a network that cannot be copied keeps its own graphs
            print(f"[ptq4vit_amd] architecture graph unavailable ({type(e).__name__}: {e})")
            rec.unavailable = True
            return None
        for m in mods2.values():
            for a in CACHES:
                m.__dict__.pop(a, None)
            m.mode = "raw"
        for p in net2.parameters():
            p.requires_grad_(False)
        rec.net, rec.mods, rec.lanes = net2, mods2, []
    sync_shadow(cal.net, rec)
    return rec


def sync_shadow(net, rec):
    """This network's parameter / buffer VALUES into the storage the architecture's graphs replay on."""
    src = [p.data for p in net.parameters()] + [b for b in net.buffers()]
    dst = [p.data for p in rec.net.parameters()] + [b for b in rec.net.buffers()]
    with torch.no_grad():
        torch._foreach_copy_(dst, src)


def record_lane(cal, dev, bs, inp, raw_pred_softmax, shadow=None):
    """Record ONE sub-batch forward + KL backward with hooks on EVERY wrapped module (so that any group of modules, on
    any later calibration, can be served from it).  Returns the Lane or None when graph capture is unavailable.
    `shadow`: record on the architecture's private copy of the network instead of on this one."""
    from .quant_calib import _register
    mods = cal.wrapped_modules if shadow is None else shadow.mods
    net = cal.net if shadow is None else shadow.net
    # (a module whose step 2 has run -- here, or on its owner rank before the interval exchange -- has had its cache
    # attributes DELETED, reference linear.py:554; the hooks below expect them to exist)
    missing = object()
    saved = {n: tuple(m.__dict__.get(a, missing) for a in CACHES) for n, m in mods.items()}

    def reset():
        for m in mods.values():
            forget_caches(m)

    inv_n = torch.full((bs,), 1.0 / min(bs, cal._ref_bs()), device=dev)      # graph passes are whole sub-batches

    def one_pass(x, tgt):
        x.grad = None
        cal._kl_loss(net(x), tgt, inv_n).backward()

    hooks = []
    for m in mods.values():
        hooks += _register(m, hasattr(m, "metric"))
    lane = None
    try:
        static_in = inp[:bs].to(dev).clone().requires_grad_(True)
        static_tgt = raw_pred_softmax[:bs].clone()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        reset()
        with torch.cuda.stream(side):            # warm-up outside the graph (allocator, autograd, library handles)
            one_pass(static_in, static_tgt)
        torch.cuda.current_stream(dev).wait_stream(side)
        reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            one_pass(static_in, static_tgt)
        # the hooks ran once, during capture: what they appended are the graph's static output tensors
        statics = {}
        for n, m in mods.items():
            with_g = hasattr(m, "metric") and m.raw_grad is not None
            if isinstance(m, MinMaxQuantMatMul):
                stat = [m.raw_input[0][0], m.raw_input[1][0], m.raw_out[0]]
            else:
                stat = [m.raw_input[0], m.raw_out[0]]
            if with_g:
                stat.append(m.raw_grad[0])
            statics[n] = (stat, with_g)
        lane = Lane(graph, static_in, static_tgt, inv_n, statics, {}, {})
    except Exception as e:  # pragma: no cover - depends on the runtime
        print(f"[ptq4vit_amd] graph capture unavailable ({type(e).__name__}: {e}); eager capture")
    finally:
        for h in hooks:
            h.remove()
        for n, m in mods.items():
            for a, v in zip(CACHES, saved[n]):
                if v is missing:
                    m.__dict__.pop(a, None)
                else:
                    setattr(m, a, v)
    return lane


def lanes_for(cal, opts, dev, bs, inp, raw_pred_softmax, n_sub):
    """(lanes, shadow) this capture replays -- the network's own cached lanes, else the architecture's, else a fresh recording
    on the network itself -- or (None, None): eager.  `shadow` is the ArchRecord when the lanes are the architecture's."""
    cache = cal.net.__dict__.setdefault("_p4v_capture_graphs", {})
    key = graph_key(cal, dev, bs, inp)
    lanes = cache.get(key)
    if lanes is not None:
        shadow = cal.net.__dict__.get("_p4v_capture_shadow")
        if shadow is None or lanes is not shadow.lanes:
            return lanes, None
        sync_shadow(cal.net, shadow)      # (the graphs are the architecture's: this network's values into their storage, every time)
        return lanes, shadow
    wanted = graph_wanted(opts, n_sub, calibrations=cal.net.__dict__.get("_p4v_calibrations", 0))
    shadow = arch_shadow(cal, opts, dev, bs, inp, build=wanted)
    if shadow is not None and not shadow.lanes:
        lane = record_lane(cal, dev, bs, inp, raw_pred_softmax, shadow)
        if lane is None:
            shadow.unavailable, shadow.net, shadow.mods = True, None, None
            shadow = None
        else:
            shadow.lanes.append(lane)
    if shadow is not None:
        cache.clear()
        cache[key] = shadow.lanes
        cal.net.__dict__["_p4v_capture_shadow"] = shadow
        return shadow.lanes, shadow
    lane = record_lane(cal, dev, bs, inp, raw_pred_softmax) if wanted else None
    if lane is None:
        return None, None
    cache.clear()                      # one geometry per network at a time: a graph pins its activations' memory
    cache[key] = [lane]
    return cache[key], None


def replay(mods, names, lanes, inp, raw_pred_softmax, bs, dev, tick):
    """Caches for `names` on the modules `mods`, filled by one replay per sub-batch of `inp`, sub-batch i on lane i % len(lanes):
    the recipe (one made for another number of sub-batches is rebuilt in place), the caches, every lane's copy table, the loop."""
    from .. import engine
    total, key_names = inp.shape[0], tuple(names)
    n_sub, n_lanes, lane0 = total // bs, len(lanes), lanes[0]
    recipe = lane0.recipes.get(key_names)
    if recipe is None or recipe.n_sub != n_sub:
        layout, is_block = [], []
        for n in names:
            for t in lane0.statics[n][0]:
                c = _cache_like(t, n_sub)
                layout.append((tuple(c.shape), tuple(c.stride()), t.dtype))
                is_block.append(_same_dense_block(c, t))
                del c
        recipe = lane0.recipes[key_names] = Recipe(n_sub, layout, is_block)
    flat_dsts, k_ = [], 0
    for n in names:
        m = mods[n]
        stat, with_g = lane0.statics[n]
        full = []
        for _t in stat:
            shp, strd, dt = recipe.layout[k_]
            full.append(torch.empty_strided(shp, strd, dtype=dt, device=dev))
            k_ += 1
        d_ = m.__dict__                        # (plain tensors: what nn.Module.__setattr__ ends up doing, without its checks)
        if isinstance(m, MinMaxQuantMatMul):
            d_["raw_input"], d_["raw_out"] = [full[0], full[1]], full[2]
        else:
            d_["raw_input"], d_["raw_out"] = full[0], full[1]
        if hasattr(m, "metric"):
            d_["raw_grad"] = full[-1] if with_g else None
        flat_dsts += full
    plans = []
    for lane in lanes:
        srcs = []
        for n in names:
            srcs += lane.statics[n][0]
        # every (static tensor -> slice i of its cache) whose memory is one dense block goes through ONE launch per
        # sub-batch (p4v_multi_copy); anything else (overlapping / gapped views) keeps torch's copy
        # (the recipe's flags were computed from lane 0's recorded tensors; another instance of the graph may have recorded
        # one of them with other strides -- then the flat copy would scramble the cache: each lane's flags are checked
        # against ITS statics once and kept with the lane)
        lane_blocks = lane.is_block.get(key_names)
        if lane_blocks is None:
            lane_blocks = [bool(b) and _same_dense_block(d, t) for d, t, b in zip(flat_dsts, srcs, recipe.is_block)]
            lane.is_block[key_names] = lane_blocks
        block = [(d, t) for d, t, b in zip(flat_dsts, srcs, lane_blocks) if b]
        other = [(d, t) for d, t, b in zip(flat_dsts, srcs, lane_blocks) if not b]
        table, max_bytes = None, 0
        if block:
            rows = [[t.data_ptr(), d.data_ptr(), t.numel() * 4] for d, t in block]
            table = torch.tensor(rows, dtype=torch.int64).to(dev, non_blocking=True)
            max_bytes = max(r[2] for r in rows)
        plans.append((lane, table, len(block), max_bytes, other))
    tick(lambda: f"caches allocated ({sum(d.numel() * 4 for d in flat_dsts) / 2**30:.1f} GiB)")
    main = torch.cuda.current_stream(dev)
    streams = [main] if n_lanes == 1 else engine.side_streams(dev, n_lanes)
    for s_ in streams:
        if s_ is not main:
            s_.wait_stream(main)          # the caches / tables / targets were produced on the current stream
    for i, st in enumerate(range(0, total, bs)):
        lane, table, n_block, max_bytes, other = plans[i % n_lanes]
        with torch.cuda.stream(streams[i % n_lanes]):
            with torch.no_grad():
                lane.static_in.copy_(inp[st:st + bs])
            lane.static_tgt.copy_(raw_pred_softmax[st:st + bs])
            lane.graph.replay()
            if table is not None:
                engine.multi_copy(table, n_block, i, max_bytes, dev)
                if i < n_lanes:
                    table.record_stream(streams[i % n_lanes])     # read on a lane's stream, released without a host sync
            for d, t in other:
                d[i * t.shape[0]:(i + 1) * t.shape[0]].copy_(t)
    for s_ in streams:
        if s_ is not main:
            main.wait_stream(s_)
    tick(lambda: f"{n_sub} replays + appends on {n_lanes} stream(s)")


def _ticker(trace, dev):
    """P4V_CAPTURE_TRACE=1: the wall time of every phase (behind a device synchronisation) on stderr."""
    t_prev = [time.time()]

    def tick(label):
        if trace:
            torch.cuda.synchronize(dev)
            print(f"[capture] {label()}: {time.time() - t_prev[0]:.3f} s", file=sys.stderr, flush=True)
            t_prev[0] = time.time()
    return tick


def capture_passes(cal, opts, names, dev, bs, raw_pred_softmax):
    """The sub-batch forward + KL backward of `cal`'s calibration set replayed from HIP graphs into the caches of `names`.
    Returns False -- the caller runs the eager passes -- if the loader is not a single batch divisible into at least two equal
    sub-batches, if `use_graph` is False, if a module is not in raw mode, or if no graph is cached and none is to be recorded
    (`graph_wanted`) or can be."""
    batches = [inp for inp, _ in cal.calib_loader]
    if len(batches) != 1 or batches[0].shape[0] % bs != 0 or batches[0].shape[0] // bs < 2:
        return False
    inp = batches[0]
    n_sub = inp.shape[0] // bs
    if opts.use_graph is False:
        return False
    # The recorded pass is the RAW forward of every wrapped module (`graph_key`).  A network that is re-calibrated
    # while modules are still in "quant_forward" (neither the reference nor `_calibrate` resets the modes) captures
    # quantised forwards on the eager path; a graph would replay raw ones, or bake in kernels that read interval
    # tensors which the next step 2 replaces.  Only the all-raw state is served from a graph.
    if any(getattr(m, "mode", "raw") != "raw" for m in cal.wrapped_modules.values()):
        return False
    tick = _ticker(opts.capture_trace, dev)
    lanes, shadow = lanes_for(cal, opts, dev, bs, inp, raw_pred_softmax, n_sub)
    if lanes is None:
        return False
    # A pass at 4 images is a chain of ~1500 kernels of a few microseconds each: the GPU is mostly idle while it runs.
    # `capture_lanes` instances of the graph (own static tensors each) replay different sub-batches on different
    # streams at the same time; every sub-batch still runs exactly the recorded kernels, so the caches do not change.
    want = max(1, min(opts.capture_lanes, n_sub))
    while len(lanes) < want:
        lane = record_lane(cal, dev, bs, inp, raw_pred_softmax, shadow)
        if lane is None:
            break
        lanes.append(lane)
    tick(lambda: f"graphs ready ({len(lanes)} instance(s))")
    replay(cal.wrapped_modules, names, lanes[:want], inp, raw_pred_softmax, bs, dev, tick)
    return True
