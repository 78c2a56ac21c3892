"""Calibration orchestrators -- API mirror of the reference's utils/quant_calib.py.

``HessianQuantCalibrator.batching_quant_calib()`` (reference quant_calib.py:300-378) is the entry point every
reference experiment uses.  Differences in HOW (not WHAT):

* capture is ONE set of forward/backward sub-batch passes hooking every module this rank owns, with the
  hooked tensors kept on the GPU (the reference repeats the whole set of passes once per module and moves
  every hooked tensor to the host, quant_calib.py:317-356).  With ``sequential=False`` every module stays in
  "raw" mode during capture, so the captured tensors are identical either way;
* ``module.calibration_step2()`` runs on the GPU through the C ABI;
* with ``torch.distributed`` initialised the modules are sharded over the ranks (one process per GPU) and the
  calibrated intervals are exchanged with one all-gather at the end (ptq4vit_amd/utils/shard.py).

The knobs of a calibration are decided once, in `calib_options` (attribute on the calibrator, then environment variable, then
default); the capture passes served from HIP graphs live in utils/capture_graph.py.
"""
import os
import threading
import time
from collections import namedtuple
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from ..quant_layers.conv import MinMaxQuantConv2d
from ..quant_layers.linear import MinMaxQuantLinear
from ..quant_layers.matmul import MinMaxQuantMatMul
from . import capture_graph, shard
from .capture_graph import _cache_like, _same_dense_block, forget_caches  # noqa: F401 - the first two are re-exported

try:
    from tqdm import tqdm
except Exception:  # pragma: no cover
    def tqdm(x, **k):
        return x


_HWQ_WARNED = False


def _warn_hw_queues(n_streams):
    """Once per process: the default of 4 search streams + 3 capture lanes was tuned with GPU_MAX_HW_QUEUES=8
    (ptq4vit_amd.configure_runtime(), before the first GPU use); with the runtime's 4 hardware queues streams share queues
    and their kernels serialise (~6 % on ViT-B/224 x 32).  Nothing is changed here -- a library must not touch the
    environment of other HIP users in the process -- the caller is told."""
    global _HWQ_WARNED
    if _HWQ_WARNED or n_streams <= 1 or os.environ.get("GPU_MAX_HW_QUEUES"):
        return
    _HWQ_WARNED = True
    import warnings
    warnings.warn(f"ptq4vit_amd: {n_streams} search streams but GPU_MAX_HW_QUEUES is unset (runtime default: 4 hardware queues); "
                  "call ptq4vit_amd.configure_runtime() before the first GPU use, or export GPU_MAX_HW_QUEUES=8", stacklevel=3)


@dataclass(frozen=True)
class CalibOptions:
    """The knobs of one calibration, decided once (`calib_options`).  DESIGN.md §6 has the table of name, attribute, environment
    variable and default."""
    use_graph: object        # True / False force the capture graph on / off, None: capture_graph.graph_wanted decides
    capture_lanes: int       # instances of the capture graph replayed side by side
    search_streams: int      # modules searched at a time; 1 also selects ONE group call
    search_grouped: object   # p4v_calibrate_group calls instead of one calibration_step2 per module
    group_calls: int         # concurrent group calls; <= 0: one for a small calibration, else three (`n_group_calls`)
    shard_capture: object    # True = sub-batch sharded capture, False = replicated, None = shard.choose_capture_mode
    arch_graphs: bool        # a fresh network replays the graph of its architecture
    group_gib: float         # scratch of all concurrent group calls together, GiB at most
    capture_trace: bool      # phase times of the graph capture and the place of an out-of-memory error on stderr / stdout

    def n_group_calls(self, cache_bytes):
        """`cache_bytes()` -> bytes of the group's captured tensors, asked only for the automatic choice: three concurrent calls
        overlap each other's small kernels and round trips (ViT-B/224 x 32: 127 ms with one call, 112 with three; ViT-S x 32:
        68.7 / 62.7; DeiT-tiny x 32: 44.3 / 41.2); a calibration whose captured tensors are a few hundred MB is issue-bound and
        pays for every extra round instead (DeiT-tiny BasePTQ x 4, BASELINE config 0: 5 rounds / 27.7 ms with one call,
        15 rounds / 29.4 ms with three)."""
        if self.search_streams == 1:     # (the launch order bench.py's roofline records describe)
            return 1
        if self.group_calls > 0:
            return self.group_calls
        return 1 if cache_bytes() < (512 << 20) else 3


def calib_options(cal):
    """Every knob from (attribute on the calibrator, then environment variable, then default).  The attributes are None after
    construction and may be set at any time before the calibration; `capture_lanes`, `search_streams` and `group_calls` fall
    through to the environment when None or 0."""
    env = os.environ.get
    shard_env = env("P4V_SHARD_CAPTURE", "auto")      # "1" / "0" force, anything else is auto
    return CalibOptions(
        use_graph=cal.use_graph,
        capture_lanes=int(cal.capture_lanes or env("P4V_CAPTURE_LANES", "3")),
        search_streams=cal.search_streams or int(env("P4V_SEARCH_STREAMS", "4")),
        search_grouped=cal.search_grouped if cal.search_grouped is not None else env("P4V_GROUPED", "1") != "0",
        group_calls=cal.group_calls or int(env("P4V_GROUP_CALLS", "0")),
        shard_capture=cal.shard_capture if cal.shard_capture is not None else {"1": True, "0": False}.get(shard_env),
        arch_graphs=env("P4V_ARCH_GRAPHS", "1") != "0",
        group_gib=float(env("P4V_GROUP_GIB", "150")),
        capture_trace=env("P4V_CAPTURE_TRACE") == "1")


# What is fixed for one `_calibrate` call.  `all_sizes`: {module: cache bytes} of EVERY module when the modules are sharded over
# ranks, else None; `shard_cap`: sub-batch sharded capture (every rank enters shard.exchange_captures).
_Calibration = namedtuple("_Calibration", "opts batching with_grad rank world names owner all_sizes n_sub shard_cap raw_pred_softmax")


def _dev_of(net):
    for p in net.parameters():
        return p.device
    return torch.device("cpu")


# ---- hook functions (reference quant_calib.py:173-201); tensors stay on their device ------------------
def grad_hook(module, grad_input, grad_output):
    if module.raw_grad is None:
        module.raw_grad = []
    module.raw_grad.append(grad_output[0].detach())


def _with_output_grad(forward_hook):
    """Forward hook that also records the gradient w.r.t. the module output -- what the reference's
    register_backward_hook(grad_hook) (quant_calib.py:330) delivers as grad_output[0] -- through a tensor hook on
    the output.  Same tensor, without the two extra autograd nodes per module call that
    register_full_backward_hook inserts (the capture pass is launch-overhead bound)."""
    def hook(module, input, output):
        forward_hook(module, input, output)
        if output.requires_grad:
            output.register_hook(lambda g, m=module: grad_hook(m, None, (g,)))
    return hook


def linear_forward_hook(module, input, output):
    if module.raw_input is None:
        module.raw_input = []
    if module.raw_out is None:
        module.raw_out = []
    module.raw_input.append(input[0].detach())
    module.raw_out.append(output.detach())


conv2d_forward_hook = linear_forward_hook


def matmul_forward_hook(module, input, output):
    if module.raw_input is None:
        module.raw_input = [[], []]
    if module.raw_out is None:
        module.raw_out = []
    module.raw_input[0].append(input[0].detach())
    module.raw_input[1].append(input[1].detach())
    module.raw_out.append(output.detach())


def _register(module, with_grad):
    hooks = []
    wrap = _with_output_grad if with_grad else (lambda h: h)
    if isinstance(module, MinMaxQuantLinear):
        hooks.append(module.register_forward_hook(wrap(linear_forward_hook)))
    if isinstance(module, MinMaxQuantConv2d):
        hooks.append(module.register_forward_hook(wrap(conv2d_forward_hook)))
    if isinstance(module, MinMaxQuantMatMul):
        hooks.append(module.register_forward_hook(wrap(matmul_forward_hook)))
    return hooks


def _concat(module, with_grad):
    """Lists of per-sub-batch tensors -> one tensor per cache (reference quant_calib.py:343-354)."""
    cat = lambda t: t[0] if len(t) == 1 else torch.cat(t, dim=0)   # a single piece needs no copy
    if isinstance(module, MinMaxQuantMatMul):
        module.raw_input = [cat(t) for t in module.raw_input]
    else:
        module.raw_input = cat(module.raw_input)
    module.raw_out = cat(module.raw_out)
    if with_grad:
        module.raw_grad = cat(module.raw_grad)


def _groupable(m):
    """May the calibrator replace this module's calibration_step2() by calibration_job() / p4v_calibrate_group / calibration_install()?
    Only while calibration_step2 IS the library's own method: an instance attribute or a subclass override (a user's hook around
    the search, a test's recorder) is called as the reference calls it, alone."""
    if "calibration_step2" in m.__dict__ or not hasattr(m, "calibration_job"):
        return False
    return getattr(getattr(type(m), "calibration_step2", None), "_p4v_grouped", False)


def _operands(m):
    """The cached input(s) of a module as a list: two for a MatMul, one otherwise."""
    ri = m.raw_input
    return list(ri) if isinstance(ri, (list, tuple)) else [ri]


def _calibrated_and_freed(m):
    """Step 2 has run: the module carries `calibrated` and its caches are deleted (reference linear.py:554)."""
    return hasattr(m, "calibrated") and not hasattr(m, "raw_out")


def _prep_is_copy_free(m):
    """Does preparing this module's group job launch no torch kernel on captured data (every cached tensor dense fp32 on the
    device: no `.contiguous()` / `.to()` copy)?"""
    dense = lambda t: t is None or (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous())
    ins = _operands(m)
    if len(ins) == 1 and not dense(ins[0]):          # (matmul operands are read through their strides)
        return False
    w = getattr(m, "weight", None)
    return (all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in ins) and dense(m.raw_out)
            and dense(getattr(m, "raw_grad", None)) and (w is None or dense(w.data)) and _groupable(m))


def _search_work(m):
    """Size of what a search sweeps (rows x K x N): the LPT order of a network that has no measured times yet."""
    ins = _operands(m)
    if len(ins) == 2:                                           # matmul: batch*heads x M x K x N
        a, b = ins
        return float(a.numel()) * b.shape[-1] * (0.2 if a.shape[-1] <= 64 else 1.0)
    ri, w = ins[0], getattr(m, "weight", None)
    return float(ri.numel()) / max(1, ri.shape[-1] if ri.dim() != 4 else 1) * (w.numel() if w is not None else 1) / (1 if ri.dim() != 4 else ri.shape[1])


def plan_groups(todo, sizes, budget, sequential, shard_cap):
    """Modules captured (and searched) together: greedily as many of `todo`, in order, as `sizes` fit into `budget` bytes -- a
    module larger than the budget stands alone.  `sizes` is not read when `sequential` or `shard_cap`."""
    if sequential:
        return [[n] for n in todo]  # predecessors must already run quantised: one capture per module
    if shard_cap:
        return [todo]               # one exchange, then everything this rank owns (possibly nothing)
    out, cur, acc = [], [], 0
    for n in todo:
        if cur and acc + sizes.get(n, 0) > budget:
            out.append(cur)
            cur, acc = [], 0
        cur.append(n)
        acc += sizes.get(n, 0)
    if cur:
        out.append(cur)
    return out


def deal_over_calls(names, kinds, n_calls):
    """Modules of one kind (`kinds[name]`) are dealt over the group calls, so that every call holds the same mixture (and its
    launches group); within a kind in the order of `names`."""
    order = sorted(names, key=lambda n: (str(kinds[n]), names.index(n)))
    return [order[i::n_calls] for i in range(n_calls)]


class QuantCalibrator:
    """Reference quant_calib.py:9-171: forward-mode calibration (calibration_step1 / calibration_step2(x))."""

    def __init__(self, net, wrapped_modules, calib_loader, sequential=True):
        self.net = net
        self.wrapped_modules = wrapped_modules
        self.calib_loader = calib_loader
        self.sequential = sequential
        self.calibrated = False

    def _run_loader(self):
        dev = _dev_of(self.net)
        with torch.no_grad():
            for inp, _ in self.calib_loader:
                self.net(inp.to(dev))

    def sequential_quant_calib(self):
        """Reference quant_calib.py:28-55: TWO passes over the calibration set.  Pass 1: every module in "calibration_step1"
        (raw forward; caches raw_input / raw_out of the RAW network).  Pass 2: every module in "calibration_step2": module k
        calibrates on the input it receives in this pass -- the output of its predecessors' calibration_step2, i.e. their
        quantised forward -- against the raw_out cached in pass 1.  Modules that already carry `calibrated` are left alone
        in pass 1 and run raw in pass 2 (the reference compares `step == 2` inside `range(2)`: a dead branch, kept)."""
        for step in range(2):
            print(f"Start calibration step={step + 1}")
            for module in self.wrapped_modules.values():
                if hasattr(module, "calibrated"):
                    if step == 1:
                        module.mode = "raw"
                else:
                    module.mode = f"calibration_step{step + 1}"
            self._run_loader()
        for module in self.wrapped_modules.values():
            module.mode = "quant_forward"
        print("sequential calibration finished")

    def parallel_quant_calib(self):
        """Reference quant_calib.py:57-93: one raw pass caches every module's raw_input / raw_out, then each module runs
        calibration_step2 on ITS OWN cached raw input (the module is called directly, not through the network)."""
        print("Start calibration step=1")
        for module in self.wrapped_modules.values():
            module.mode = "raw" if hasattr(module, "calibrated") else "calibration_step1"
        self._run_loader()
        dev = _dev_of(self.net)
        for name, module in tqdm(self.wrapped_modules.items(), desc="Calibration"):
            if hasattr(module, "calibrated"):
                continue
            module.mode = "calibration_step2"
            with torch.no_grad():
                if isinstance(module, MinMaxQuantMatMul):
                    module.forward(module.raw_input[0].to(dev), module.raw_input[1].to(dev))
                else:
                    module.forward(module.raw_input.to(dev))
        for module in self.wrapped_modules.values():
            module.mode = "quant_forward"
        print("calibration finished")

    def quant_calib(self):
        print(f"prepare parallel calibration for {list(self.wrapped_modules)}")
        if self.sequential:
            self.sequential_quant_calib()
        else:
            self.parallel_quant_calib()
        self.calibrated = True

    def batching_quant_calib(self):
        """Cached-tensor calibration without gradients (reference :95-171); any non-hessian metric.  One forward pass
        over the loader's own batches fills the caches, then every module runs calibration_step2()."""
        h = HessianQuantCalibrator(self.net, self.wrapped_modules, self.calib_loader, sequential=self.sequential,
                                   batch_size=getattr(self.calib_loader, "batch_size", None) or 1)
        h._calibrate(batching=True, with_grad=False)
        self.calibrated = True


class HessianQuantCalibrator(QuantCalibrator):
    """Reference quant_calib.py:203-378."""

    def __init__(self, net, wrapped_modules, calib_loader, sequential=False, batch_size=1,
                 cache_budget_bytes=None, capture_batch_size=None):
        super().__init__(net, wrapped_modules, calib_loader, sequential=sequential)
        self.batch_size = batch_size
        # images per capture pass; None = `batch_size`, the reference's passes (quant_calib.py:333-339).  A larger value
        # (a multiple of batch_size) runs fewer, larger passes -- a pass of 4 images is launch-bound on this GPU (8 ms for
        # 2 ms of arithmetic on ViT-B) -- with the KL loss weighted per sample by 1 / (rows of the reference sub-batch the
        # sample belongs to), i.e. what "batchmean" over that sub-batch divides by: raw_input / raw_out and, for a given
        # target distribution, raw_grad are those of the reference's passes up to GEMM rounding.  It is NOT the default
        # because of what the target is: with every module in raw mode the prediction equals the target up to rounding, so
        # raw_grad of a non-sequential calibration is rounding noise of the (batch_size-image pass) - (whole-batch pass)
        # logit difference, in the reference as here, and its realisation changes with the shape of the passes.
        self.capture_batch_size = capture_batch_size
        # bytes of captured tensors kept resident at a time; None = what the GPU has free minus head room for the search
        # workspaces and the capture pass itself (288 GB of HBM3E hold the 207 GB of Swin-B/384 x 128 images in ONE group;
        # every further group repeats the whole capture pass)
        self.cache_budget_bytes = cache_budget_bytes
        # the knobs (`calib_options`): None = the environment variable, then the default; settable until the calibration starts
        self.use_graph = self.capture_lanes = self.search_streams = None
        self.search_grouped = self.group_calls = self.shard_capture = None
        self.timings = {}

    SEARCH_HEADROOM_BYTES = 44 << 30

    def _resolve_budget(self):
        """Bytes of captured tensors resident at a time: what the GPU has free minus head room for the search workspaces."""
        if self.cache_budget_bytes is not None:
            return int(self.cache_budget_bytes)
        dev = _dev_of(self.net)
        if dev.type != "cuda":
            return 96 << 30
        # The engine's scratch buffers persist between calibrations (keyed by stream and group member).  A grouped search of a
        # 128-image configuration leaves > 100 GiB of them behind (Swin-B/384 x 128: 184 GiB): the next network's caches then do
        # not fit next to them, the capture is split into groups and every group repeats the whole capture pass (round 6: 10-36 s
        # per calibration instead of 6).  Buffers of that size go back to torch's pool here; the search takes what it needs
        # from the same pool again (`_search_grouped` sizes its scratch to what is free once the caches are resident).
        from .. import engine
        if engine.workspace_bytes(dev) > (16 << 30):
            engine.release_workspace()
        free, _total = torch.cuda.mem_get_info(dev)
        pooled = torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)    # cached by torch's allocator: reusable
        return max(8 << 30, int(free + pooled) - self.SEARCH_HEADROOM_BYTES)

    # ---- capture ------------------------------------------------------------------------------------
    def _ref_bs(self):
        return getattr(self, "batch_size", None) or self.calib_loader.batch_size

    def _capture_bs(self):
        """Images per capture pass: the reference sub-batch, or the multiple of it asked for by `capture_batch_size`."""
        bs = self._ref_bs()
        cbs = getattr(self, "capture_batch_size", None)
        return bs if not cbs else max(bs, (int(cbs) // bs) * bs)

    @staticmethod
    def _kl_loss(pred, target, inv_n):
        """Sum over samples of KL(target || softmax(pred)) / n(sample), n = rows of the reference sub-batch the sample is
        in: the gradients of the reference's per-sub-batch F.kl_div(..., reduction="batchmean") (quant_calib.py:333-339)
        for all of its sub-batches at once."""
        kl = F.kl_div(F.log_softmax(pred, dim=-1), target, reduction="none").sum(dim=-1)
        return (kl * inv_n).sum()

    @staticmethod
    def _inv_rows(total, st, n, ref_bs, dev):
        """1 / (rows of the reference sub-batch) for samples st .. st+n of a loader batch of `total` images."""
        j = torch.arange(st, st + n, device=dev)
        rows = torch.clamp(total - (j // ref_bs) * ref_bs, max=ref_bs)
        return 1.0 / rows.to(torch.float32)

    def _raw_pred_softmax(self):
        dev = _dev_of(self.net)
        with torch.no_grad():
            for inp, _ in self.calib_loader:
                raw_pred = self.net(inp.to(dev))
                raw_pred_softmax = F.softmax(raw_pred, dim=-1).detach()
        return raw_pred_softmax

    def _capture(self, names, raw_pred_softmax, with_grad, stride=None, opts=None):
        """Forward (+ backward of the KL loss, reference :333-339) over the calibration set in sub-batches,
        with hooks on `names` only.  `stride = (r, w)`: run only the sub-batches i with i % w == r and leave the
        per-sub-batch pieces on the modules as lists (sub-batch sharded capture, shard.exchange_captures).
        `opts`: the calibration's options; a direct call (tests, tools) decides its own."""
        opts = opts or calib_options(self)
        dev = _dev_of(self.net)
        bs = self._capture_bs()
        for n in names:
            forget_caches(self.wrapped_modules[n])   # step 2 deletes the caches: re-create for re-calibration
        # Only gradients w.r.t. ACTIVATIONS are captured (grad_hook): no parameter gradient is ever looked at.  For the
        # duration of the capture NO parameter requires grad (no weight-gradient GEMMs -- a third of the backward pass --
        # no bias / LayerNorm reductions, no .grad accumulation); the graph hangs off the input images instead, which
        # are marked as requiring grad, so every hooked output still receives exactly the same grad_output.
        frozen = []
        if with_grad:
            for prm in self.net.parameters():
                if prm.requires_grad:
                    prm.requires_grad_(False)
                    frozen.append(prm)
        try:
            # the passes replayed from HIP graphs kept with the network or its architecture (utils/capture_graph.py) ...
            if stride is None and with_grad and dev.type == "cuda" and not self.sequential:
                if capture_graph.capture_passes(self, opts, names, dev, bs, raw_pred_softmax):
                    return
            hooks = []                                 # ... or run eagerly under hooks
            for n in names:
                m = self.wrapped_modules[n]
                hooks += _register(m, with_grad and hasattr(m, "metric"))
            try:
                self._capture_passes(dev, bs, raw_pred_softmax, with_grad, stride)
            finally:
                for h in hooks:
                    h.remove()
        finally:
            for wt in frozen:
                wt.requires_grad_(True)
        if stride is not None:
            return
        for n in names:
            m = self.wrapped_modules[n]
            _concat(m, with_grad and hasattr(m, "metric"))

    _ARCH = capture_graph.ARCH      # architecture key -> capture_graph.ArchRecord: the one table, for the life of the process

    def _capture_passes(self, dev, bs, raw_pred_softmax, with_grad, stride=None):
        i = -1
        for inp, _ in self.calib_loader:
            total = inp.shape[0]
            for st in range(0, total, bs):
                i += 1
                if stride is not None and i % stride[1] != stride[0]:
                    continue
                inp_ = inp[st:st + bs].to(dev)
                if with_grad:
                    inp_ = inp_.detach().requires_grad_(True)     # root of the autograd graph (parameters are frozen)
                    inv_n = self._inv_rows(total, st, inp_.shape[0], self._ref_bs(), dev)
                    self._kl_loss(self.net(inp_), raw_pred_softmax[st:st + bs], inv_n).backward()
                else:
                    with torch.no_grad():
                        self.net(inp_)

    # ---- search -------------------------------------------------------------------------------------
    def _on_side_streams(self, names, n_streams, body, inputs_ready=None, on_caller=False):
        """What both searches of independent modules share: `n_streams` persistent side streams behind the capture, one host
        thread per stream running `body(i, errors, inputs_ready)` under stream i and no_grad, the first error re-raised on the
        calling thread after everything has been joined and synchronised.  `on_caller`: a single stream's body runs on the
        calling thread.  `inputs_ready`: the event recorded behind the capture passes; it is handed on to the bodies -- which then
        start while the capture is still on the GPU -- only when preparing the calls launches no torch kernel on captured data
        (`_prep_is_copy_free`); otherwise, and without an event, the streams wait first and the bodies get None."""
        from .. import engine
        dev = _dev_of(self.net)
        main = torch.cuda.current_stream(dev)
        _warn_hw_queues(n_streams)
        streams = engine.side_streams(dev, n_streams)
        if not hasattr(self, "_module_ms"):
            self._module_ms = {}
        mods = [self.wrapped_modules[n] for n in names]
        if inputs_ready is None or not all(_prep_is_copy_free(m) for m in mods):
            inputs_ready = None
            for s in streams:
                s.wait_stream(main)                   # the captured tensors were produced on the current stream
        # the caches are freed by calibration_step2 (reference linear.py:554) while the other stream may still be
        # running: hold them until everything has been joined so that the allocator cannot hand the memory out again
        keep = [(m.raw_input, m.raw_out, getattr(m, "raw_grad", None)) for m in mods]
        errors = []

        def run(i):
            try:
                torch.cuda.set_device(dev)
                with torch.cuda.stream(streams[i]), torch.no_grad():
                    body(i, errors, inputs_ready)
            except BaseException as e:  # noqa: BLE001 - re-raised on the calling thread
                errors.append(e)

        if on_caller and n_streams == 1:
            run(0)
        else:
            threads = [threading.Thread(target=run, args=(i,)) for i in range(n_streams)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
        for s in streams:
            main.wait_stream(s)
        torch.cuda.synchronize(dev)
        del keep
        if errors:
            raise errors[0]

    def _search_concurrent(self, names, n_streams):
        """Independent modules (sequential=False) searched `n_streams` at a time, one host thread + HIP stream each.

        A search is a chain of ~50 kernels with a host round trip after every pass (the pass memo reads the selected
        interval back); with a single stream the GPU idles during those round trips, during the small
        finish/select kernels and in the tail of every sweep (1200 workgroups on 256 CUs).  A second stream fills
        these holes with another module's kernels.  Results do not depend on the interleaving: the kernels are
        deterministic and every call has its own scratch (engine.workspace is per stream).
        """
        todo = list(names)
        measured = (self.net.__dict__.get("_p4v_module_ms") or {}).get("ms", {})   # {"world", "ms"}: see _exchange
        if all(n in measured for n in names):
            todo.sort(key=lambda n: measured[n], reverse=True)        # what each search took last time on this network
        else:
            # longest first (by the size of what a search sweeps), so that the last modules in flight are the
            # small ones and the streams run dry together; the results do not depend on the order
            todo.sort(key=lambda n: _search_work(self.wrapped_modules[n]), reverse=True)
        lock = threading.Lock()

        def body(_i, errors, _inputs_ready):
            while True:
                with lock:
                    if not todo or errors:
                        return
                    n = todo.pop(0)
                module = self.wrapped_modules[n]
                t_mod = time.perf_counter()
                module.calibration_step2()
                module.mode = "raw"
                self._module_ms[n] = (time.perf_counter() - t_mod) * 1e3

        self._on_side_streams(names, n_streams, body)

    def _search_grouped(self, names, n_calls, inputs_ready=None, opts=None):
        """Independent modules (sequential=False) searched TOGETHER: `n_calls` p4v_calibrate_group calls (one host thread + HIP
        stream each), every call running the calibration_step2 of its modules in lock step with the kernel launches of the
        same kind issued once for all of them (csrc/p4v_api.hip, Group).  Replaces the loop of the reference's calibrator
        (utils/quant_calib.py:371-372).  Results do not depend on the partition: a grouped kernel runs every module's own
        code on its own parameters and scratch.

        `inputs_ready`: the event recorded behind the capture passes.  The group calls then start while the capture is still on
        the GPU -- the library issues what needs no captured tensor first (weight abs-max, candidate tables, the 100 candidate
        planes of every Linear's weights: 8.5 GB of k_pack output per ViT-B calibration) and waits for the event on its own
        stream where the first captured tensor is read (when `_on_side_streams` allows it)."""
        from .. import engine
        opts = opts or calib_options(self)
        dev = _dev_of(self.net)
        n_calls = max(1, min(n_calls, len(names)))
        kinds = {}
        for n in names:
            m, ins = self.wrapped_modules[n], _operands(self.wrapped_modules[n])
            shp = tuple(tuple(t.shape) for t in ins) if len(ins) == 2 else tuple(ins[0].shape)
            kinds[n] = (type(m).__name__, shp, tuple(m.raw_out.shape))
        parts = deal_over_calls(names, kinds, n_calls)
        # Scratch of all concurrent group calls together: P4V_GROUP_GIB at most, and never more than what is free NOW -- the
        # captured tensors of this group are resident (their allocation is host-side and behind us) -- plus what torch's pool and
        # the engine's own kept buffers can be re-used for, minus a margin for the allocator's rounding and torch temporaries.
        # (Round 6 sized it to a constant 150 GiB: next to the 207 GB of captured tensors of Swin-B/384 x 128 the first call ran
        # out of memory three times, and the buffers it left behind starved the next calibration's caches.)
        budget_all = int(opts.group_gib * (1 << 30))
        if dev.type == "cuda":
            free, _tot = torch.cuda.mem_get_info(dev)
            pooled = torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
            avail = int(free + pooled) + engine.workspace_bytes(dev) - (6 << 30)
            if avail < budget_all:
                engine.release_workspace()      # (buffers sized for another mixture of members would be stranded next to the new ones)
                budget_all = max(4 << 30, avail)
        budget = budget_all // n_calls
        # (one call runs on the calling thread: p4v_stats_* are per calling thread -- bench.py's roofline step)
        self._on_side_streams(names, n_calls, lambda i, errors, ready: self._group_call(parts[i], budget, errors, ready),
                              inputs_ready=inputs_ready, on_caller=True)

    def _group_call(self, part, budget, errors, inputs_ready):
        """One stream's share of a grouped search: p4v_calibrate_group over as many modules of `part` at a time as their scratch
        fits into `budget` bytes."""
        from .. import engine
        todo = list(part)
        while todo and not errors:
            t_grp = time.perf_counter()
            batch, jobs, sizes, acc = [], [], {}, 0
            while todo:
                n = todo[0]
                m = self.wrapped_modules[n]
                if not _groupable(m):        # calibration_step2 overridden / a class without the two-step protocol: alone
                    if batch:
                        break
                    todo.pop(0)
                    m.calibration_step2()
                    m.mode = "raw"
                    self._module_ms[n] = (time.perf_counter() - t_grp) * 1e3
                    t_grp = time.perf_counter()
                    continue
                sizes[n] = 4 * sum(t.numel() for t in _operands(m)) + 8 * m.raw_out.numel()
                job = m.calibration_job()
                held = (int(job.need) + 4095) & ~4095          # (its share of the call's arena, engine.calibrate_group)
                if batch and acc + held > budget:              # scratch of the members so far fills the budget: next call
                    break
                todo.pop(0)
                batch.append(n); jobs.append(job); acc += held
            if not batch:
                continue
            engine.calibrate_group(jobs, inputs_ready=inputs_ready)
            for n, j in zip(batch, jobs):
                m = self.wrapped_modules[n]
                m.calibration_install(j)
                m.mode = "raw"
            ms = (time.perf_counter() - t_grp) * 1e3
            w = {n: shard.module_cost_ms(self.wrapped_modules[n], sizes[n]) for n in batch}
            tot = sum(w.values()) or 1.0
            for n in batch:                     # (the call's wall time, shared out by the cost model: next LPT plan)
                self._module_ms[n] = ms * w[n] / tot

    def _estimate_cache_bytes(self, names):
        """One cheap probe forward of a single image to size the caches of `names` (kept with the network: the sizes depend
        on the architecture and the image geometry only; every rank of a sharded calibration needs them each time)."""
        dev = _dev_of(self.net)
        geom = None
        for inp, _ in self.calib_loader:
            geom = (tuple(inp.shape[1:]), int(inp.shape[0]), tuple(self.wrapped_modules))
            break
        memo = self.net.__dict__.setdefault("_p4v_cache_sizes", {})
        if geom in memo and all(n in memo[geom] for n in names):
            return {n: memo[geom][n] for n in names}
        # ... and with the ARCHITECTURE for the life of the process: a fresh network object of a known architecture (the step the
        # reference times, example/test_all.py:24-34) does not pay the probe again -- an eager single-image forward, 3.6 ms of
        # launch latency: 3 % of a ViT-B/224 x 32 calibration, 10 % of DeiT-tiny x 4 (tools/step_breakdown.py)
        arch = (type(self.net).__name__, str(dev), geom,
                tuple((n, tuple(p_.shape)) for n, p_ in self.net.named_parameters()),
                tuple((n, type(m).__name__) for n, m in self.wrapped_modules.items()))
        known = HessianQuantCalibrator._ARCH_SIZES.get(arch)
        if known is not None and all(n in known[0] for n in names):
            for n, mn in known[1].items():
                if n in self.wrapped_modules:
                    self.wrapped_modules[n]._p4v_out_mn = mn
            memo.setdefault(geom, {}).update(known[0])
            return {n: known[0][n] for n in names}
        sizes = {}
        hooks = []

        def mk(n):
            def hook(mod, inp, out):
                numel = sum(t.numel() for t in inp if torch.is_tensor(t)) + 2 * out.numel()
                sizes[n] = numel * 4
                if out.dim() >= 2:
                    mod._p4v_out_mn = (int(out.shape[-2]), int(out.shape[-1]))       # tile geometry for shard.module_cost_ms
            return hook

        for n in names:
            hooks.append(self.wrapped_modules[n].register_forward_hook(mk(n)))
        total = 0
        with torch.no_grad():
            for inp, _ in self.calib_loader:
                total = inp.shape[0]
                self.net(inp[:1].to(dev))
                break
        for h in hooks:
            h.remove()
        out = {n: s * total for n, s in sizes.items()}
        memo.setdefault(geom, {}).update(out)
        rec = HessianQuantCalibrator._ARCH_SIZES.setdefault(arch, ({}, {}))
        rec[0].update(out)
        rec[1].update({n: self.wrapped_modules[n]._p4v_out_mn for n in out if hasattr(self.wrapped_modules[n], "_p4v_out_mn")})
        return out

    _ARCH_SIZES = {}      # architecture + image geometry -> ({module: cache bytes}, {module: (rows, columns) of its output})

    # ---- entry points ------------------------------------------------------------------------------
    def quant_calib(self):
        """Non-batching Hessian calibration (reference :216-298): same capture, then calibration_step2(x)."""
        self._calibrate(batching=False, with_grad=True)

    def batching_quant_calib(self, with_grad=True):
        self._calibrate(batching=True, with_grad=with_grad)

    def _calibrate(self, batching, with_grad):
        opts = calib_options(self)
        names = list(self.wrapped_modules)
        print(f"prepare parallel calibration for {names}")
        print("start hessian calibration")
        rank, world = shard.rank_world()
        t0 = time.time()
        owner, all_sizes = self._assign_owners(names, rank, world)
        mine = [n for n in names if owner[n] == rank]
        self.owner = owner
        raw_pred_softmax = self._raw_pred_softmax() if with_grad else None
        bs = self._capture_bs()
        n_sub = sum(-(-inp.shape[0] // bs) for inp, _ in self.calib_loader)
        shard_cap = self._sharded_capture(opts, names, owner, all_sizes, world, n_sub, with_grad)
        self.capture_mode = "sharded" if shard_cap else "replicated"
        cal = _Calibration(opts=opts, batching=batching, with_grad=with_grad, rank=rank, world=world, names=names, owner=owner,
                           all_sizes=all_sizes, n_sub=n_sub, shard_cap=shard_cap, raw_pred_softmax=raw_pred_softmax)
        budget = self._resolve_budget()
        groups = self._plan(cal, mine, budget)
        t_cap = t_cal = 0.0
        done = set()
        while groups:
            grp = groups.pop(0)
            try:
                dc, ds = self._run_group(cal, grp)
            except torch.cuda.OutOfMemoryError as oom:
                groups, budget = self._replan_after_oom(cal, oom, grp, groups, done, budget)
                continue
            done.update(grp)
            t_cap += dc
            t_cal += ds
        t_ex = self._exchange(cal)
        for module in self.wrapped_modules.values():
            module.mode = "quant_forward"
        self.net.__dict__["_p4v_calibrations"] = self.net.__dict__.get("_p4v_calibrations", 0) + 1
        self.timings = {"capture_s": t_cap, "search_s": t_cal, "exchange_s": t_ex, "total_s": time.time() - t0,
                        "modules": len(names), "owned": len(mine)}
        self.calibrated = True
        print("hessian calibration finished")

    def _assign_owners(self, names, rank, world):
        """({module: owning rank}, {module: cache bytes} of every module or None): the modules balanced over the ranks."""
        if world <= 1 or self.sequential:
            return {n: rank for n in names}, None
        # balance by predicted search time (needs every module's captured size: one single-image probe forward)
        all_sizes = self._estimate_cache_bytes(names)
        costs = {n: shard.module_cost_ms(self.wrapped_modules[n], all_sizes.get(n, 0)) for n in names}
        # from the second calibration of a network on: what every module's search actually took last time (gathered from
        # all ranks at the end of that calibration, hence the same on every rank) -- the cost model does not know whether
        # the exact pruning applies to a module (it depends on where raw_grad^2 sits), the clock does
        # Only a table that was all-gathered by a calibration of THIS world size counts (a single-process warm-up before
        # init_process_group leaves local wall-clock times behind: tagged world 1, ignored here), and because the owner map
        # drives the collectives of exchange_captures / exchange_intervals it must be the same on every rank whatever each
        # rank's history is: rank 0's costs are broadcast (a few hundred floats) before the assignment.
        measured = self.net.__dict__.get("_p4v_module_ms") or {}
        if measured.get("world") == world and all(n in measured.get("ms", {}) for n in names):
            costs = {n: float(measured["ms"][n]) for n in names}
        box = [[costs[n] for n in names]]
        shard.dist.broadcast_object_list(box, src=0)
        costs = dict(zip(names, box[0]))
        return shard.assign_modules(self.wrapped_modules, world, costs), all_sizes

    def _sharded_capture(self, opts, names, owner, all_sizes, world, n_sub, with_grad):
        """Capture plan.  Replicated (the design BASELINE.json's north_star names; False): every rank runs the same deterministic
        capture passes with hooks on its OWN modules only -- no data-path collective -- and the only exchange is the
        interval all-gather at the end.  Sharded (True): every rank runs 1/world of the sub-batch passes hooking ALL modules and
        the pieces travel to the module owners in one all_to_all (shard.exchange_captures); chosen by the cost model where
        the replicated passes would cap the speed-up.  Whether that collective is entered must be the SAME decision on every
        rank, so it is derived from rank-invariant quantities only (all_sizes covers every module on every rank; a rank that
        owns nothing, or whose own cache would need several groups, decides exactly like the others)."""
        # `shard_capture` / P4V_SHARD_CAPTURE: True / "1" = sharded, False / "0" = replicated, None / "auto" (default) = the
        # cost model of shard.choose_capture_mode (rank-invariant inputs only) where all_to_all_single works on every rank
        want_shard = opts.shard_capture
        if want_shard is None:
            # (auto: the cost model with the all_to_all rate MEASURED on this process group -- replicated, north_star's plan,
            # unless the measurement says the transfer pays; P4V_SHARD_CAPTURE=0 never touches the collective)
            want_shard = (world > 1 and not self.sequential and with_grad and all_sizes is not None
                          and shard.choose_capture_mode(self.wrapped_modules, all_sizes, world, n_sub, shard.a2a_rate_gbps()) == "sharded")
        if not (world > 1 and not self.sequential and want_shard):
            return False
        bs = self._capture_bs()
        per_rank = [sum(all_sizes.get(n, 0) for n in names if owner[n] == r) for r in range(world)]
        during = sum(all_sizes.values()) / world          # every rank holds all modules x its share of sub-batches
        shard_budget = self.cache_budget_bytes if self.cache_budget_bytes is not None else (200 << 30)   # NOT the locally
        # (pieces of all modules + the send buffer, then the receive buffer + the reassembled tensors of the own modules)
        return (n_sub >= world and 2 * max(per_rank) + 2 * during <= shard_budget                         # measured one
                and all(inp.shape[0] % bs == 0 for inp, _ in self.calib_loader))

    def _plan(self, cal, todo, budget):
        sizes = None
        if not (self.sequential or cal.shard_cap):
            sizes = cal.all_sizes if cal.all_sizes is not None else self._estimate_cache_bytes(todo)
        return plan_groups(todo, sizes, budget, self.sequential, cal.shard_cap)

    def _run_group(self, cal, grp):
        """Capture and search of one group of modules; returns the seconds of either."""
        opts = cal.opts
        t1 = time.time()
        # (the grouped search is one call however many streams the per-module search would use: search_streams = 1 selects ONE
        # group call)
        concurrent = (cal.batching and not self.sequential and (opts.search_streams > 1 or opts.search_grouped)
                      and _dev_of(self.net).type == "cuda" and len(grp) > 1)
        # The search streams wait for the capture ON THE DEVICE (wait_stream): the host does not -- its threads prepare and
        # enqueue the first searches while the last capture passes still run (a host synchronisation here left the GPU idle
        # for ~2 ms per calibration: thread start, descriptors, workspace planning).  The capture / search split of the
        # timings then comes from a device event instead of the host clock.
        cap_done = None
        if cal.shard_cap:
            self._capture(cal.names, cal.raw_pred_softmax, cal.with_grad, stride=(cal.rank, cal.world), opts=opts)
            grad_names = {n for n in cal.names if cal.with_grad and hasattr(self.wrapped_modules[n], "metric")}
            shard.exchange_captures(self.wrapped_modules, cal.owner, cal.n_sub, grad_names)
        else:
            self._capture(grp, cal.raw_pred_softmax, cal.with_grad, opts=opts)
        if concurrent and not cal.shard_cap:
            cap_done = torch.cuda.Event(enable_timing=True)
            cap_done.record(torch.cuda.current_stream(_dev_of(self.net)))
        elif torch.cuda.is_available():
            torch.cuda.synchronize()
        t2 = time.time()
        if not concurrent:
            self._search_serial(cal, grp)
        elif opts.search_grouped:
            calls = opts.n_group_calls(lambda: sum(self._estimate_cache_bytes(grp).values()))
            self._search_grouped(grp, calls, inputs_ready=cap_done, opts=opts)
        else:
            self._search_concurrent(grp, opts.search_streams)
        if cap_done is not None:            # (everything is synchronised now) when the capture really ended
            ref = torch.cuda.Event(enable_timing=True)
            ref.record(torch.cuda.current_stream(_dev_of(self.net)))
            ref.synchronize()
            t_end = time.time()
            t2 = max(t2, t_end - cap_done.elapsed_time(ref) * 1e-3)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        return t2 - t1, time.time() - t2

    def _search_serial(self, cal, grp):
        """The reference's loop (quant_calib.py:371-372): one module after the other on the current stream."""
        for n in tqdm(grp, desc="Hessian"):
            module = self.wrapped_modules[n]
            with torch.no_grad():
                if cal.batching:
                    module.calibration_step2()
                elif isinstance(module, MinMaxQuantMatMul):
                    module.calibration_step2(module.raw_input[0], module.raw_input[1])
                else:
                    module.calibration_step2(module.raw_input)
            module.mode = "quant_forward" if self.sequential else "raw"

    def _replan_after_oom(self, cal, oom, grp, groups, done, budget):
        """The budget was an estimate (allocator fragmentation, another tenant on the GPU): drop this group's caches and scratch,
        halve the budget and re-plan what is not calibrated yet; returns (groups, budget).  (Not possible mid-collective.)"""
        if cal.opts.capture_trace:
            import traceback
            tb = traceback.extract_tb(oom.__traceback__)
            print("[ptq4vit_amd] OOM at " + " <- ".join(f"{os.path.basename(f.filename)}:{f.lineno}({f.name})" for f in tb[-4:]) + ": " + str(oom).split("\n")[0][:200], flush=True)
        if cal.shard_cap or len(grp) <= 1:      # a single module that does not fit cannot be split any further
            raise oom
        from .. import engine
        for n in grp:
            if n not in done and not _calibrated_and_freed(self.wrapped_modules[n]):
                forget_caches(self.wrapped_modules[n])
        engine.release_workspace()
        torch.cuda.empty_cache()
        budget //= 2
        print(f"[ptq4vit_amd] out of memory with {len(grp)} modules resident: retrying with a cache budget of {budget >> 30} GiB")
        left = [n for n in grp if not _calibrated_and_freed(self.wrapped_modules[n])]
        left += [n for g in groups for n in g]
        return self._plan(cal, left, budget), budget

    def _exchange(self, cal):
        """Intervals to every rank, and every module's search time of this calibration (of this world size) with the network: the
        next calibration's LPT order and owner costs.  Returns the seconds of the interval exchange."""
        t_ex = 0.0
        mine_ms = dict(getattr(self, "_module_ms", {}))
        if cal.world > 1 and not self.sequential:
            t1 = time.time()
            shard.exchange_intervals(self.wrapped_modules, cal.owner)
            t_ex = time.time() - t1          # includes waiting for the slowest rank's search (the collective is the barrier)
            parts = [None] * cal.world
            shard.dist.all_gather_object(parts, mine_ms)                 # a few hundred floats: next calibration's LPT costs
            mine_ms = {k: v for part in parts for k, v in (part or {}).items()}
        if mine_ms:          # replaced, not merged: the table describes ONE calibration (of this world size), gathered from all ranks
            self.net.__dict__["_p4v_module_ms"] = {"world": cal.world, "ms": dict(mine_ms)}
        return t_ex
