"""GPU: the stream contract of the C ABI (include/ptq4vit_hip.h, Conventions) through every public entry point of
ptq4vit_amd/engine.py -- "all work is enqueued on `stream`", "*_quant_forward, p4v_quantize_i8 and p4v_fake_quant never
synchronise", "safe to call concurrently on different devices / streams".

The parity suite calls the engine on the null stream, where csrc/p4v_api.hip's host_mirror() has no mapped block and every
interval and survivor read-back is a copy; a calibration runs on named side streams, in three threads, and reads through the
mapped-host mirror (IvMirror g_mir[], attach_mirror, read_dev, the (device, stream) table).  Here the two paths are held equal:

 1  every entry point on a named stream gives, bit for bit, what it gives on the null stream (the call the parity suite holds to
    the oracle) -- and, for the calibrations, launches the same kernels and stages the same passes;
 2  every launch is on the caller's stream: inputs that only become valid on the stream behind a delay, outputs copied on the
    stream right behind the call, no host synchronisation in between (tests/stream_cases.py, Probe, "ordered"); the entry points
    the header promises it for return while the stream is still busy;
 3  p4v_calibrate_group's `inputs_ready` event: captured tensors produced on another stream;
 4  concurrent callers: threads x streams, one thread alternating streams, one stream handed from thread to thread, group calls
    in three threads.

Reference everywhere: the null-stream result.  Every comparison is of bytes.

The delay in front of an ordered call is D = max(50 ms, 20 x the host time the call took on the named stream in 1): a launch on
a wrong stream has the whole delay to read the NaN inputs.  Twenty is arbitrary; a loaded machine lengthens the delay, not the
race.  $P4V_STREAMS_OUT: a JSON file of the host times, delays and counts (profiles/r32_stream_contract.json)."""
import contextlib
import json
import os
import threading

import pytest
import torch

from tests import stream_cases as sc
from tests.stream_cases import BY_ID, ENTRIES, Probe

pytestmark = pytest.mark.gpu

IDS = [e.id for e in ENTRIES]
LOOSE = sc.LOOSE
_REF, _NAMED, _PROFILE = {}, {}, {}


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    yield engine
    engine.release_workspace()


class Ctx:
    def __init__(self, eng):
        self.dev = torch.device("cuda", torch.cuda.current_device())
        # four streams, the first one of the calibrator's own persistent side streams
        self.streams = [eng.side_streams(self.dev, 3)[0]] + [torch.cuda.Stream() for _ in range(3)]
        self.delay = sc.Delay(self.dev)


@pytest.fixture(scope="module")
def ctx(eng):
    c = Ctx(eng)
    yield c
    torch.cuda.synchronize()
    path = os.environ.get("P4V_STREAMS_OUT")
    if path and _PROFILE:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump({"ms_per_delay_gemm": c.delay.ms_per_gemm, "delay_rule": "max(50 ms, 20 x host_ms)",
                       "entries": {k: _PROFILE[k] for k in sorted(_PROFILE)}}, fh, indent=1)


def _run(eng, entry, stream, stats=False, probe=None):
    """one plain call of `entry` on `stream` (None: the null stream): its results on the host, the host time of its ABI calls,
    with `stats` the kernels it launched, the prune counters and the pass memo's (hits, misses)"""
    probe = probe or Probe(eng)
    torch.cuda.synchronize()
    if stats:
        eng.launch_counters(reset=True)
        eng.prune_counters(reset=True)
        eng.stats_reset()
        eng.stats_enable(True)
    try:
        with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()), torch.no_grad():
            assert (torch.cuda.current_stream().cuda_stream == 0) == (stream is None)
            res = entry.call(probe)
        torch.cuda.synchronize()
        out = dict(res=sc.to_host(res), host_ms=probe.host_ms)
        if stats:
            st = eng.stats_get()
            recs = eng.stats_launches()
            out.update(kernels=[(r["kernel"], r["stage"]) for r in recs], grids=[(r["grid_x"], r["grid_z"]) for r in recs],
                       prune=eng.prune_counters(), memo=(int(st["memo_hits"]), int(st["memo_misses"])))
    finally:
        if stats:
            eng.stats_enable(False)
    return out


def reference(eng, entry):
    if entry.id not in _REF:
        _REF[entry.id] = _run(eng, entry, None, stats=entry.calibration)
    return _REF[entry.id]


def named(eng, ctx, entry):
    """on the first named stream: once as it is (results, host time), the calibrations once more with launch records"""
    if entry.id not in _NAMED:
        r = _run(eng, entry, ctx.streams[0])
        if entry.calibration:
            r["stats"] = _run(eng, entry, ctx.streams[0], stats=True)
        _NAMED[entry.id] = r
    return _NAMED[entry.id]


def _same(got, want, what):
    assert len(got) == len(want) and len(want) > 0, f"{what}: {len(got)} result tensors, the null stream gave {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[:2] == w[:2], f"{what}: result {i} is {g[:2]}, on the null stream {w[:2]}"
        if g[2] != w[2]:
            n = sum(a != b for a, b in zip(g[2], w[2]))
            raise AssertionError(f"{what}: result {i} {w[:2]} differs from the null stream's in {n} of {len(w[2])} bytes")
    return len(want)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", IDS)
def test_named_stream_equals_null_stream(eng, ctx, id):
    entry = BY_ID[id]
    ref, nm = reference(eng, entry), named(eng, ctx, entry)
    n = _same(nm["res"], ref["res"], f"{id} on a named stream")
    if not entry.calibration:
        print(f"[streams] {id}: {n} tensors bit-identical; host {nm['host_ms']:.3f} ms")
        return
    st = nm["stats"]
    _same(st["res"], ref["res"], f"{id} on a named stream, launch timing on")
    print(f"[streams] {id}: {n} tensors bit-identical; host {nm['host_ms']:.3f} ms; {len(ref['kernels'])} sweep launches; prune {ref['prune']}; "
          f"memo {ref['memo']}; grids equal: {st['grids'] == ref['grids']}")
    # the path does not change which kernels run, nor what the pruning decides
    assert st["kernels"] == ref["kernels"], (id, [(i, a, b) for i, (a, b) in enumerate(zip(st["kernels"], ref["kernels"])) if a != b][:4],
                                             len(st["kernels"]), len(ref["kernels"]))
    assert st["prune"] == ref["prune"], (id, st["prune"], ref["prune"])
    assert st["memo"] == ref["memo"], (id, st["memo"], ref["memo"])
    for r in (ref, st):
        p = r["prune"]
        if entry.prune == "staged":
            assert p["staged"] > 0, (id, p)
        elif entry.prune == "kept":
            assert p["staged"] == 0 and p["kept_full_sweep"] > 0, (id, p)
        elif entry.prune == "never":
            assert p["staged"] == 0 and p["kept_full_sweep"] == 0 and p["not_eligible"] > 0, (id, p)
        if id.endswith(f"{sc.TWIN}-memo"):
            assert r["memo"][0] > 0, f"{id}: the case is here for its pass-memo hits, got (hits, misses) = {r['memo']}"


def test_group_call_on_a_named_stream_equals_the_null_stream(eng, ctx):
    """six members of tests/test_hip_group.py's mixture: every member has a mirror of its own on either stream"""
    from tests.test_hip_group import _jobs, _mixture
    specs = _mixture(eng)[:6]
    torch.cuda.synchronize()
    ref = sc.to_host([j.outputs for j in eng.calibrate_group(_jobs(eng, specs))])
    torch.cuda.synchronize()
    with torch.cuda.stream(ctx.streams[0]):
        got = [j.outputs for j in eng.calibrate_group(_jobs(eng, specs))]
    torch.cuda.synchronize()
    _same(sc.to_host(got), ref, "calibrate_group of six Linear layers on a named stream")


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def _ordered(eng, ctx, entry):
    ref, nm = reference(eng, entry), named(eng, ctx, entry)
    s = ctx.streams[0]
    D = max(50.0, 20.0 * nm["host_ms"])
    probe = Probe(eng, stream=s, delay=ctx.delay, delay_ms=D)
    with torch.cuda.stream(s), torch.no_grad():
        res = entry.call(probe)
    s.synchronize()
    got = sc.to_host(res)
    torch.cuda.synchronize()
    n = _same(got, ref["res"], f"{entry.id} behind {D:.0f} ms of work on its stream, inputs NaN until then")
    assert probe.calls >= 1 and len(probe.busy) == probe.calls
    busy = 0
    if entry.never_syncs:
        for i, b in enumerate(probe.busy):
            assert b, f"{entry.id}: call {i} returned with its stream idle behind {D:.0f} ms of work: it waited for the stream"
            busy += 1
        assert busy == probe.calls == 1
    _PROFILE[entry.id] = dict(host_ms=round(nm["host_ms"], 4), delay_ms=round(D, 3), outputs_compared=n, abi_calls=probe.calls,
                              busy_asserts=busy, returned_busy=sum(probe.busy))
    print(f"[streams] {entry.id}: host {nm['host_ms']:.3f} ms, delay {D:.0f} ms, {n} tensors, returned busy {sum(probe.busy)}/{probe.calls}")
    return busy


@pytest.mark.parametrize("id", IDS)
def test_everything_is_enqueued_on_the_callers_stream(eng, ctx, id):
    _ordered(eng, ctx, BY_ID[id])


def test_every_never_synchronise_assert_ran(eng, ctx):
    """the entry points the header promises "never synchronises" for (and p4v_pack_plane_i8, p4v_export_quantize): each returned
    while its stream was busy, and none was left out"""
    want = [e for e in ENTRIES if e.never_syncs]
    ran = sum(_PROFILE[e.id]["busy_asserts"] if e.id in _PROFILE else _ordered(eng, ctx, e) for e in want)
    assert ran == len(want) == 11, (ran, len(want))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fired", [False, True], ids=["event_behind_the_producer", "event_already_fired"])
def test_group_waits_for_inputs_ready_where_it_reads_a_captured_tensor(eng, ctx, fired):
    """Three Linear jobs and a MatMul job on stream s; their captured tensors are produced on stream p behind a delay, the event
    recorded behind the producer copies.  s never waits for p in Python.  `fired`: the event recorded on an idle p, the data ready."""
    entry = BY_ID["calibrate_group-3_linear_1_matmul"]
    ref, nm = reference(eng, entry), named(eng, ctx, entry)
    D = max(50.0, 20.0 * nm["host_ms"])
    s, p = ctx.streams[1], ctx.streams[2]
    pairs, jobs = [], []
    for kind, kw in sc._small_group_specs():
        kw = dict(kw)
        for k in sc.CAPTURED[kind]:
            buf = sc._nan_like(kw[k])
            pairs.append((buf, kw[k]))
            kw[k] = buf
        jobs.append(getattr(eng, kind + "_job")(**kw))
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    if fired:
        for buf, real in pairs:
            buf.copy_(real)
        torch.cuda.synchronize()
        ev.record(p)
        ctx.delay(p, D)
    else:
        ctx.delay(p, D)
        with torch.cuda.stream(p):
            for buf, real in pairs:
                buf.copy_(real)
        ev.record(p)
    with torch.cuda.stream(s), torch.no_grad():
        eng.calibrate_group(jobs, inputs_ready=ev)
        got = sc._clone([j.outputs for j in jobs])
    s.synchronize()
    got = sc.to_host(got)
    torch.cuda.synchronize()
    _same(got, ref["res"], f"calibrate_group(inputs_ready), producer behind {D:.0f} ms on another stream")


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
ROTATION = ["linear_job+run_job-lin650_cls-memo", f"linear_job+run_job-{sc.TWIN}-memo", "matmul_job+run_job-qk65-memo",
            "matmul_job+run_job-sos65-memo", "conv_job+run_job-conv640_a8-memo", "linear_job+run_job-lin650_nV33-memo", "mlp_quant_forward"]


def _threads(n, work):
    """`work(i)` in n threads held at a barrier before their first call; what they raise is raised here"""
    barrier, errors = threading.Barrier(n), []

    def body(i):
        try:
            work(i, barrier)
        except BaseException as e:      # noqa: BLE001
            barrier.abort()
            errors.append((i, e))
    ts = [threading.Thread(target=body, args=(i,)) for i in range(n)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errors:
        raise AssertionError(f"thread {errors[0][0]} of {n} ({len(errors)} failed): {errors[0][1]!r}") from errors[0][1]


def test_three_threads_on_three_streams(eng, ctx):
    """A rotation of seven jobs, thread i starting at job i, twice round.  The cases' process-wide A/B words (the forced pruning) are
    set once for the whole test -- references included -- and the cases' own writes to them are switched off."""
    jobs = [BY_ID[i] for i in ROTATION]
    eng.debug_variant(LOOSE)
    try:
        refs = [_run(eng, e, None, probe=Probe(eng, freeze_debug=True))["res"] for e in jobs]
        got = [[] for _ in range(3)]

        def work(i, barrier):
            s = ctx.streams[i]
            with torch.cuda.stream(s), torch.no_grad():
                probe = Probe(eng, freeze_debug=True)
                barrier.wait(timeout=120)
                for k in range(2 * len(jobs)):
                    j = (i + k) % len(jobs)
                    res = jobs[j].call(probe)
                    s.synchronize()
                    got[i].append((j, sc.to_host(res)))
        _threads(3, work)
        torch.cuda.synchronize()
    finally:
        eng.debug_variant(0)
    for i in range(3):
        assert [j for j, _ in got[i]] == [(i + k) % len(jobs) for k in range(2 * len(jobs))]
        for k, (j, res) in enumerate(got[i]):
            _same(res, refs[j], f"thread {i}, call {k} ({jobs[j].id}) next to two other threads")


def test_one_thread_alternating_two_streams(eng, ctx):
    """call by call s0, s1, s0, ...: a Linear on s0, a MatMul on s1, then the granular calls of a Linear on s0 and of a MatMul on s1
    in turn, then the two fused calls again -- the thread's mirror slots are bound to other vectors and another block every call"""
    s0, s1 = ctx.streams[0], ctx.streams[1]
    lin, mm = BY_ID["linear_job+run_job-lin650_cls-memo"], BY_ID["matmul_job+run_job-qk65-memo"]
    lin_steps, mm_steps = BY_ID["LinearStepper-linear_steps"], BY_ID["MatMulStepper-qk_steps"]
    want = {e.id: reference(eng, e)["res"] for e in (lin, mm, lin_steps, mm_steps)}
    torch.cuda.synchronize()
    probe, got = Probe(eng), []
    with torch.no_grad():
        for rnd in range(2):
            with torch.cuda.stream(s0):
                got.append((lin.id, lin.call(probe)))
            with torch.cuda.stream(s1):
                got.append((mm.id, mm.call(probe)))
            gens = [(lin_steps.id, sc.linear_steps_gen(probe), s0), (mm_steps.id, sc.qk_steps_gen(probe), s1)]
            while gens:
                for item in list(gens):
                    name, gen, s = item
                    with torch.cuda.stream(s):
                        try:
                            next(gen)
                        except StopIteration as e:
                            got.append((name, e.value))
                            gens.remove(item)
    torch.cuda.synchronize()
    assert len(got) == 8
    for k, (name, res) in enumerate(got):
        _same(sc.to_host(res), want[name], f"call {k} ({name}) of one thread alternating two streams")


def test_one_stream_handed_from_thread_to_thread(eng, ctx):
    """three threads one after the other on the same stream: the (device, stream) table of mirror blocks read from other threads"""
    s = ctx.streams[3]
    jobs = [BY_ID["linear_job+run_job-lin650_cls-memo"], BY_ID["matmul_job+run_job-sos65-memo"], BY_ID["ConvStepper-conv_steps"]]
    want = [reference(eng, e)["res"] for e in jobs]
    torch.cuda.synchronize()
    for t in range(3):
        got = []

        def work(_i, _barrier):
            with torch.cuda.stream(s), torch.no_grad():
                probe = Probe(eng)
                for e in jobs:
                    res = e.call(probe)
                    s.synchronize()
                    got.append(sc.to_host(res))
        _threads(1, work)
        assert len(got) == len(jobs)
        for e, res, w in zip(jobs, got, want):
            _same(res, w, f"{e.id} in thread {t} of three using one stream in turn")


def test_group_calls_in_three_threads_on_three_streams(eng, ctx):
    """the calibrator's own pattern (utils/quant_calib.py, _on_side_streams): three p4v_calibrate_group calls at a time, four
    members of tests/test_hip_group.py's mixture each"""
    from tests.test_hip_group import _jobs, _mixture
    specs = _mixture(eng)
    parts = [specs[4 * i:4 * i + 4] for i in range(3)]
    assert all(len(p) == 4 for p in parts)
    torch.cuda.synchronize()
    refs = []
    for p in parts:
        refs.append(sc.to_host([j.outputs for j in eng.calibrate_group(_jobs(eng, p))]))
        torch.cuda.synchronize()
    eng.launch_counters(reset=True)
    got = [None] * 3

    def work(i, barrier):
        s = ctx.streams[i]
        with torch.cuda.stream(s), torch.no_grad():
            jobs = _jobs(eng, parts[i])
            barrier.wait(timeout=120)
            eng.calibrate_group(jobs)
            s.synchronize()
            got[i] = sc.to_host([j.outputs for j in jobs])
    _threads(3, work)
    torch.cuda.synchronize()
    cnt = eng.launch_counters(reset=True)
    assert cnt["groups"] == 3, cnt
    for i in range(3):
        _same(got[i], refs[i], f"group call {i} of three concurrent ones")


# ---- the list of entry points ---------------------------------------------------------------------------------------------------------
# public functions and classes of engine.py that take tensors and make an ABI call: each is in the `api` of an entry above
COVERED = {"run_job", "calibrate_group", "linear_job", "matmul_job", "conv_job", "linear_calibrate", "matmul_calibrate", "conv_calibrate",
           "LinearStepper", "MatMulStepper", "ConvStepper", "linear_quant_forward", "matmul_quant_forward", "matmul_blocks_quant_forward",
           "mlp_quant_forward", "attn_quant_forward", "window_attn_quant_forward", "qkv_attn_quant_forward", "quantize_i8", "pack_plane_i8",
           "fake_quant", "export_quantize", "score_argmax_gather", "multi_copy"}
# the debug_* entry points (tests and tools only), launch timing and counters
EXCLUDED = {"debug_variant", "debug_tuning", "debug_arena_gap", "debug_arena_ranges", "debug_bound_totals", "debug_prune_tables",
            "debug_prune_decide", "debug_topk_rows", "debug_pack_dual", "debug_pack_cands", "debug_gather_im2col", "debug_prep_epi6",
            "debug_sos_sweep", "stats_enable", "stats_reset", "stats_get", "stats_launches", "launch_counters", "prune_counters"}
# no ABI call on tensors: torch-side helpers and the record of a prepared call
NO_ABI = {"device_of", "to_dev", "workspace", "release_workspace", "workspace_bytes", "workspace_held", "side_streams",
          "candidate_multipliers", "ptr", "stream_ptr", "metric_id", "has_blocks", "Job"}


@pytest.mark.parametrize("id", ["engine_entry_points"])
def test_every_public_entry_point_has_a_stream_test(eng, id):
    public = {n for n, v in vars(eng).items() if not n.startswith("_") and callable(v) and getattr(v, "__module__", None) == eng.__name__}
    assert not (COVERED & EXCLUDED) and not (COVERED & NO_ABI) and not (EXCLUDED & NO_ABI)
    assert all(n.startswith(("debug_", "stats_")) or n.endswith("_counters") for n in EXCLUDED)
    assert public - EXCLUDED - NO_ABI == COVERED, (sorted(public - EXCLUDED - NO_ABI - COVERED), sorted(COVERED - public))
    assert (EXCLUDED | NO_ABI) <= public, sorted((EXCLUDED | NO_ABI) - public)
    # ... and the ids of the parametrised tests name them
    for name in COVERED:
        assert any(name in e.api and name in e.id for e in ENTRIES), f"{name}: no entry of tests/stream_cases.py goes through it by name"
    # every Probe wrapper stands for an entry point of the list
    assert set(sc.SINGLE) | set(sc.JOBS) | set(sc.STEPPERS) <= COVERED
