"""A guarded, exact, poisoned workspace for the tests of the caller-workspace contract (include/ptq4vit_hip.h, Conventions).

`Guard` replaces `ptq4vit_amd.engine.workspace` (and wraps `calibrate_group` and the steppers' call helpers, which use a workspace
taken earlier) for the duration of a test.  The replacement keeps the signature `(dev, nbytes, slot=0)` and the keying by (device,
current stream, slot) and returns a uint8 view with

  exact size   numel() == nbytes: no 5 %, no 1 MiB, none of the arena's 1 MiB -- the engine passes `ws.numel()` as workspace_bytes
  guards       one zone in front of the view and one behind it, inside ONE allocation, each >= int(nbytes * 0.05) + 1 MiB (the pad
               engine.workspace adds in production): what that pad has been absorbing lands in a guard, not in foreign memory
  alignment    the view starts at an ODD multiple of WS_ALIGN, the minimum the header documents: no more alignment than a
               conforming C caller must give
  poison       before EVERY engine call (the contract: content on entry is arbitrary, for every call, the granular ones included)
               the guards are filled with GUARD_BYTE and the view with `poison`

After a call (at the next use of the buffer, or in `finish()`), behind a synchronisation, the check compares on the device:
  guard bytes that changed (must be none); the highest touched offset of the view = last byte that differs from the poison + 1
  (a lower bound: a kernel that stores the poison's own value is not seen; the tests run two poisons); for an arena slot the
  bytes that changed in the slack between offs[i] + need_i and offs[i + 1] (the carving of engine.calibrate_group, learnt by
  wrapping it); with the arena gap on (p4v_debug_set_arena_gap) the bytes that changed outside p4v_debug_arena_ranges.
"""
import threading

import torch

WS_ALIGN = 16            # include/ptq4vit_hip.h: minimum alignment of d_workspace
GUARD_BYTE = 0xA5
CHUNK = 1 << 20


def guard_bytes(nbytes):
    return int(nbytes * 0.05) + (1 << 20)


def _count_changed(t, value):
    return int((t != value).sum()) if t.numel() else 0


def _touched(view, poison):
    """last byte of `view` that differs from `poison`, + 1 (0: none)"""
    n = view.numel()
    full = n // CHUNK * CHUNK
    if n > full:
        nz = (view[full:] != poison).nonzero()
        if nz.numel():
            return full + int(nz[-1]) + 1
    if full:
        hit = (view[:full].view(-1, CHUNK) != poison).any(1).nonzero()
        if hit.numel():
            c = int(hit[-1])
            nz = (view[c * CHUNK:(c + 1) * CHUNK] != poison).nonzero()
            return c * CHUNK + int(nz[-1]) + 1
    return 0


class _Buf:
    __slots__ = ("alloc", "front", "nbytes", "declared", "slot", "pending", "carve", "group", "virgin", "stream")

    def view(self):
        return self.alloc[self.front:self.front + self.declared]

    def full(self):
        return self.alloc[self.front:self.front + self.nbytes]


class Guard:
    """with Guard(engine, monkeypatch, poison) as g: ... engine calls ...; reports = g.finish()

    `declare`: maps the size asked for to the size the engine is TOLD (the view's numel); the allocation behind the view always holds
    the full size plus the guards -- for the tests of a declared size that is too small.
    `gap`: the arena gap is on (set by the caller BEFORE the jobs are built): every check also reads p4v_debug_arena_ranges."""

    def __init__(self, eng, monkeypatch, poison, *, gap=0, declare=None):
        self.eng, self.mp, self.poison, self.gap, self.declare = eng, monkeypatch, int(poison), int(gap), declare
        self.bufs, self.reports, self.lock = {}, [], threading.Lock()

    # ---- the replacement of engine.workspace ------------------------------------------------------------------------------------
    def workspace(self, dev, nbytes, slot=0):
        nbytes = int(nbytes)
        key = (dev, torch.cuda.current_stream(dev).cuda_stream, slot)
        with self.lock:
            b = self.bufs.get(key)
        if b is not None:
            self._check(b)
        if b is None or b.nbytes != nbytes:
            with self.lock:
                self.bufs.pop(key, None)
            b = None
            g = guard_bytes(nbytes)
            nb = _Buf()
            nb.alloc = torch.empty(g + 2 * WS_ALIGN + nbytes + g, dtype=torch.uint8, device=dev)
            base = nb.alloc.data_ptr()
            front = g
            while (base + front) % (2 * WS_ALIGN) != WS_ALIGN:          # an odd multiple of the minimum alignment
                front += 1
            nb.front, nb.nbytes, nb.slot, nb.pending, nb.carve, nb.group, nb.stream = front, nbytes, slot, False, None, False, key[1]
            b = nb
            with self.lock:
                self.bufs[key] = b
        self._one_call_at_a_time(b)
        b.declared = nbytes if self.declare is None else int(self.declare(nbytes))
        assert 0 <= b.declared <= b.nbytes
        self._poison(b)
        b.virgin = True                      # handed out, no call yet (a stepper takes its workspace before its first call)
        v = b.view()
        assert v.numel() == b.declared and v.data_ptr() % WS_ALIGN == 0 and (v.data_ptr() // WS_ALIGN) % 2 == 1
        assert b.front >= guard_bytes(nbytes) and b.alloc.numel() - b.front - b.nbytes >= guard_bytes(nbytes)
        return v

    def _poison(self, b):
        b.alloc[:b.front].fill_(GUARD_BYTE)
        b.alloc[b.front + b.nbytes:].fill_(GUARD_BYTE)
        b.full().fill_(self.poison)
        b.pending = True

    def _one_call_at_a_time(self, b):
        """With the gap on a check reads p4v_debug_arena_ranges, the ranges of the calling thread's LAST call: a call on `b` while
        another buffer still has an unchecked call behind it would have that buffer checked against the wrong ranges."""
        if not self.gap:
            return
        with self.lock:
            others = [o for o in self.bufs.values() if o is not b and o.pending and not o.group]
        assert not others, "arena gap on: a second buffer is used before the first call's ranges were checked (call finish() in between)"

    def _find(self, ws):
        with self.lock:
            for b in self.bufs.values():
                if b.alloc.data_ptr() + b.front == ws.data_ptr():
                    return b
        raise AssertionError("an engine call used a workspace the guard did not hand out")

    # ---- the check --------------------------------------------------------------------------------------------------------------
    def _check(self, b):
        if not b.pending:
            return
        b.pending = False
        torch.cuda.current_stream(b.alloc.device).synchronize()
        rep = dict(slot=str(b.slot), stream=b.stream, need=b.nbytes, declared=b.declared, poison=self.poison)
        rep["guard_changed"] = (_count_changed(b.alloc[:b.front], GUARD_BYTE) +
                                _count_changed(b.alloc[b.front + b.nbytes:], GUARD_BYTE))
        full = b.full()
        rep["touched"] = _touched(full, self.poison)
        if b.carve is not None:                     # an arena: the slack behind every member's exact need
            bad, slack = 0, 0
            ends = [o for o, _ in b.carve[1:]] + [b.nbytes]
            for (off, need), end in zip(b.carve, ends):
                bad += _count_changed(full[off + need:end], self.poison)
                slack += end - off - need
            rep["slack_bytes"], rep["slack_changed"] = slack, bad
            b.carve = None
        if self.gap and not b.group:
            ranges = self.eng.debug_arena_ranges()
            bad, free, at = 0, 0, 0
            for lo, hi in ranges + [(b.nbytes, b.nbytes)]:
                assert at <= lo <= hi <= b.nbytes, (ranges, b.nbytes)
                bad += _count_changed(full[at:lo], self.poison)
                free += lo - at
                at = hi
            rep["ranges"], rep["unalloc_bytes"], rep["unalloc_changed"] = len(ranges), free, bad
        with self.lock:
            self.reports.append(rep)

    def finish(self):
        """Check every buffer that has an unchecked call behind it; returns all reports of this guard so far."""
        torch.cuda.synchronize()
        with self.lock:
            bufs = list(self.bufs.values())
        for b in bufs:
            self._check(b)
        return list(self.reports)

    # ---- installation -----------------------------------------------------------------------------------------------------------
    def __enter__(self):
        eng, guard = self.eng, self
        eng.release_workspace()
        self._ctx = self.mp.context()              # undone in __exit__: the next guard wraps the engine's own functions again
        mp = self._ctx.__enter__()
        mp.setattr(eng, "workspace", self.workspace)
        orig_group = eng.calibrate_group

        def calibrate_group(jobs, inputs_ready=None):
            jobs = list(jobs)
            if not jobs:
                return orig_group(jobs, inputs_ready=inputs_ready)
            carve, total = [], 0
            for job in jobs:                       # the carving of engine.calibrate_group
                carve.append((total, int(job.need)))
                total += (int(job.need) + 4095) & ~4095
            out = orig_group(jobs, inputs_ready=inputs_ready)      # (takes workspace(dev, total, slot="arena"): poisoned there)
            key = (jobs[0].dev, torch.cuda.current_stream(jobs[0].dev).cuda_stream, "arena")
            with guard.lock:
                b = guard.bufs[key]
            assert b.nbytes == total, (b.nbytes, total)
            b.carve, b.group = carve, True
            return out

        mp.setattr(eng, "calibrate_group", calibrate_group)

        def wrap(cls, name):
            orig = getattr(cls, name)

            def call(st, *args, **kw):
                b = guard._find(st.ws)
                guard._one_call_at_a_time(b)
                if b.virgin:
                    b.virgin = b.pending = False
                guard._check(b)                    # the previous call of the sequence
                guard._poison(b)                   # arbitrary content on entry of EVERY granular call
                return orig(st, *args, **kw)
            mp.setattr(cls, name, call)

        wrap(eng._Stepper, "_call")
        wrap(eng.MatMulStepper, "_call_blocks")
        return self

    def __exit__(self, *exc):
        self._ctx.__exit__(*exc)
        self.bufs.clear()
        self.eng.release_workspace()
        return False


def summarise(reports):
    """One row of profiles/r17_workspace_contract.json from the reports of one guarded run."""
    out = dict(calls=len(reports), need=max((r["need"] for r in reports), default=0),
               touched=max((r["touched"] for r in reports), default=0),
               guard_changed=sum(r["guard_changed"] for r in reports),
               slack_changed=sum(r.get("slack_changed", 0) for r in reports),
               unalloc_changed=sum(r.get("unalloc_changed", 0) for r in reports))
    shares = [r["unalloc_bytes"] / r["need"] for r in reports if "unalloc_bytes" in r and r["touched"] > 0]
    if shares:
        out["unalloc_share_min"] = min(shares)
    return out
