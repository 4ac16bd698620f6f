"""The gated run: where an entry queues its work, tested on the device (a plain helper module like kernel_guards; the self-checks of
test_gpu_stream_contract.py prove in every session that it reports each fault it is for).

include/omnivggt_hip.h promises for every entry: never allocates or frees, never synchronises the device, the work goes to the caller's
stream. One protocol checks all of it:

  setup, default stream     real inputs -> the entry into guarded outputs / workspaces -> `want` (bytes); decoy inputs (same shapes and dtypes,
                            valid data of the same kind) -> the entry again -> must differ from `want` in bytes; synchronize. The tensors the
                            entry reads ("live") now hold the decoys, outputs and workspaces the decoy run's leftovers.
  gated section, stream S   blocker (torch.cuda._sleep), event ev, then per case: refill every output / workspace buffer with GUARD_BYTE,
                            live.copy_(real), the entry call on S; `early = not ev.query()` directly after the call returns.
  afterwards                S.synchronize(), guard checks, output bytes == want.

A stage queued on any other stream runs while S is still blocked: on decoys, or on workspace that is refilled later -> the bytes differ.
A call that synchronises or copies synchronously returns after the blocker -> early is False. torch.cuda.memory_stats() across the call
shows an allocation or a free of the caching allocator (so the Python wrappers are held to "never allocates" with every buffer supplied,
and a hipMalloc behind torch.empty cannot be what spoils `early`).

Case builders describe one call:
    c = Case("layernorm bf16")
    x = c.inp(torch.randn(257, 1024))            # live device tensor; real kept aside; decoy = rows reversed unless given
    y = c.out((257, 1024), torch.bfloat16)       # kernel_guards.guarded view
    c.call = lambda: ops.layernorm(x, ..., out=y)
ops.* read torch.cuda.current_stream(); the gated section runs under torch.cuda.stream(S), and every L.call is intercepted to record the
entry's name (coverage) and to assert that the handle it was given is S's.
"""
import contextlib
import gc
import time

import torch

import kernel_guards as kg
from omnivggt_official_amd import lib as L

DEV = "cuda"
MIN_BLOCK_MS = 100.0          # a condition, not a measurement: must dwarf the host cost of queueing one group of calls
BLOCK_OVER_CASE = 20.0        # and last at least this many times the longest default-stream duration of the group's cases
MAX_GROUP = 10


class ContractError(AssertionError):
    pass


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
def default_decoy(real):
    """Same shape / dtype / value set: the rows reversed (indices stay in range, counts stay what they were); a one-row tensor has its
    elements reversed. Builders pass their own decoy where the order of elements carries meaning (sorted tables, poses)."""
    if real.dim() and real.shape[0] > 1:
        d = real.flip(0)
        if not torch.equal(d, real):
            return d.contiguous()
    return real.flatten().flip(0).reshape(real.shape).contiguous()


class Case:
    def __init__(self, name):
        self.name = name
        self.live, self.real, self.decoy = [], [], []
        self.outs, self.checks, self.bufs = [], [], []
        self.consts = []                        # kept alive with the case: a raw parameter struct holds pointers, not references
        self.call = None
        self.entries = []                       # filled by the recorder: names of the entries the call reached
        self.want = None
        self.ms = 0.0

    def inp(self, real, decoy=None):
        """-> the live device tensor the call reads. `real` is copied (the builder's tensor is never written)."""
        real = real.to(DEV).contiguous().clone()
        decoy = default_decoy(real) if decoy is None else decoy.to(DEV).contiguous().clone()
        assert decoy.shape == real.shape and decoy.dtype == real.dtype, (self.name, decoy.shape, real.shape)
        live = real.clone()
        self.live.append(live)
        self.real.append(real)
        self.decoy.append(decoy)
        return live

    def const(self, t):
        """An input that is the same in both runs (weights, tables)."""
        t = t.to(DEV).contiguous().clone()
        self.consts.append(t)
        return t

    def out(self, shape, dtype, ld=None, compare=True):
        shape = tuple(int(s) for s in shape)
        flat = len(shape) < 2
        v, chk = kg.guarded((1,) + shape if flat else shape, dtype, DEV, ld=ld, guard_bytes=4096)
        if flat:
            v = v[0]
        self.checks.append(chk)
        self.bufs.append(chk.buffer)
        if compare:
            self.outs.append(v)
        return v

    def ws(self, nbytes):
        """A guarded workspace of exactly nbytes (uint8, 16-byte aligned); its content is not compared, its guard bands are checked."""
        return self.out((max(int(nbytes), 1),), torch.uint8, compare=False)

    def inout(self, real, decoy=None):
        """A tensor the entry reads and updates in place: restored from `real` before the gated call, compared afterwards."""
        live = self.inp(real, decoy)
        self.outs.append(live)
        return live

    # protocol steps
    def _load(self, which):
        for l, s in zip(self.live, which):
            l.copy_(s)

    def _refill(self):
        for b in self.bufs:
            b.fill_(kg.GUARD_BYTE)

    def _bytes(self):
        return [o.clone().contiguous().view(-1).view(torch.uint8).clone() for o in self.outs]

    def _check_guards(self, what):
        for i, c in enumerate(self.checks):
            c("%s: %s buffer %d" % (self.name, what, i))


@contextlib.contextmanager
def recorder(log, expect_stream=None):
    """Every L.call inside appends the entry's name to `log`; with expect_stream, a call that is handed another handle raises."""
    orig = L.call

    def call(name, params, stream):
        log.append(name)
        if expect_stream is not None and (stream or 0) != expect_stream:
            raise ContractError("%s was handed stream %r, the caller's is %r" % (name, stream, expect_stream))
        return orig(name, params, stream)
    L.call = call
    try:
        yield
    finally:
        L.call = orig


def _alloc_stats():
    s = torch.cuda.memory_stats()
    return (s.get("allocation.all.allocated", 0), s.get("allocation.all.freed", 0), s.get("segment.all.allocated", 0), s.get("segment.all.freed", 0))


# ---------------------------------------------------------------------------------------------
# the blocker and the side stream
# ---------------------------------------------------------------------------------------------
class Gate:
    """One per session: the calibrated blocker and the side stream the concurrency control settled on."""
    _instance = None

    def __init__(self):
        self.use_sleep = hasattr(torch.cuda, "_sleep")
        self._mm = None
        self.cycles, self.block_ms = self._calibrate(MIN_BLOCK_MS)
        self.stream, self.stream_index, self.concurrency_log = self._pick_stream()

    @classmethod
    def get(cls):
        if cls._instance is None:
            cls._instance = Gate()
        return cls._instance

    def block(self, scale=1):
        """Queue the blocker on the current stream."""
        if self.use_sleep:
            torch.cuda._sleep(int(self.cycles * scale))
        else:                                   # a chain of matmuls sized the same way
            for _ in range(int(self.cycles * scale)):
                torch.mm(self._mm, self._mm, out=self._mm2)

    def _time(self, cycles):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        if self.use_sleep:
            torch.cuda._sleep(int(cycles))
        else:
            for _ in range(int(cycles)):
                torch.mm(self._mm, self._mm, out=self._mm2)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def _calibrate(self, want_ms):
        if not self.use_sleep:
            self._mm = torch.zeros(1024, 1024, device=DEV)
            self._mm2 = torch.zeros(1024, 1024, device=DEV)
        cycles = 1 << 20 if self.use_sleep else 16
        self._time(cycles)                      # warm-up
        for _ in range(24):
            ms = self._time(cycles)
            if ms >= want_ms:
                print("blocker: %s(%d) lasts %.1f ms (wanted >= %.0f ms)" % ("torch.cuda._sleep" if self.use_sleep else "matmul chain", cycles, ms, want_ms), flush=True)
                return cycles, ms
            cycles *= 2
        raise ContractError("no blocker of %.0f ms within %d cycles" % (want_ms, cycles))

    def scale_for(self, longest_case_ms):
        """Integer factor on the calibrated blocker so that it lasts >= MIN_BLOCK_MS and >= BLOCK_OVER_CASE x the longest case."""
        need = max(MIN_BLOCK_MS, BLOCK_OVER_CASE * longest_case_ms)
        return max(1, int(-(-need // self.block_ms)))

    def concurrent(self, s):
        """Concurrency control: with the blocker running on `s`, a tiny torch copy on the default stream must complete before the
        blocker does. -> (ok, message)."""
        a, b = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
        ev, done = torch.cuda.Event(), torch.cuda.Event()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            self.block()
            ev.record(s)
        a.copy_(b)
        done.record()
        t0 = time.perf_counter()
        done.synchronize()
        waited = (time.perf_counter() - t0) * 1e3
        blocked = not ev.query()
        s.synchronize()
        return blocked, "copy on the default stream finished after %.2f ms, the blocker (%.0f ms) was %s" % (
            waited, self.block_ms, "still running" if blocked else "already over: the two streams share a queue")

    def _pick_stream(self):
        log = []
        for i in range(4):
            s = torch.cuda.Stream()
            ok, msg = self.concurrent(s)
            log.append("stream %d: %s" % (i, msg))
            print("concurrency control, " + log[-1], flush=True)
            if ok:
                return s, i, log
        return None, -1, log

    def require_stream(self):
        if self.stream is None:
            raise ContractError("no side stream runs concurrently with the default stream, the gated run cannot tell streams apart:\n  " +
                                "\n  ".join(self.concurrency_log))
        return self.stream


# ---------------------------------------------------------------------------------------------
# the protocol
# ---------------------------------------------------------------------------------------------
class Report:
    """What the gated run saw of one case; ok() raises ContractError listing every broken promise."""

    def __init__(self, case):
        self.case, self.name = case, case.name
        self.early, self.bytes_equal, self.allocated, self.freed, self.guard_error, self.mismatch = None, None, 0, 0, None, ""

    def faults(self, early=True, alloc=True):
        f = []
        if not self.bytes_equal:
            f.append("bytes: %s" % self.mismatch)
        if early and not self.early:
            f.append("early: the call returned only after the blocker had finished (it synchronised or copied synchronously)")
        if alloc and (self.allocated or self.freed):
            f.append("allocation: %d allocations and %d frees across the call" % (self.allocated, self.freed))
        if self.guard_error:
            f.append("guard: %s" % self.guard_error)
        return f

    def ok(self, early=True, alloc=True):
        f = self.faults(early, alloc)
        if f:
            raise ContractError("%s breaks the stream contract:\n  %s" % (self.name, "\n  ".join(f)))


def setup_case(c):
    """Default stream: real -> want, decoy -> must differ; leaves the decoys in the live tensors. Times the real run by events."""
    assert c.call is not None and c.outs, c.name
    torch.cuda.synchronize()
    c._load(c.real)
    c._refill()
    log = []
    with recorder(log):
        c.call()                                # first call: module load, opt-ins, the plan -- not timed
        torch.cuda.synchronize()
        c._load(c.real)
        c._refill()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        c.call()
        b.record()
    torch.cuda.synchronize()
    c.ms = a.elapsed_time(b)
    c.entries = sorted(set(log))
    c._check_guards("default-stream run")
    c.want = c._bytes()
    c._load(c.decoy)
    c._refill()
    c.call()
    torch.cuda.synchronize()
    c._check_guards("decoy run")
    got = c._bytes()
    if all(torch.equal(g, w) for g, w in zip(got, c.want)):
        raise ContractError("%s: the decoy inputs give the same output bytes as the real ones: the case cannot tell the two apart" % c.name)
    return c


def gated_group(cases, gate=None, stream=None, check_stream_handle=True):
    """The gated section for up to ~10 prepared cases behind one blocker -> [Report]."""
    gate = gate or Gate.get()
    S = stream or gate.require_stream()
    assert 0 < len(cases) <= MAX_GROUP + 2, len(cases)
    longest = max(c.ms for c in cases)
    scale = gate.scale_for(longest)
    print("gated group of %d: blocker %d x %d cycles = %.0f ms; longest case on the default stream %.3f ms (x %.0f)" % (
        len(cases), scale, gate.cycles, scale * gate.block_ms, longest, scale * gate.block_ms / max(longest, 1e-6)), flush=True)
    reports = [Report(c) for c in cases]
    ev = torch.cuda.Event()
    # the allocator's counters are process-wide: cyclic garbage of earlier tests that the collector happens to free during a call would be
    # charged to that call, so it is collected now and the collector stays off while the group is queued
    gc.collect()
    gc_was_on = gc.isenabled()
    gc.disable()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        with torch.cuda.stream(S):
            gate.block(scale)
            ev.record(S)
            for c, r in zip(cases, reports):
                c._refill()
                c._load(c.real)
                log = []
                before = _alloc_stats()
                with recorder(log, S.cuda_stream if check_stream_handle else None):
                    c.call()
                r.early = not ev.query()
                after = _alloc_stats()
                r.allocated = (after[0] - before[0]) + (after[2] - before[2])
                r.freed = (after[1] - before[1]) + (after[3] - before[3])
    finally:
        if gc_was_on:
            gc.enable()
    host_ms = (time.perf_counter() - t0) * 1e3
    S.synchronize()
    torch.cuda.synchronize()
    print("gated group queued in %.2f ms of host time; early: %s" % (host_ms, [r.early for r in reports]), flush=True)
    for c, r in zip(cases, reports):
        try:
            c._check_guards("gated run")
        except kg.GuardError as e:
            r.guard_error = str(e)
        got = c._bytes()
        bad = ["output %d: %d of %d bytes differ" % (i, int((g != w).sum()), g.numel()) for i, (g, w) in enumerate(zip(got, c.want)) if not torch.equal(g, w)]
        r.bytes_equal, r.mismatch = not bad, "; ".join(bad)
    return reports


def run_family(builders, early=True, alloc=True):
    """builders: callables -> Case. Sets each up, gates them in groups of MAX_GROUP, asserts the contract -> the cases (for coverage)."""
    cases = [setup_case(b()) for b in builders]
    for i in range(0, len(cases), MAX_GROUP):
        reports = gated_group(cases[i:i + MAX_GROUP])
        problems = []
        for r in reports:
            problems += ["%s: %s" % (r.name, f) for f in r.faults(early, alloc)]
        assert not problems, "stream contract broken:\n  " + "\n  ".join(problems)
    for c in cases:
        print("[PASS] gated %-60s %s" % (c.name, ",".join(c.entries)), flush=True)
    return cases
