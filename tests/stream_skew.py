"""Skewed-stream harness for the C ABI's stream contract (a plain helper module, imported by tests/test_gpu_stream_skew_harness.py
and tests/stream_order_runner.py).

include/imk.h: a call enqueues on `stream`, never synchronises, and leaves all of its work -- the part on the pool's side streams
included -- ordered after prior work on `stream` and before later work on `stream`.  With every stream idle, a side stream trails
the caller's by microseconds and a missing fork, a missing join or a write-after-read on a reused buffer comes out right by luck.
Here ONE stream is held back for a bounded time, so that the others run as far ahead as their dependencies allow, while every
buffer a premature reader could touch holds poison:

  * the caller's stream held: the inputs are produced BEHIND the hold (their device buffers hold poison until then), so work that
    a call puts on a side stream without making it wait for the caller's stream reads poison;
  * a side stream held: the caller's stream runs on to the end of the call, clones the outputs and overwrites the inputs with
    poison (the caller reusing its buffers right behind the call); side-stream work that the caller's stream was not made to
    wait for has then not written its results yet, or reads poison when it finally runs.

A hold is torch.cuda._sleep: a kernel that spins on the clock for a number of cycles and ends by itself.  No host-released gate, no
wait on a memory value, no dependence on another stream -- two streams that share a hardware queue cannot deadlock on it (the skew
is then weaker, never wrong).  The fills are tests/arena.py's: 0xFF (fp16 / fp32 NaN) and 0x3C (plausible finite fp16 values).
"""
import ctypes
import hashlib
import time

import torch

FILLS = (0xFF, 0x3C)
MIN_HOLD_MS = 50.0
HOLD_FACTOR = 20.0
_CYCLES_PER_MS = None


def as_bytes(t):
    """a contiguous tensor of any dtype as a flat uint8 VIEW of its memory"""
    assert t.is_contiguous(), "buffers handed to the harness are contiguous (a copy would be poisoned instead of the buffer)"
    return t.reshape(-1).view(torch.uint8)


def poison(t, fill):
    as_bytes(t).fill_(fill)


def digest(outs):
    """sha256 over the named outputs {name: uint8 tensor}, names in sorted order"""
    h = hashlib.sha256()
    for name in sorted(outs):
        h.update(name.encode())
        h.update(outs[name].cpu().numpy().tobytes())
    return h.hexdigest()


def side_stream(model, i):
    """side stream i (0 .. 1) of the pool every plan of the process shares, as a torch stream (imk_unet_plan_side_stream creates it
    if the library has not done so yet)"""
    from inconsistencymasks_amd._lib import check, lib
    s = ctypes.c_void_p()
    check(lib.imk_unet_plan_side_stream(model.plan.ptr, int(i), ctypes.byref(s)), "imk_unet_plan_side_stream")
    assert s.value, "the pool's side stream is the null stream"
    return torch.cuda.ExternalStream(s.value)


def cycles_per_ms():
    """torch.cuda._sleep's cycles per millisecond, measured once per process with events: the count is doubled until one sleep
    takes at least 5 ms, then the rate is that of a second sleep of the same count"""
    global _CYCLES_PER_MS
    if _CYCLES_PER_MS is None:
        s = torch.cuda.Stream()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed(n):
            with torch.cuda.stream(s):
                a.record(s)
                torch.cuda._sleep(n)
                b.record(s)
            b.synchronize()
            return a.elapsed_time(b)
        n = 100_000
        timed(n)                    # the kernel's first launch
        while timed(n) < 5.0:
            n *= 2
            assert n < 1 << 40, "torch.cuda._sleep does not take time"
        _CYCLES_PER_MS = n / timed(n)
    return _CYCLES_PER_MS


def hold(stream, ms):
    """a finite delay of about `ms` milliseconds on `stream`; returns the event recorded right behind it (its release)"""
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * cycles_per_ms()))
        ev.record(stream)
    return ev


def runs_ahead(stream, held, ms=10.0):
    """True if `stream` gets work done while `held` is held: the two do not share a hardware queue (the runtime multiplexes all
    streams of a process onto a few, and behind a hold every stream of its queue waits -- a skew between two such streams holds
    both back and can show nothing).  One finite hold; the host waits for `stream` only, never for a value."""
    stream.synchronize()
    held.synchronize()
    ev = hold(held, ms)
    done = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.zeros(1, device="cuda").add_(1)
        done.record(stream)
    done.synchronize()
    ahead = not ev.query()
    ev.synchronize()
    return ahead


def caller_stream_beside(others, tries=8):
    """a new torch stream that runs ahead of every stream in `others` and that each of them runs ahead of; (stream, True), or
    (the last candidate, False) if none of `tries` candidates does"""
    cands = [torch.cuda.Stream() for _ in range(tries)]      # all alive at once: the pool hands out distinct streams
    for s in cands:
        if all(runs_ahead(s, o) and runs_ahead(o, s) for o in others):
            return s, True
    return cands[-1], False


def hold_ms_for(wall_ms):
    """max(50 ms, 20 x the undisturbed wall time of the call plus its synchronise)"""
    return max(MIN_HOLD_MS, HOLD_FACTOR * wall_ms)


def _calls(call):
    return list(call) if isinstance(call, (list, tuple)) else [call]


def wall_ms(call, inputs, caller_stream, runs=5):
    """median wall time in ms of the call(s) plus a synchronise, every stream undisturbed (the inputs restored before each run)"""
    times = []
    for _ in range(runs):
        with torch.cuda.stream(caller_stream):
            for buf, pristine in inputs.values():
                as_bytes(buf).copy_(as_bytes(pristine))
            caller_stream.synchronize()
            t0 = time.perf_counter()
            for f in _calls(call):
                f()
            caller_stream.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    return sorted(times)[len(times) // 2]


def run_skewed(call, inputs, outputs, scratch, skew, caller_stream, fill=0xFF, hold_ms=MIN_HOLD_MS, sides=None, timing=None):
    """One run of `call` under a skew, all of it on the non-default stream `caller_stream` (S).

    call      a callable, or a list of callables made back to back with no host synchronisation in between; each enqueues on the
              current stream (S) and must not synchronise
    inputs    {name: (device buffer, pristine device copy)}: what the call reads (read-write state included)
    outputs   {name: device tensor}: what is compared (a view into a larger buffer is fine; a name may also be an input's)
    scratch   [device tensors]: workspaces and whole output allocations, poisoned on entry
    skew      names of the streams held BEFORE the first call, "main" = S and every other name a key of `sides`; or
              {call index: names} for holds placed in front of a later call of the list
    sides     {name: torch stream}

    Order: (1) outputs, scratch and the inputs' device buffers filled with `fill`; (2) S held if "main" is in the skew;
    (3) the pristine inputs copied into their buffers on S, behind the hold; (4) the side streams of the skew held; (5) the calls;
    (6) no hold may have been released by now, else the run FAILS naming the times; (7) on S every output cloned, then the input
    buffers filled with `fill` again; (8) S synchronised.  Returns {name: uint8 clone}.
    timing (a dict, optional) receives `returned_ms` and `synced_ms`: when the last call had returned and when S had been
    synchronised, both counted from just before the first hold was enqueued -- under the hold of a stream the call joins, S cannot
    be through before the hold is."""
    sides = sides or {}
    calls = _calls(call)
    skew = dict(skew) if isinstance(skew, dict) else {0: tuple(skew)}
    for names in skew.values():
        for n in names:
            assert n == "main" or n in sides, f"unknown stream {n!r} in the skew"
    assert caller_stream != torch.cuda.default_stream(), "the caller's stream must not be the default stream"
    holds = []
    with torch.cuda.stream(caller_stream):
        for t in list(outputs.values()) + list(scratch) + [buf for buf, _ in inputs.values()]:      # (1)
            poison(t, fill)
        t0 = time.perf_counter()
        if "main" in skew.get(0, ()):                                                                # (2)
            holds.append(("main", hold(caller_stream, hold_ms)))
        for buf, pristine in inputs.values():                                                        # (3)
            as_bytes(buf).copy_(as_bytes(pristine), non_blocking=True)
        for i, f in enumerate(calls):
            for n in skew.get(i, ()):                                                                # (4)
                if n != "main":
                    holds.append((n, hold(sides[n], hold_ms)))
                elif i > 0:
                    holds.append((n, hold(caller_stream, hold_ms)))
            f()                                                                                      # (5)
        returned_ms = (time.perf_counter() - t0) * 1e3
        released = [n for n, ev in holds if ev.query()]                                              # (6)
        snaps = {name: as_bytes(t.contiguous()).clone() for name, t in outputs.items()}              # (7)
        for buf, _ in inputs.values():
            poison(buf, fill)
        caller_stream.synchronize()                                                                  # (8)
        synced_ms = (time.perf_counter() - t0) * 1e3
    if timing is not None:
        timing.update(returned_ms=returned_ms, synced_ms=synced_ms)
    for _, ev in holds:
        ev.synchronize()
    if released:
        raise AssertionError(f"the skew was not real: the hold(s) on {released} of {hold_ms:.1f} ms each had been released when the "
                             f"call(s) returned, {returned_ms:.1f} ms after the first hold was enqueued")
    return snaps
