"""A torch stream that is BEHIND: lagging(stream) enqueues a delay on it and returns an event recorded right after the delay.

While event.query() is False the stream has not reached whatever was enqueued behind the delay: the host is ahead of the
device by at least that much, which is how a prover that keeps several streams busy sees the library, and how the default-stream
tests never do.  A call issued then must be ORDERED behind the stream's earlier work -- it cannot rely on it having finished.

The delay is plain torch work that has nothing to do with the engine under test: element-wise passes over one large tensor, each
a kernel of its own, so the length is a number of passes.  The time of one pass is measured once per module with events on the side
stream while it is idle (calibration(): it takes no stream of its own); the number of passes is chosen to give TARGET_MS, and
release() gives the tensor back when the module is through.  A test proves that the delay outlasted the host's issue of its call
by asserting event.query() is False -- after a call that only enqueues, immediately before a call that synchronises."""
from __future__ import annotations

import math

import torch

TARGET_MS = 50.0          # the delay aimed at
WORDS = 1 << 27           # int64 elements of the tensor the passes sweep (1 GiB: a pass is ~2 GiB of traffic, a fraction of a ms)
PROBE_PASSES = 32         # passes timed by the calibration

_state: dict = {}

LATE = ("the stream caught up with the host before the call under test was issued: the delay was too short for this call, or the "
        "call allocated (an engine's scratch growing, torch's allocator asking the driver) -- warm it up with the same shapes first")


def _passes(x: torch.Tensor, count: int) -> None:
    for _ in range(count):
        x.add_(1)


def calibration(stream: torch.cuda.Stream) -> dict:
    """{"ms_per_pass", "passes", "delay_ms"}: one pass timed with events on `stream`, which must be idle (the mean of PROBE_PASSES
    after a warm-up), the passes lagging() enqueues and the delay they amount to.  Measured once; release() forgets it."""
    if not _state:
        torch.cuda.synchronize(stream.device)
        x = torch.zeros((WORDS,), dtype=torch.int64, device=stream.device)
        with torch.cuda.stream(stream):
            _passes(x, 4)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            _passes(x, PROBE_PASSES)
            t1.record(stream)
        stream.synchronize()
        per = t0.elapsed_time(t1) / PROBE_PASSES
        count = max(1, math.ceil(TARGET_MS / per))
        _state.update(x=x, ms_per_pass=per, passes=count, delay_ms=per * count)
    return {k: _state[k] for k in ("ms_per_pass", "passes", "delay_ms")}


def release() -> None:
    """give the swept tensor back (the device synchronised first): what runs later in the process has the whole card again"""
    if _state:
        torch.cuda.synchronize(_state["x"].device)
        _state.clear()
        torch.cuda.empty_cache()


def lagging(stream: torch.cuda.Stream, factor: float = 1.0) -> torch.cuda.Event:
    """enqueue the delay (factor times TARGET_MS) on `stream`; the event returned is recorded right after it.  The stream's earlier
    work is untouched, and so is torch's current stream."""
    calibration(stream)
    with torch.cuda.stream(stream):
        _passes(_state["x"], max(1, math.ceil(_state["passes"] * factor)))
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev
