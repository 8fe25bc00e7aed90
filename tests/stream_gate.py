"""A gate that makes stream-ordering mistakes deterministic (tests/test_gpu_streams.py).

On the default stream an ordering mistake is invisible: the null stream is ordered with itself and with every
blocking call.  Here the library runs on a side stream from torch's pool (non-blocking: not ordered with the
null stream) that is held shut by a spinning kernel:

    g = gate.shut(host_seconds)          # torch.cuda._sleep on the side stream, an event behind it
    g.stage(actions, real_actions)       # actions holds a sentinel; the real contents arrive behind the sleep
    with g.stream():
        env.step_actions(actions)        # the call under test
    assert g.still_shut()                # it returned while the gate was shut: no host synchronisation
    g.side.synchronize()

A launch that is not on the side stream, or that does not wait for what the side stream holds, runs while the
gate is shut: it reads the sentinels, or state its predecessors have not written yet, and the result differs
from the same calls on the default stream.  Every sentinel is a value the kernels accept (SENTINELS), so a
mis-ordered launch gives a wrong result, never an access out of range.

The hold is not fixed in advance.  The spin is calibrated once per process (cycles per millisecond, timed with
two events on the side stream); each chain is run once ungated on the side stream as a warm pass, which absorbs
first-use allocations and attribute queries, and its host time is the yardstick: the gate holds for the larger
of MIN_HOLD_S and HOLD_FACTOR times that (the factor covers host jitter on a shared machine).  A hold above
MAX_HOLD_S fails the test, so that none becomes slow quietly.  Every figure is printed with a `stream-gate`
prefix."""
from __future__ import annotations

import contextlib
import time

import torch

MIN_HOLD_S = 0.050
HOLD_FACTOR = 10.0
MAX_HOLD_S = 0.500
CALIBRATION_CYCLES = 20_000_000

# what an input holds before its real contents are staged through the gate
SENTINELS = {
    "actions": 255,      # the invalid code: counted per env by error_count(), the env does not move
    "obs_int8": 0x7F,    # int8 observation rows
    "indices": 0,        # sample indices, snapshot slot and env lists: slot or env 0
    "mask": 0,           # a reset of no env
    "weights": 0.0,
}


class ShutGate:
    """One hold of the side stream: made by StreamGate.shut()."""

    def __init__(self, side, event, hold_s: float):
        self.side, self.event, self.hold_s = side, event, hold_s

    def stream(self):
        """The context the library is called in: the side stream current."""
        return torch.cuda.stream(self.side)

    def stage(self, dst, src) -> None:
        """dst <- src on the side stream, behind the sleep.  src is a device tensor whose contents are already
        there (written on the default stream and synchronised), so the copy neither reads host memory nor
        blocks the host."""
        assert src.is_cuda and dst.is_cuda
        with torch.cuda.stream(self.side):
            dst.copy_(src, non_blocking=True)

    def still_shut(self) -> bool:
        """False: the hold was too short, or the call before this one synchronised with the host."""
        return not self.event.query()

    def open(self) -> None:
        """Wait until everything queued on the side stream has run."""
        self.side.synchronize()


class StreamGate:
    """A side stream and its calibrated spin.  One per test module (the calibration is kept)."""

    def __init__(self, device=0):
        self.device = torch.device("cuda", device)
        self.side = torch.cuda.Stream(self.device)
        self.cycles_per_s = None

    def calibrate(self) -> float:
        """Cycles of torch.cuda._sleep per second on this device, from one timed spin (after a short one that
        takes the first launch's overhead)."""
        if self.cycles_per_s is None:
            with torch.cuda.stream(self.side):
                torch.cuda._sleep(100_000)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(self.side)
                torch.cuda._sleep(CALIBRATION_CYCLES)
                e1.record(self.side)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            assert ms > 0.0, "the calibration spin took no time"
            self.cycles_per_s = CALIBRATION_CYCLES / (ms * 1e-3)
            print(f"stream-gate calibration: {CALIBRATION_CYCLES} cycles in {ms:.3f} ms = {self.cycles_per_s:.4g} cycles/s")
        return self.cycles_per_s

    @contextlib.contextmanager
    def on_side(self):
        """The side stream current, ordered behind everything queued so far (the caller's change of stream), and
        drained on the way out."""
        torch.cuda.synchronize(self.device)
        with torch.cuda.stream(self.side):
            yield self.side
        self.side.synchronize()

    def warm(self, name: str, chain) -> float:
        """Run chain() once ungated on the side stream; returns its host time in seconds (the yardstick of the
        hold).  The device is idle before and after."""
        torch.cuda.synchronize(self.device)
        with torch.cuda.stream(self.side):
            t0 = time.perf_counter()
            chain()
            host_s = time.perf_counter() - t0
        self.side.synchronize()
        print(f"stream-gate {name}: warm pass {host_s * 1e3:.3f} ms on the host")
        return host_s

    def hold_for(self, name: str, host_s: float) -> float:
        hold = max(MIN_HOLD_S, HOLD_FACTOR * host_s)
        assert hold <= MAX_HOLD_S, (f"stream-gate {name}: a hold of {hold * 1e3:.0f} ms (host time {host_s * 1e3:.1f} ms) is above "
                                    f"{MAX_HOLD_S * 1e3:.0f} ms: the chain is too long for one gate")
        return hold

    def shut(self, name: str, host_s: float, sleep: bool = True) -> ShutGate:
        """Hold the side stream for hold_for(host_s) from now.  The device is drained first, so what the caller
        wrote on the default stream (sentinels, the staged contents' sources) is there.  sleep=False queues no
        spin: the controls must then fail."""
        hold = self.hold_for(name, host_s)
        cycles = int(hold * self.calibrate())
        torch.cuda.synchronize(self.device)
        event = torch.cuda.Event()
        with torch.cuda.stream(self.side):
            if sleep:
                torch.cuda._sleep(cycles)
            event.record(self.side)
        print(f"stream-gate {name}: hold {hold * 1e3:.1f} ms = {cycles} cycles (host time {host_s * 1e3:.3f} ms)")
        return ShutGate(self.side, event, hold)
