"""The event timer of the engine's launches and the hipGraph capture of a short launch sequence."""
from __future__ import annotations

import typing

import torch

from signals_amd import _native, runtime


class KernelTimer:
    """Optional per-kernel HIP-event timing on the launch stream (bench.py's roofline leg)."""

    def __init__(self, sample_every: int = 1, region: bool = False):
        """`sample_every` = n: only every n-th launch of a kernel is bracketed by events (an event pair between two
        launches drains the queue: bracketing every 200-us launch cost the stream 12 %); the summary's calls, time and
        units then count the bracketed launches only, so its averages stay per launch.
        `region`: ONE event in front of the first launch and one behind the last (`close()`): nothing between the launches, so
        the stream runs exactly as it does untimed; the elapsed time is shared out evenly over the launches (for schedules
        that are one launch per step -- the average then includes the gap between two launches, as the wall clock does)"""
        self.records: list[tuple[str, torch.cuda.Event, torch.cuda.Event, dict]] = []
        self.sample_every = max(1, int(sample_every))
        self.region = region
        self._seen: dict[str, int] = {}
        self._units: dict[str, int] = {}
        self._start = self._stop = None

    def launch(self, name: str, fn: typing.Callable, **meta):
        n = self._seen.get(name, 0)
        self._seen[name] = n + 1
        if self.region:
            self._units[name] = self._units.get(name, 0) + meta.get('units', 0)
            if self._start is None:
                self._start = torch.cuda.Event(enable_timing=True)
                self._start.record()
            return fn()
        if n % self.sample_every:
            return fn()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        self.records.append((name, start, stop, meta))
        return out

    def close(self) -> None:
        """region mode: the event behind the last launch"""
        if self.region and self._start is not None and self._stop is None:
            self._stop = torch.cuda.Event(enable_timing=True)
            self._stop.record()

    def summary(self) -> dict[str, dict]:
        """call after a device sync"""
        acc: dict[str, dict] = {}
        if self.region:
            self.close()
            if self._start is None:
                return acc
            total, launches = self._start.elapsed_time(self._stop), sum(self._seen.values())
            for name, calls in self._seen.items():
                acc[name] = {'calls': calls, 'ms': total * calls / launches, 'units': self._units.get(name, 0)}
            return acc
        for name, start, stop, meta in self.records:
            e = acc.setdefault(name, {'calls': 0, 'ms': 0.0, 'units': 0})
            e['calls'] += 1
            e['ms'] += start.elapsed_time(stop)
            e['units'] += meta.get('units', 0)
        return acc

    def reset(self):
        self.records.clear()
        self._seen.clear()
        self._units.clear()
        self._start = self._stop = None


class _CapturedLaunches:
    """A short launch sequence captured once into a hipGraph (torch.cuda.CUDAGraph on ROCm) and replayed per
    call: the frame position lives in a device int64 that the kernels read and the graph's last node
    advances, so consecutive blocks replay with no host work beyond one graph launch.  The output buffer is
    owned by the graph and overwritten by every replay."""

    def __init__(self, record: typing.Callable[[torch.Tensor], torch.Tensor], advance: int, position: int, keys: tuple,
                 self_advancing: bool = False):
        """`self_advancing`: the recorded launches move the device position themselves (sig_latency_voice_bus)"""
        dev = runtime.device()
        self.keys = keys                                    # identities of the tensors baked into the graph
        self.advance = advance
        self.pos = torch.tensor([position], dtype=torch.int64, device=dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                       # warm-up outside capture, as graph capture requires
            record(self.pos)
        torch.cuda.current_stream(dev).wait_stream(side)
        self.pos.fill_(position)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = record(self.pos)
            if not self_advancing:
                _native.advance_position(self.pos, advance)
        self.pos.fill_(position)
        self.next_position = position

    def run(self, position: int) -> torch.Tensor:
        if position != self.next_position:
            self.pos.fill_(position)                        # seek
        self.graph.replay()
        self.next_position = position + self.advance
        return self.out
