#!/usr/bin/env python3
"""Throughput of a resonant voice -- ResonantLowPass(Sawtooth), 1024 voices, 48 kHz, q dealt from {0.5, 1/sqrt2, 2, 8} -- (i) storing
its rows and (ii) under a stereo SumBus, four ways: the eager pull path block by block, one kernel per node (fuse=False), the
voice-program interpreter, and the voice program specialised for the graph.  The same graphs with fx.LowPass in place of the resonant
node are timed in the same run, route by route and taking turns, so that the two can be compared against the run's own spread: every
batched figure is the median of `REPEATS` timed runs of about a quarter of a second each after a warm-up, printed with the lowest and
the highest of them.  Prints one JSON object per (shape, filter).

    python tools/time_resonant.py [blocks per batch] [block frames]        (needs a GPU)
"""
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

import bench_configs as cfg

RATE = 48000
REPEATS = 5
QS = (0.5, 2.0 ** -0.5, 2.0, 8.0)


def voice(V, resonant, bus):
    from signals_amd.chain import ext, fx, osc
    p = cfg.c2_params(V)
    o = osc.Sawtooth()
    o.hertz = cfg.fixed(p['hertz']); o.phase = cfg.fixed(p['phase'])
    if resonant:
        f = ext.ResonantLowPass()
        f.resonance = cfg.fixed(np.array([QS[v % 4] for v in range(V)])[None, :])
    else:
        f = fx.LowPass()
    f.input = o; f.cutoff = cfg.fixed(p['cutoff'])
    if not bus:
        return f, V
    b = ext.SumBus(); b.input = f; b.get_state().gains = np.ascontiguousarray(p['pan'])
    return b, 2


def eager(build, V, N, blocks):
    """the pull path: one request per block through the nodes' own respond()"""
    from signals_amd import SignalFlags
    from signals_amd.chain import BlockLoc, Receiver, Shape, port

    class Probe(Receiver):
        input = port('input')
        HOST_ARRAYS = False

        @classmethod
        def flags(cls):
            return SignalFlags(0)
    d = Probe()
    d.input, C = build()
    loc = lambda b: BlockLoc(position=b * N, rate=RATE, shape=Shape(frames=N, channels=C))
    for b in range(4):
        d.input.request(loc(b))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(4, 4 + blocks):
        d.input.request(loc(b))
    torch.cuda.synchronize()
    return V * N * blocks / (time.perf_counter() - t0) / 1e12


def batched(builds, V, N, K, **kw):
    """per build of `builds` (the resonant and the plain voice): (median, lowest, highest) T voice-samples/s over REPEATS timed runs
    and the launches of the route.  The builds take turns, run by run, so that a drift of the machine meets both alike; every run
    lasts about a quarter of a second (its render count comes from the warm-up's pace)"""
    from signals_amd import _native
    from signals_amd.engine import BatchRenderer, KernelTimer
    _native.voice_program_use_attached(bool(kw.get('specialise')))

    def renderer(build, **more):
        top, C = build()
        r = BatchRenderer(top, C, RATE, **more, **kw)
        if kw.get('fuse_program') == 'always':
            # the program routes: the fused Filter(Osc) kernels, which would take the LowPass voice first, are switched off, so
            # that both filters run the voice program and the comparison is between its two variants
            r.fuse = r.fuse_bus = r.fuse_cascade = False
        return r

    def run(r, pos, steps):
        t0 = time.perf_counter()
        for _ in range(steps):
            r.render(pos, N, K); pos += N * K
        torch.cuda.synchronize()
        return pos, time.perf_counter() - t0
    state = []
    for build in builds:
        r = renderer(build)
        pos, _ = run(r, 0, 2)                                                # (code objects loaded, a specialised kernel built)
        done, spent = 0, 0.0
        while spent < 0.3:
            pos, dt = run(r, pos, 2)
            done, spent = done + 2, spent + dt
        state.append([r, pos, max(2, int(round(0.25 * done / spent))), []])
    for _ in range(REPEATS):
        for entry in state:
            r, pos, steps, rates = entry
            entry[1], dt = run(r, pos, steps)
            rates.append(V * N * K * steps / dt / 1e12)
    out = []
    for build, (r, pos, steps, rates) in zip(builds, state):
        timer = KernelTimer()
        renderer(build, timer=timer).render(0, N, K)
        torch.cuda.synchronize()
        out.append(([round(float(x), 3) for x in (np.median(rates), min(rates), max(rates))], sorted(timer.summary())))
    return out


if __name__ == '__main__':
    from signals_amd import runtime, specialise
    runtime.set_device('cuda:0')
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    V = 1024
    routes = [('per_node', {'fuse': False}), ('interpreter', {'fuse_program': 'always'})]
    if specialise.hipcc():
        routes.append(('specialised', {'fuse_program': 'always', 'specialise': True}))
    for bus in (False, True):
        builds = [lambda resonant=resonant: voice(V, resonant, bus) for resonant in (True, False)]
        lines = [{'shape': 'voice_bus' if bus else 'voice', 'filter': name, 'voices': V, 'block_frames': N, 'blocks_per_batch': K,
                  'eager_T': round(eager(build, V, N, 64), 4)} for name, build in zip(('ResonantLowPass', 'LowPass'), builds)]
        for route, kw in routes:
            for line, (rates, launches) in zip(lines, batched(builds, V, N, K, **kw)):
                line[route + '_T'], line[route + '_launches'] = rates, launches
        for line in lines:
            print(json.dumps(line), flush=True)
