#!/usr/bin/env python3
"""Throughput of voices whose control paths hold a filter, 1024 voices, stereo bus, 48 kHz:
  (a) SumBus(Gain(LowPass(Sine))) with the cutoff a Square LFO through LowPass(4 Hz), scaled to 300-3000 Hz (every voice the
      same LFO; the control filter is as wide as the request, fx.py's per-channel loop);
  (b) the C2 voice, SumBus(Gain(LowPass(Sine))), with LowPass(White, 1 Hz) as +-1 % drift on `hertz` (one column per voice);
each through the eager pull path (one request per block), fuse=False (one kernel per node), the default schedule and
specialise=True, and the same graph with the control filter removed (its input straight into the scaling) as the yardstick.
Prints one JSON object: us per batch, T voice-samples/s and the control-program launch's own time (KernelTimer).

    python tools/time_filtered_control.py [blocks per batch] [block frames]        (needs a GPU)
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


def scaled(src, lo, hi):
    """lo + (hi - lo) * src as Mix(Gain(src, 2 (hi - lo)), 2 lo, 0.5)"""
    from signals_amd.chain import fx
    g = fx.Gain(); g.left = src; g.right = cfg.fixed(2.0 * np.asarray(hi - lo))
    m = fx.Mix(); m.left = g; m.right = cfg.fixed(2.0 * np.asarray(lo)); m.mix = cfg.fixed([[0.5]])
    return m


def graph(which, V, filtered=True):
    from signals_amd.chain import ext, fx, noise, osc
    p = cfg.c2_params(V)
    o = osc.Sine(); o.hertz = cfg.fixed(p['hertz']); o.phase = cfg.fixed(p['phase'])
    f = fx.LowPass(); f.input = o; f.cutoff = cfg.fixed(p['cutoff'])
    if which == 'a':
        lfo = osc.Square(); lfo.hertz = cfg.fixed([[3.0] * V])
        src = lfo
        if filtered:
            src = fx.LowPass(); src.input = lfo; src.cutoff = cfg.fixed([[4.0] * V])
        f.cutoff = scaled(src, 300.0, 3000.0)
    else:
        w = noise.White(); w.get_state().channels = V; w.get_state().seed = 7
        src = w
        if filtered:
            src = fx.LowPass(); src.input = w; src.cutoff = cfg.fixed([[1.0] * V])
        hz = np.asarray(p['hertz'])
        o.hertz = scaled(src, 0.99 * hz, 1.01 * hz)
    g = fx.Gain(); g.left = f; g.right = cfg.fixed(p['gain'])
    b = ext.SumBus(); b.input = g; b.get_state().gains = np.ascontiguousarray(p['pan'])
    return b


def batched(which, V, N, K, steps, filtered=True, **kw):
    from signals_amd import _native
    from signals_amd.engine import BatchRenderer, KernelTimer
    _native.voice_program_use_attached(bool(kw.get('specialise')))
    timer = KernelTimer(sample_every=4)
    r = BatchRenderer(graph(which, V, filtered), 2, RATE, timer=timer, **kw)
    pos = 0
    t_end = time.perf_counter() + 0.3
    while time.perf_counter() < t_end:
        r.render(pos, N, K); pos += N * K
        torch.cuda.synchronize()
    timer.reset()
    t0 = time.perf_counter()
    for _ in range(steps):
        r.render(pos, N, K); pos += N * K
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    launches = {k: round(e['ms'] / e['calls'] * 1e3, 1) for k, e in timer.summary().items()}
    ctl = sum(v for k, v in launches.items() if k.startswith('control_program['))
    return {'us_per_batch': round(dt * 1e6, 1), 'T': round(V * N * K / dt / 1e12, 4), 'control_us': round(ctl, 1),
            'launches_us': launches}


def eager(which, V, N, blocks, filtered=True):
    from signals_amd.chain import BlockLoc, Shape
    sys.path.insert(0, str(ROOT / 'tests'))
    from helpers import Probe
    probe = Probe()
    probe.input = graph(which, V, filtered)
    pos = 0
    for _ in range(4):
        probe.input.request(BlockLoc(position=pos, rate=RATE, shape=Shape(frames=N, channels=2))); pos += N
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(blocks):
        probe.input.request(BlockLoc(position=pos, rate=RATE, shape=Shape(frames=N, channels=2))); pos += N
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / blocks
    return {'us_per_block': round(dt * 1e6, 1), 'T': round(V * N / dt / 1e12, 6)}


if __name__ == '__main__':
    from signals_amd import runtime, specialise
    runtime.set_device('cuda:0')
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    V = 1024
    out = {'voices': V, 'block_frames': N, 'blocks_per_batch': K}
    for which in ('a', 'b'):
        e = eager(which, V, N, 64)
        res = {'eager': e,
               'per_node': batched(which, V, N, K, 4, fuse=False),
               'default': batched(which, V, N, K, 10),
               'specialised': batched(which, V, N, K, 10, specialise=True) if specialise.hipcc() else None,
               'unfiltered_default': batched(which, V, N, K, 10, filtered=False)}
        res['default_over_eager'] = round(res['default']['T'] / e['T'], 1)
        res['default_over_unfiltered_batch_time'] = round(res['default']['us_per_batch'] / res['unfiltered_default']['us_per_batch'], 3)
        out[which] = res
    print(json.dumps(out), flush=True)
