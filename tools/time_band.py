#!/usr/bin/env python3
"""Throughput of a swept band-filter voice -- SumBus(Gain(BandPass(Sawtooth))) with `low` and `high` on block-rate LFOs, 1024
voices, stereo bus, 48 kHz -- four ways: the eager pull path (one request per block), one kernel per node (band_coldstart with
one band per block), the voice-program interpreter (Band instruction) and the voice program specialised for this graph.
Prints one JSON object.

    python tools/time_band.py [blocks per batch] [block frames]        (needs a GPU)
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


def lfo(hz, depth, centre):
    """depth * sin + centre per voice, as Mix(Gain(Sine, 2 depth), 2 centre, 0.5)"""
    from signals_amd.chain import fx, osc
    s = osc.Sine(); s.hertz = cfg.fixed([[hz]])
    g = fx.Gain(); g.left = s; g.right = cfg.fixed(2.0 * np.asarray(depth))
    m = fx.Mix(); m.left = g; m.right = cfg.fixed(2.0 * np.asarray(centre)); m.mix = cfg.fixed([[0.5]])
    return m


def swept_band_voice(V, cls='BandPass'):
    from signals_amd.chain import ext, fx, osc
    p = cfg.c2_params(V)
    rng = np.random.default_rng(2)
    lo = rng.uniform(150, 2500, (1, V))
    hi = lo * rng.uniform(2.5, 4.0, (1, V))
    o = osc.Sawtooth(); o.hertz = cfg.fixed(p['hertz']); o.phase = cfg.fixed(p['phase'])
    f = getattr(fx, cls)(); f.input = o; f.low = lfo(1.7, 0.4 * lo, lo); f.high = lfo(3.1, 0.3 * hi, hi)
    g = fx.Gain(); g.left = f; g.right = cfg.fixed(p['gain'])
    b = ext.SumBus(); b.input = g; b.get_state().gains = np.ascontiguousarray(p['pan'])
    return b


def batched(V, N, K, steps, **kw):
    from signals_amd import _native
    from signals_amd.engine import BatchRenderer, KernelTimer
    _native.voice_program_use_attached(bool(kw.get('specialise')))
    timer = KernelTimer(sample_every=4)
    r = BatchRenderer(swept_band_voice(V), 2, RATE, timer=timer, **kw)
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
    return V * N * K / dt / 1e12, {k: round(e['ms'] / e['calls'] * 1e3, 1) for k, e in timer.summary().items()}


def eager(V, N, blocks):
    from signals_amd.chain import BlockLoc, Shape
    sys.path.insert(0, str(ROOT / 'tests'))
    from helpers import Probe
    probe = Probe()
    probe.input = swept_band_voice(V)
    pos = 0
    for _ in range(8):
        probe.input.request(BlockLoc(position=pos, rate=RATE, shape=Shape(frames=N, channels=2))); pos += N
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(blocks):
        probe.input.request(BlockLoc(position=pos, rate=RATE, shape=Shape(frames=N, channels=2))); pos += N
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / blocks
    return V * N / dt / 1e12, dt * 1e6


if __name__ == '__main__':
    from signals_amd import runtime, specialise
    runtime.set_device('cuda:0')
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    V = 1024
    eager_T, eager_us = eager(V, N, 256)
    node_T, node_launches = batched(V, N, K, 4, fuse_program=False)
    prog_T, prog_launches = batched(V, N, K, 10, fuse_program='always')
    spec_T, spec_launches = batched(V, N, K, 10, fuse_program='always', specialise=True) if specialise.hipcc() else (None, {})
    print(json.dumps({'shape': 'swept_bandpass_voice', 'voices': V, 'block_frames': N, 'blocks_per_batch': K,
                      'eager_T': round(eager_T, 4), 'eager_us_per_block': round(eager_us, 1),
                      'per_node_T': round(node_T, 3), 'per_node_launches_us': node_launches,
                      'interpreter_T': round(prog_T, 3), 'interpreter_launches_us': prog_launches,
                      'specialised_T': spec_T and round(spec_T, 3), 'specialised_launches_us': spec_launches}), flush=True)
