#!/usr/bin/env python3
"""Throughput of the filter-envelope voice, 1024 voices, stereo bus, 48 kHz: the C2 voice, SumBus(Gain(LowPass(Sine))), with
the cutoff on an envelope, cutoff = Mix(Fixed(6000), Fixed(300), mix=ADSR) with per-voice envelope times (gate times
are absolute: the envelopes are spread over the first seconds of the stream; the work per block does not depend on the stage), as
  envelope:  the default schedule, and specialise=True -- the ADSR as a word of the block-rate control program;
  lfo:       the same voice with a Sine LFO on the cutoff in place of the envelope, its batched neighbour;
  eager:     the envelope voice through BlockDriver, one pull per block -- what the graph ran on before the engine had the word.
Prints one JSON object: us per batch (per block for the eager path), T voice-samples/s and the control-program launch's own
time (KernelTimer).

    python tools/time_envelope.py [blocks per batch] [block frames]        (needs a GPU)
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
BASE, PEAK = 300.0, 6000.0


def graph(which, V):
    from signals_amd.chain import ext, fx, osc
    p = cfg.c2_params(V)
    o = osc.Sine(); o.hertz = cfg.fixed(p['hertz']); o.phase = cfg.fixed(p['phase'])
    f = fx.LowPass(); f.input = o
    m = fx.Mix(); m.left = cfg.fixed([[PEAK]]); m.right = cfg.fixed([[BASE]])
    if which == 'envelope':
        rng = np.random.default_rng(3)
        on = rng.uniform(0.0, 4.0, (1, V))
        env = ext.ADSR()
        env.attack = cfg.fixed(rng.uniform(0.002, 0.05, (1, V))); env.decay = cfg.fixed(rng.uniform(0.05, 0.4, (1, V)))
        env.sustain = cfg.fixed(rng.uniform(0.1, 0.6, (1, V))); env.release = cfg.fixed(rng.uniform(0.05, 0.5, (1, V)))
        env.gate_on = cfg.fixed(on); env.gate_off = cfg.fixed(on + rng.uniform(0.2, 1.0, (1, V)))
        m.mix = env
    else:                                                      # 0.5 + 0.5 sin: the same range of cutoffs
        lfo = osc.Sine(); lfo.hertz = cfg.fixed(np.random.default_rng(3).uniform(0.5, 4.0, (1, V)))
        unit = fx.Mix(); unit.left = lfo; unit.right = cfg.fixed([[1.0]]); unit.mix = cfg.fixed([[0.5]])   # 0.5 sin + 0.5
        m.mix = unit
    f.cutoff = m
    g = fx.Gain(); g.left = f; g.right = cfg.fixed(p['gain'])
    b = ext.SumBus(); b.input = g; b.get_state().gains = np.ascontiguousarray(p['pan'])
    return b


def batched(which, V, N, K, steps, **kw):
    from signals_amd import _native
    from signals_amd.engine import BatchRenderer, KernelTimer
    _native.voice_program_use_attached(bool(kw.get('specialise')))
    timer = KernelTimer(sample_every=4)
    r = BatchRenderer(graph(which, V), 2, RATE, timer=timer, **kw)
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


def eager(V, N, blocks):
    from signals_amd.chain.driver import BlockDriver
    d = BlockDriver(blocksize=N); d.get_state().channels = 2; d.input = graph('envelope', V)
    d.render(4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d.render(blocks)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / blocks
    return {'us_per_block': round(dt * 1e6, 1), 'T': round(V * N / dt / 1e12, 6)}


if __name__ == '__main__':
    from signals_amd import runtime, specialise
    runtime.set_device('cuda:0')
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    V = 1024
    out = {'voices': V, 'block_frames': N, 'blocks_per_batch': K,
           'eager_block_driver': eager(V, N, 64),
           'envelope_default': batched('envelope', V, N, K, 10),
           'envelope_specialised': batched('envelope', V, N, K, 10, specialise=True) if specialise.hipcc() else None,
           'lfo_default': batched('lfo', V, N, K, 10)}
    out['envelope_over_eager'] = round(out['envelope_default']['T'] / out['eager_block_driver']['T'], 1)
    out['envelope_over_lfo_batch_time'] = round(out['envelope_default']['us_per_batch'] / out['lfo_default']['us_per_batch'], 3)
    print(json.dumps(out), flush=True)
