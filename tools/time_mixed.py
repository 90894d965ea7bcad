#!/usr/bin/env python3
"""Throughput of three patches that combine the extension nodes -- (i) UnisonSawtooth -> ResonantLowPass, (ii) Wavetable ->
ResonantLowPass, (iii) UnisonSawtooth -> ResonantLowPass -> Shaper; 1024 voices under a stereo SumBus, 48 kHz -- three ways, timed in
alternation: one kernel per node (mixed_programs=False, what such a graph runs without the option: the baseline), the mixed
voice-program interpreter, and the kernel specialised for the program.  Every route is built and warmed once; then `rounds` rounds
time each route in turn over a window of `window` seconds of back-to-back batches, so that clock and temperature drift hit all three
alike.  Attached specialised kernels are process-wide and found by the program's words, so every warm-up and every window switches
them on for the specialised route and off for the other two (sig_voice_program_use_attached): the interpreter route runs
voice_program_kernel<.., vp_family::mixed>.  Per patch one JSON object:
the median over the rounds per route, the spread (max - min over the rounds, relative to the median) per route, and whether the
interpreter beats the baseline by more than the larger of the two spreads.

    python tools/time_mixed.py [blocks per batch] [block frames] [rounds] [window seconds]        (needs a GPU)
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
ROUTES = {'per_node': {'mixed_programs': False}, 'interpreter': {'mixed_programs': True, 'fuse_program': 'always'},
          'specialised': {'mixed_programs': True, 'fuse_program': 'always', 'specialise': True}}


def voice(V, which):
    from signals_amd.chain import ext
    p = cfg.c2_params(V)
    rng = np.random.default_rng(2)
    if which == 'wavetable_resonant':
        src = ext.Wavetable()
        k = np.arange(256)[:, None] / 256.0
        src.get_state().table = np.concatenate([np.sin(2 * np.pi * k), np.sin(2 * np.pi * k) ** 3], axis=1)
        src.hertz = cfg.fixed(p['hertz']); src.phase = cfg.fixed(p['phase']); src.select = cfg.fixed((np.arange(V) % 2).astype(float)[None, :])
    else:
        src = ext.UnisonSawtooth()
        src.hertz = cfg.fixed(p['hertz']); src.phase = cfg.fixed(p['phase']); src.spread = cfg.fixed(np.ones((1, 1)))
    top = ext.ResonantLowPass(); top.input = src; top.cutoff = cfg.fixed(p['cutoff']); top.resonance = cfg.fixed(rng.uniform(0.6, 4.0, (1, V)))
    if which == 'supersaw_resonant_shaper':
        s = ext.Shaper(); s.get_state().table = np.tanh(2.0 * np.linspace(-1.0, 1.0, 257))[:, None] / np.tanh(2.0); s.input = top
        top = s
    b = ext.SumBus(); b.input = top; b.get_state().gains = np.ascontiguousarray(p['pan'])
    return b


class Route:
    def __init__(self, build, N, K, **kw):
        from signals_amd.engine import BatchRenderer, KernelTimer
        self.timer = KernelTimer(sample_every=4)
        self.attached = bool(kw.get('specialise'))
        self.r = BatchRenderer(build(), 2, RATE, timer=self.timer, **kw)
        self.N, self.K, self.pos = N, K, 0
        self.steps = 4

    def run(self, steps):
        from signals_amd import _native
        _native.voice_program_use_attached(self.attached)                     # (process-wide: set for every burst of launches)
        for _ in range(steps):
            self.r.render(self.pos, self.N, self.K); self.pos += self.N * self.K

    def warm(self, seconds, window):
        """first-launch work, the specialised build, clocks; then the batches per window from the rate seen"""
        t_end = time.perf_counter() + seconds
        while time.perf_counter() < t_end:
            self.run(1)
            torch.cuda.synchronize()
        self.steps = max(4, int(round(window / self.timed(8))))
        self.timer.reset()

    def timed(self, steps=None):
        steps = steps or self.steps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.run(steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps


if __name__ == '__main__':
    from signals_amd import _native, runtime, specialise
    runtime.set_device('cuda:0')
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    window = float(sys.argv[4]) if len(sys.argv) > 4 else 0.5
    V = 1024
    for which in ('supersaw_resonant', 'wavetable_resonant', 'supersaw_resonant_shaper'):
        names = [n for n in ROUTES if n != 'specialised' or specialise.hipcc()]
        routes = {n: Route(lambda: voice(V, which), N, K, **ROUTES[n]) for n in names}
        for r in routes.values():
            r.warm(0.5, window)
        times = {n: [] for n in names}
        for _ in range(rounds):                                               # in alternation
            for n in names:
                times[n].append(routes[n].timed())
        rate = {n: V * N * K / float(np.median(t)) / 1e12 for n, t in times.items()}
        spread = {n: (max(t) - min(t)) / float(np.median(t)) for n, t in times.items()}
        margin = max(spread['per_node'], spread['interpreter'])
        _native.voice_program_use_attached(True)
        print(json.dumps({'patch': which, 'voices': V, 'block_frames': N, 'blocks_per_batch': K, 'rounds': rounds, 'window_s': window,
                          'batches_per_window': {n: routes[n].steps for n in names},
                          **{f'{n}_T': round(rate[n], 3) for n in names},
                          **{f'{n}_spread': round(spread[n], 3) for n in names},
                          'interpreter_beats_per_node': bool(rate['interpreter'] > rate['per_node'] * (1.0 + margin)),
                          **{f'{n}_launches_us': {k: round(e['ms'] / e['calls'] * 1e3, 1) for k, e in routes[n].timer.summary().items()}
                             for n in names}}), flush=True)
