#!/usr/bin/env python3
"""Timing of the short delay line.  (i) sig_delay_taps alone -- 1024 voices, blocks of 256 frames, float32 in and out (8 B per
voice-sample), U = 1 and U = 4 taps, one time row for the launch and one per block -- next to elementwise[Gain] on the same shape
in the same session (the same 8 B per voice-sample) and the 8 TB/s HBM roof.  (ii) the flanger voice under a stereo bus,
SumBus(Mix(Sawtooth, Delay(Sawtooth, time = LFO))): one kernel per node in the batched engine, with the per-launch figures, against
(a) the eager pull path block by block and (b) the same voice without the Delay, SumBus(Mix(Sawtooth, Sawtooth')), which needs no
Delay to render.  Prints one JSON object per kernel line and one per shape.

    python tools/time_delay.py [blocks per batch] [block frames]        (needs a GPU)
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
HBM_ROOF = 8.0e12


def voice(V, delayed):
    from signals_amd.chain import ext, fx, osc
    p = cfg.c2_params(V)
    dry = osc.Sawtooth()
    dry.hertz = cfg.fixed(p['hertz']); dry.phase = cfg.fixed(p['phase'])
    if delayed:
        lfo = osc.Sine(); lfo.hertz = cfg.fixed(np.array([[0.7]])); lfo.phase = cfg.fixed(p['phase'])
        swing = fx.Gain(); swing.left = lfo; swing.right = cfg.fixed(np.array([[0.0015]]))
        t = fx.Mix(); t.left = swing; t.right = cfg.fixed(np.array([[0.0015]])); t.mix = cfg.fixed(np.array([[0.5]]))
        wet = ext.Delay(); wet.input = dry; wet.time = t
    else:
        wet = osc.Sawtooth()                                                   # a second oscillator in the Delay's place
        wet.hertz = cfg.fixed(p['hertz'] * 1.003); wet.phase = cfg.fixed(p['phase'])
    mix = fx.Mix(); mix.left = dry; mix.right = wet; mix.mix = cfg.fixed(np.array([[0.5]]))
    b = ext.SumBus(); b.input = mix; b.get_state().gains = np.ascontiguousarray(p['pan'])
    return b


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
    d.input = build()
    loc = lambda b: BlockLoc(position=b * N, rate=RATE, shape=Shape(frames=N, channels=2))
    for b in range(4):
        d.input.request(loc(b))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(4, 4 + blocks):
        d.input.request(loc(b))
    torch.cuda.synchronize()
    return V * N * blocks / (time.perf_counter() - t0) / 1e12


def batched(build, V, N, K, steps, **kw):
    from signals_amd.engine import BatchRenderer, KernelTimer
    timer = KernelTimer(sample_every=4)
    r = BatchRenderer(build(), 2, RATE, timer=timer, **kw)
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


def median_us(launch, warm=5, reps=11, burst=10):
    """the median over `reps` bursts of `burst` launches queued back to back, per launch (tools/time_shaper.py has the reasons)"""
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(burst):
            launch()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / burst)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def kernel_rates(V=1024, N=256, K=1024):
    """sig_delay_taps alone, float32 in and out, next to elementwise[Gain] on the same shape in the same session (8 B per
    voice-sample both; the delay line's tiles re-read 100 rows of halo per 220, not counted)"""
    from signals_amd import _native
    rng = np.random.default_rng(0)
    d = lambda a, dt=torch.float64: torch.from_numpy(np.array(a)).to('cuda:0', dt)
    rows = N * K
    window = d(rng.uniform(-1.0, 1.0, (100 + rows, V)), torch.float32)
    x = window[100:]
    gain = d(rng.uniform(0.2, 1.0, (1, V)))
    out = torch.empty((rows, V), dtype=torch.float32, device='cuda:0')

    def line(name, stats, **more):
        us, lo, hi = stats
        return dict({'kernel': name, 'voice_samples': V * rows, 'us': round(us, 1), 'us_min': round(lo, 1), 'us_max': round(hi, 1),
                     'hbm_TB_per_s': round(8.0 * rows * V / us / 1e6, 2),
                     'of_8_TB_per_s_roof': round(8.0 * rows * V / (us * 1e-6) / HBM_ROOF, 3)}, **more)
    ew = {burst: median_us(lambda: _native.elementwise('Gain', x, gain, None, out), burst=burst) for burst in (10, 1)}
    for burst in (10, 1):
        yield line('sig_elementwise[Gain]', ew[burst], launches_per_sync=burst)
    for U in (1, 4):
        taps = np.stack([np.linspace(1.0, 0.25, U), np.full(U, 1.0 / U)], axis=1)
        for what, t in (('one row', d(rng.uniform(0, 0.002, (1, V)))), ('per block', d(rng.uniform(0, 0.002, (K, V))))):
            for burst in (10, 1):
                stats = median_us(lambda: _native.delay_taps(RATE, 4096, N, K, window, 100, t, taps, out), burst=burst)
                yield line(f'sig_delay_taps[U={U}]', stats, time=what, launches_per_sync=burst, of_gain_kernel=round(ew[burst][0] / stats[0], 3))


if __name__ == '__main__':
    from signals_amd import runtime
    runtime.set_device('cuda:0')
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    V = 1024
    for line in kernel_rates(V, N, K):
        print(json.dumps(line), flush=True)
    for name, delayed in (('flanger_voice', True), ('voice_without_delay', False)):
        eager_T = eager(lambda: voice(V, delayed), V, N, 64)
        node_T, node = batched(lambda: voice(V, delayed), V, N, K, 6, fuse=False)
        dflt_T, dflt = batched(lambda: voice(V, delayed), V, N, K, 6)
        print(json.dumps({'shape': name, 'voices': V, 'block_frames': N, 'blocks_per_batch': K, 'eager_T': round(eager_T, 4),
                          'per_node_T': round(node_T, 3), 'per_node_launches_us': node,
                          'default_T': round(dflt_T, 3), 'default_launches_us': dflt}), flush=True)
