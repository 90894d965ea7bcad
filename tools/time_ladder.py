#!/usr/bin/env python3
"""Timing of the 4-pole ladder filter.  (i) sig_ladder_coldstart alone -- 1024 voices, 1024 blocks of 256 frames, float32 in and out,
linear (drive unplugged: the kernel without tanh) and driven (a drive row > 0) -- next to sig_biquad_coldstart_q and elementwise[Gain]
on the same shape in the same session.  (ii) the voice SumBus(Ladder(Sawtooth)) under a stereo bus: one kernel per node in the batched
engine, with the per-launch figures, against the eager pull path block by block.  Prints one JSON object per kernel line and one for
the voice.

    python tools/time_ladder.py [blocks per batch] [block frames]        (needs a GPU)
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


def voice(V):
    from signals_amd.chain import ext, osc
    p = cfg.c2_params(V)
    saw = osc.Sawtooth()
    saw.hertz = cfg.fixed(p['hertz']); saw.phase = cfg.fixed(p['phase'])
    lad = ext.Ladder(); lad.input = saw; lad.cutoff = cfg.fixed(p['cutoff'])
    lad.resonance = cfg.fixed(np.full((1, V), 3.0)); lad.drive = cfg.fixed(np.full((1, V), 2.0))
    b = ext.SumBus(); b.input = lad; b.get_state().gains = np.ascontiguousarray(p['pan'])
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


def median_us(launch, warm=3, reps=9, burst=4):
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
    """the three kernels on one shape, float32 in and out (8 B per voice-sample each; the filters re-read 100 context rows per block,
    not counted).  The ladder's row loop is 26 float64 operations per voice-sample, 22 of them one dependent chain (the biquad's: 9 and 4), with drive a tanh more"""
    from signals_amd import _native
    rng = np.random.default_rng(0)
    d = lambda a, dt=torch.float64: torch.from_numpy(np.array(a)).to('cuda:0', dt)
    rows = N * K
    window = d(rng.uniform(-1.0, 1.0, (100 + rows, V)), torch.float32)
    x = window[100:]
    gain = d(rng.uniform(0.2, 1.0, (1, V)))
    cut, q = d(rng.uniform(200.0, 8000.0, (1, V))), d(rng.uniform(0.5, 8.0, (1, V)))
    k, drive = d(rng.uniform(0.0, 4.0, (1, V))), d(rng.uniform(0.5, 4.0, (1, V)))
    out = torch.empty((rows, V), dtype=torch.float32, device='cuda:0')

    def line(name, stats, **more):
        us, lo, hi = stats
        return dict({'kernel': name, 'voice_samples': V * rows, 'us': round(us, 1), 'us_min': round(lo, 1), 'us_max': round(hi, 1),
                     'G_voice_samples_per_s': round(V * rows / us / 1e3, 1), 'hbm_TB_per_s': round(8.0 * rows * V / us / 1e6, 2)}, **more)
    ew = median_us(lambda: _native.elementwise('Gain', x, gain, None, out))
    yield line('sig_elementwise[Gain]', ew)
    bq = median_us(lambda: _native.biquad_coldstart_q('lp', RATE, 4096, N, K, 100, cut, q, window, 100, out))
    yield line('sig_biquad_coldstart_q[lp]', bq)
    for name, drv in (('linear', None), ('driven', drive)):
        for poles in (4,):
            stats = median_us(lambda: _native.ladder_coldstart(RATE, 4096, N, K, 100, cut, k, drv, poles, window, 100, out))
            yield line(f'sig_ladder_coldstart[{name}]', stats, poles=poles, of_biquad_q=round(bq[0] / stats[0], 3), of_gain_kernel=round(ew[0] / stats[0], 3))


if __name__ == '__main__':
    from signals_amd import runtime
    runtime.set_device('cuda:0')
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    V = 1024
    for line in kernel_rates(V, N, K):
        print(json.dumps(line), flush=True)
    eager_T = eager(lambda: voice(V), V, N, 64)
    node_T, node = batched(lambda: voice(V), V, N, K, 6, fuse=False)
    dflt_T, dflt = batched(lambda: voice(V), V, N, K, 6)
    print(json.dumps({'shape': 'saw_ladder_bus', 'voices': V, 'block_frames': N, 'blocks_per_batch': K, 'eager_T': round(eager_T, 4),
                      'per_node_T': round(node_T, 3), 'per_node_launches_us': node,
                      'default_T': round(dflt_T, 3), 'default_launches_us': dflt}), flush=True)
