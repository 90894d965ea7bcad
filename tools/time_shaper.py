#!/usr/bin/env python3
"""Throughput of a waveshaped voice -- (i) SumBus(Gain(Shaper(Sawtooth))) and (ii) the same shaper behind a LowPass, 1024 voices,
stereo bus, 48 kHz, a 513-point tanh(3x)/tanh(3) curve -- five ways: the eager pull path block by block, one kernel per node
(fuse=False), the voice-program interpreter, the voice program specialised for the graph, and the engine's default route.  Then the
per-node kernel sig_shaper_table alone (float32 in and out, 8 B per voice-sample) against elementwise[Gain] on the same shape (the
same 8 B per voice-sample) and the 8 TB/s HBM roof.  Prints one JSON object per shape and one per kernel.

    python tools/time_shaper.py [blocks per batch] [block frames]        (needs a GPU)
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


def tanh_table(points=513, drive=3.0, curves=1):
    one = (np.tanh(drive * np.linspace(-1.0, 1.0, points)) / np.tanh(drive))[:, None]
    return np.repeat(one, curves, axis=1)


def voice(V, filtered):
    from signals_amd.chain import ext, fx, osc
    p = cfg.c2_params(V)
    o = osc.Sawtooth()
    o.hertz = cfg.fixed(p['hertz']); o.phase = cfg.fixed(p['phase'])
    top = o
    if filtered:
        top = fx.LowPass(); top.input = o; top.cutoff = cfg.fixed(p['cutoff'])
    s = ext.Shaper(); s.input = top
    s.get_state().table = tanh_table()
    g = fx.Gain(); g.left = s; g.right = cfg.fixed(p['gain'])
    b = ext.SumBus(); b.input = g; b.get_state().gains = np.ascontiguousarray(p['pan'])
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
    from signals_amd import _native
    from signals_amd.engine import BatchRenderer, KernelTimer
    _native.voice_program_use_attached(bool(kw.get('specialise')))
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
    """the median over `reps` bursts of `burst` launches queued back to back, per launch: what a launch costs inside a stream
    that is kept busy, as the engine's are (the per-kernel figures of `batched` are taken the same way); `burst` = 1 brackets
    single launches with a synchronisation between them, which adds the start-up of an idle queue to each"""
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
    return float(np.median(times))


def kernel_rates(V=1024, rows=262144):
    """sig_shaper_table alone, float32 in and out, next to elementwise[Gain] on the same shape in the same session (8 B per
    voice-sample both): queued bursts and single synchronised launches, `select` unplugged and a per-voice row"""
    from signals_amd import _native
    rng = np.random.default_rng(0)
    d = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0', dt)
    x = d(rng.uniform(-1.5, 1.5, (rows, V)), torch.float32)
    gain = d(rng.uniform(0.2, 1.0, (1, V)))
    out = torch.empty((rows, V), dtype=torch.float32, device='cuda:0')
    line = lambda name, us, **more: dict({'kernel': name, 'voice_samples': V * rows, 'us': round(us, 1),
                                          'hbm_TB_per_s': round(8.0 * rows * V / us / 1e6, 2),
                                          'of_8_TB_per_s_roof': round(8.0 * rows * V / (us * 1e-6) / HBM_ROOF, 3)}, **more)
    ew = {burst: median_us(lambda: _native.elementwise('Gain', x, gain, None, out), burst=burst) for burst in (10, 1)}
    for burst in (10, 1):
        yield line('sig_elementwise[Gain]', ew[burst], launches_per_sync=burst)
    for T, W in ((513, 1), (513, 3), (2049, 7)):
        tab = d(tanh_table(T, 3.0, W), torch.float32)
        for what, sel in (('unplugged', None), ('per voice', d(rng.uniform(0, W, (1, V))))):
            for burst in (10, 1):
                us = median_us(lambda: _native.shaper_table(x, sel, tab, out), burst=burst)
                yield line(f'sig_shaper_table[T={T},W={W}]', us, select=what, launches_per_sync=burst,
                           of_gain_kernel=round(ew[burst] / us, 3))


if __name__ == '__main__':
    from signals_amd import runtime, specialise
    runtime.set_device('cuda:0')
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    V = 1024
    for name, filtered in (('shaper_voice', False), ('shaper_voice_lowpass', True)):
        eager_T = eager(lambda: voice(V, filtered), V, N, 64)
        node_T, node = batched(lambda: voice(V, filtered), V, N, K, 4, fuse=False)
        prog_T, prog = batched(lambda: voice(V, filtered), V, N, K, 10, fuse_program='always')
        spec_T, spec = batched(lambda: voice(V, filtered), V, N, K, 10, fuse_program='always', specialise=True) if specialise.hipcc() else (None, {})
        dflt_T, dflt = batched(lambda: voice(V, filtered), V, N, K, 10)
        print(json.dumps({'shape': name, 'voices': V, 'block_frames': N, 'blocks_per_batch': K, 'eager_T': round(eager_T, 4),
                          'per_node_T': round(node_T, 3), 'per_node_launches_us': node,
                          'interpreter_T': round(prog_T, 3), 'interpreter_launches_us': prog,
                          'specialised_T': spec_T and round(spec_T, 3), 'specialised_launches_us': spec,
                          'default_T': round(dflt_T, 3), 'default_launches_us': dflt}), flush=True)
    for line in kernel_rates():
        print(json.dumps(line), flush=True)
