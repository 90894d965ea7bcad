#!/usr/bin/env python3
"""Throughput of a wavetable voice -- (i) SumBus(Gain(Wavetable)) and (ii) the same oscillator behind a LowPass, 1024 voices,
stereo bus, 48 kHz -- five ways: the eager pull path block by block, one kernel per node (fuse=False), the voice-program
interpreter, the voice program specialised for the graph, and the same voice with the closed-form osc.Sawtooth on the engine's
default route, so the table's cost over a closed-form oscillator is visible.  Then the per-node kernel sig_osc_bank_table alone
at (T, W) = (2048, 1) and (2048, 8) against osc_bank_kernel[Sawtooth] (both write the same 4 B per voice-sample) and the 8 TB/s
HBM roof.  Prints one JSON object per shape and one per kernel.

    python tools/time_wavetable.py [blocks per batch] [block frames]        (needs a GPU)
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


def saw_table(points=2048, harmonics=16, waves=1):
    k = np.arange(points)[:, None] / points
    h = np.arange(1, harmonics + 1)[None, :]
    one = 2.0 / np.pi * np.sum(np.sin(2.0 * np.pi * k * h) / h * (-1.0) ** (h + 1), axis=1, keepdims=True)
    return np.repeat(one, waves, axis=1)


def voice(V, filtered, closed_form=False):
    from signals_amd.chain import ext, fx, osc
    p = cfg.c2_params(V)
    if closed_form:
        o = osc.Sawtooth()
    else:
        o = ext.Wavetable()
        o.get_state().table = saw_table()
    o.hertz = cfg.fixed(p['hertz']); o.phase = cfg.fixed(p['phase'])
    top = o
    if filtered:
        top = fx.LowPass(); top.input = o; top.cutoff = cfg.fixed(p['cutoff'])
    g = fx.Gain(); g.left = top; g.right = cfg.fixed(p['gain'])
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
    """sig_osc_bank_table alone, float32 out, next to osc_bank_kernel[Sawtooth] in the same session: queued bursts and single
    synchronised launches, `select` unplugged and a per-voice row"""
    from signals_amd import _native
    rng = np.random.default_rng(0)
    d = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0', dt)
    hz, ph = d(rng.uniform(55, 1760, (1, V))), d(rng.uniform(0, 1, (1, V)))
    out = torch.empty((rows, V), dtype=torch.float32, device='cuda:0')
    line = lambda name, us, **more: dict({'kernel': name, 'voice_samples': V * rows, 'us': round(us, 1),
                                          'hbm_TB_per_s': round(4.0 * rows * V / us / 1e6, 2),
                                          'of_8_TB_per_s_roof': round(4.0 * rows * V / (us * 1e-6) / HBM_ROOF, 3)}, **more)
    saw = {burst: median_us(lambda: _native.osc_bank('Sawtooth', 0, RATE, hz, ph, out), burst=burst) for burst in (10, 1)}
    for burst in (10, 1):
        yield line('sig_osc_bank[Sawtooth]', saw[burst], launches_per_sync=burst)
    for W in (1, 8):
        tab = d(saw_table(waves=W), torch.float32)
        for what, sel in (('unplugged', None), ('per voice', d(rng.uniform(0, W, (1, V))))):
            for burst in (10, 1):
                us = median_us(lambda: _native.osc_bank_table(0, RATE, hz, ph, sel, tab, out), burst=burst)
                yield line(f'sig_osc_bank_table[T=2048,W={W}]', us, select=what, launches_per_sync=burst,
                           of_sawtooth_kernel=round(saw[burst] / us, 3))


if __name__ == '__main__':
    from signals_amd import runtime, specialise
    runtime.set_device('cuda:0')
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    V = 1024
    for name, filtered in (('wavetable_voice', False), ('wavetable_voice_lowpass', True)):
        eager_T = eager(lambda: voice(V, filtered), V, N, 64)
        node_T, node = batched(lambda: voice(V, filtered), V, N, K, 4, fuse=False)
        prog_T, prog = batched(lambda: voice(V, filtered), V, N, K, 10, fuse_program='always')
        spec_T, spec = batched(lambda: voice(V, filtered), V, N, K, 10, fuse_program='always', specialise=True) if specialise.hipcc() else (None, {})
        dflt_T, dflt = batched(lambda: voice(V, filtered), V, N, K, 10)
        saw_T, saw = batched(lambda: voice(V, filtered, closed_form=True), V, N, K, 10)
        print(json.dumps({'shape': name, 'voices': V, 'block_frames': N, 'blocks_per_batch': K, 'eager_T': round(eager_T, 4),
                          'per_node_T': round(node_T, 3), 'per_node_launches_us': node,
                          'interpreter_T': round(prog_T, 3), 'interpreter_launches_us': prog,
                          'specialised_T': spec_T and round(spec_T, 3), 'specialised_launches_us': spec,
                          'default_T': round(dflt_T, 3), 'default_launches_us': dflt,
                          'sawtooth_default_T': round(saw_T, 3), 'sawtooth_default_launches_us': saw}), flush=True)
    for line in kernel_rates():
        print(json.dumps(line), flush=True)
