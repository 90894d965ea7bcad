#!/usr/bin/env python3
"""Timing of the additive oscillator.  (i) sig_osc_bank_additive alone -- 1024 voices, blocks of 256 frames, float32 out (4 B per
voice-sample), H = 1, 8, 32, 64 partials of a sawtooth spectrum at pitches low enough that every partial is kept -- next to
sig_osc_bank_table and elementwise[Gain] on the same shape in the same session, as microseconds, as a fraction of the 8 TB/s HBM
roof and as a fraction of the float64 vector rate at 5 H operations per voice-sample: the kernel's counted operations per
partial-sample are the accumulation's fma and the rotation's two multiplies and two fmas, an fma counted as ONE operation, so the
figure is a fraction of the instruction rate; the sine / cosine pair per sample and the weight per voice and partial are not
counted.  (ii) the saw voice under a stereo bus, SumBus(Gain(Additive[sawtooth(64)])): one kernel per node in the batched engine,
with the per-launch figures, against the eager pull path block by block.  Prints one JSON object per kernel line and one per shape.

    python tools/time_additive.py [blocks per batch] [block frames]        (needs a GPU)
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
F64_VECTOR_OPS = 256 * 4 * 16 * 2.4e9          # 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz: one f64 multiply, add or fma per lane and clock
OPS_PER_PARTIAL = 5


def voice(V, H=64):
    from signals_amd.chain import ext, fx
    p = cfg.c2_params(V)
    a = ext.Additive(); a.get_state().table = ext.Additive.sawtooth(H)
    a.hertz = cfg.fixed(p['hertz']); a.phase = cfg.fixed(p['phase'])
    g = fx.Gain(); g.left = a; g.right = cfg.fixed(p['gain'])
    bus = ext.SumBus(); bus.input = g; bus.get_state().gains = np.ascontiguousarray(p['pan'])
    return bus


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


def median_us(launch, warm=3, reps=7, burst=4):
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
    """sig_osc_bank_additive alone, float32 out, next to sig_osc_bank_table and elementwise[Gain] on the same shape in the same session"""
    from signals_amd import _native
    from signals_amd.chain.ext import Additive
    rng = np.random.default_rng(0)
    d = lambda a, dt=torch.float64: torch.from_numpy(np.array(a)).to('cuda:0', dt)
    rows = N * K
    hertz = d(rng.uniform(55.0, 0.98 * RATE / 2 / 65, (1, V)))                # below rate / (2 * 65): k = H for every H timed
    phase = d(rng.uniform(0, 1, (1, V)))
    gain = d(rng.uniform(0.2, 1.0, (1, V)))
    out = torch.empty((rows, V), dtype=torch.float32, device='cuda:0')
    x = torch.empty((rows, V), dtype=torch.float32, device='cuda:0').uniform_(-1, 1)

    def line(name, stats, bytes_per=4.0, ops=0, **more):
        us, lo, hi = stats
        return dict({'kernel': name, 'voice_samples': V * rows, 'us': round(us, 1), 'us_min': round(lo, 1), 'us_max': round(hi, 1),
                     'of_8_TB_per_s_roof': round(bytes_per * rows * V / (us * 1e-6) / HBM_ROOF, 3),
                     'f64_ops_per_voice_sample': ops,
                     'of_f64_vector_rate': round(ops * rows * V / (us * 1e-6) / F64_VECTOR_OPS, 3)}, **more)
    ew = median_us(lambda: _native.elementwise('Gain', x, gain, None, out))
    yield line('sig_elementwise[Gain]', ew, bytes_per=8.0, ops=1)
    wavetable = d(Additive.cycle(Additive.sawtooth(16), 2048), torch.float32)
    wt = median_us(lambda: _native.osc_bank_table(0, RATE, hertz, phase, None, wavetable, out))
    yield line('sig_osc_bank_table[T=2048]', wt, of_gain_kernel=round(ew[0] / wt[0], 3))
    for H in (1, 8, 32, 64):
        tab = d(Additive.sawtooth(H), torch.float32)
        stats = median_us(lambda: _native.osc_bank_additive(0, RATE, hertz, phase, None, tab, out))
        yield line(f'sig_osc_bank_additive[H={H}]', stats, ops=OPS_PER_PARTIAL * H, of_gain_kernel=round(ew[0] / stats[0], 3),
                   of_table_kernel=round(wt[0] / stats[0], 3))
    # a pitch spread up to Nyquist: the lanes of a wave hold different k, the loop runs to the wave's largest
    wide = d(rng.uniform(55.0, RATE / 2, (1, V)))
    kept = float(np.mean(np.clip(np.ceil(RATE / 2 / wide.cpu().numpy()) - 1, 0, 64)))
    tab = d(Additive.sawtooth(64), torch.float32)
    stats = median_us(lambda: _native.osc_bank_additive(0, RATE, wide, phase, None, tab, out))
    yield line('sig_osc_bank_additive[H=64,55 Hz..Nyquist]', stats, ops=round(OPS_PER_PARTIAL * kept, 1), mean_partials_kept=round(kept, 2))


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
    print(json.dumps({'shape': 'additive_saw_voice', 'voices': V, 'block_frames': N, 'blocks_per_batch': K, 'eager_T': round(eager_T, 4),
                      'per_node_T': round(node_T, 3), 'per_node_launches_us': node,
                      'default_T': round(dflt_T, 3), 'default_launches_us': dflt}), flush=True)
