#!/usr/bin/env python3
"""Timing of the dense FIR filter.  (i) sig_fir_taps alone -- 1024 voices, blocks of 256 frames, float32 in and out (8 B per
voice-sample), L = 1, 17, 51, 101 taps, one column -- next to sig_delay_taps (U = 1) and elementwise[Gain] on the same shape in the
same session, as microseconds, as a fraction of the 8 TB/s HBM roof at 8 B per voice-sample and as a fraction of the float64 vector
rate at 2 L - 1 operations per voice-sample (a multiply and an add are one operation each: the sum is not fused).  (ii) the
frequency-shifter voice under a stereo bus, SumBus(Mix(RingMod(Delay(Saw, 50 frames), cos), RingMod(FIR_hilbert(Saw), -sin))): one
kernel per node in the batched engine, with the per-launch figures, against the eager pull path block by block.  Prints one JSON
object per kernel line and one per shape.

    python tools/time_fir.py [blocks per batch] [block frames]        (needs a GPU)
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
F64_VECTOR_OPS = 256 * 4 * 16 * 2.4e9          # 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz: one f64 multiply or add per lane and clock


def voice(V, shift_hz=5.0):
    from signals_amd.chain import ext, fx, osc
    p = cfg.c2_params(V)
    one = lambda v: cfg.fixed(np.array([[v]]))
    x = osc.Sawtooth()
    x.hertz = cfg.fixed(p['hertz']); x.phase = cfg.fixed(p['phase'])
    d = ext.Delay(); d.input = x; d.time = one(50.0 / RATE)
    h = ext.FIR(); h.get_state().taps = ext.FIR.hilbert(); h.input = x
    cos = osc.Sine(); cos.hertz = one(shift_hz); cos.phase = one(0.25)
    msin = osc.Sine(); msin.hertz = one(shift_hz); msin.phase = one(0.5)
    a = fx.RingMod(); a.left = d; a.right = cos
    b = fx.RingMod(); b.left = h; b.right = msin
    mix = fx.Mix(); mix.left = a; mix.right = b; mix.mix = one(0.5)
    bus = ext.SumBus(); bus.input = mix; bus.get_state().gains = np.ascontiguousarray(p['pan'])
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
    """sig_fir_taps alone, float32 in and out, next to sig_delay_taps (U = 1) and elementwise[Gain] on the same shape in the same session
    (8 B per voice-sample each; the tiles' re-read of 100 rows of halo is not counted)"""
    from signals_amd import _native
    from signals_amd.chain.ext import FIR
    rng = np.random.default_rng(0)
    d = lambda a, dt=torch.float64: torch.from_numpy(np.array(a)).to('cuda:0', dt)
    rows = N * K
    window = d(rng.uniform(-1.0, 1.0, (100 + rows, V)), torch.float32)
    x = window[100:]
    gain = d(rng.uniform(0.2, 1.0, (1, V)))
    out = torch.empty((rows, V), dtype=torch.float32, device='cuda:0')

    def line(name, stats, ops=0, **more):
        us, lo, hi = stats
        return dict({'kernel': name, 'voice_samples': V * rows, 'us': round(us, 1), 'us_min': round(lo, 1), 'us_max': round(hi, 1),
                     'of_8_TB_per_s_roof': round(8.0 * rows * V / (us * 1e-6) / HBM_ROOF, 3),
                     'f64_ops_per_voice_sample': ops,
                     'of_f64_vector_rate': round(ops * rows * V / (us * 1e-6) / F64_VECTOR_OPS, 3)}, **more)
    ew = median_us(lambda: _native.elementwise('Gain', x, gain, None, out))
    yield line('sig_elementwise[Gain]', ew, ops=1)
    t = d(rng.uniform(0, 0.002, (1, V)))
    one = np.array([[1.0, 1.0]])
    dl = median_us(lambda: _native.delay_taps(RATE, 4096, N, K, window, 100, t, one, out))
    yield line('sig_delay_taps[U=1]', dl, ops=4, of_gain_kernel=round(ew[0] / dl[0], 3))
    for L in (1, 17, 51, 101):
        h = np.array([[1.0]]) if L == 1 else FIR.lowpass(3000.0, RATE, taps=L)
        tab = d(h)
        stats = median_us(lambda: _native.fir_taps(RATE, 4096, N, K, window, 100, None, tab, out))
        yield line(f'sig_fir_taps[L={L}]', stats, ops=2 * L - 1, of_gain_kernel=round(ew[0] / stats[0], 3),
                   of_delay_kernel=round(dl[0] / stats[0], 3))
    bank = d(np.hstack([FIR.lowpass(3000.0, RATE), FIR.highpass(500.0, RATE), FIR.bandpass(800.0, 4000.0, RATE)]))
    sel = d(rng.uniform(0, 3, (K, V)))
    stats = median_us(lambda: _native.fir_taps(RATE, 4096, N, K, window, 100, sel, bank, out))
    yield line('sig_fir_taps[L=101,W=3,per-block]', stats, ops=201, of_gain_kernel=round(ew[0] / stats[0], 3))


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
    print(json.dumps({'shape': 'frequency_shifter_voice', 'voices': V, 'block_frames': N, 'blocks_per_batch': K, 'eager_T': round(eager_T, 4),
                      'per_node_T': round(node_T, 3), 'per_node_launches_us': node,
                      'default_T': round(dflt_T, 3), 'default_launches_us': dflt}), flush=True)
