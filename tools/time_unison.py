#!/usr/bin/env python3
"""Throughput of a supersaw voice -- (i) SumBus(UnisonSawtooth), seven copies, and (ii) the same oscillator behind a LowPass, 1024
voices, stereo bus, 48 kHz -- five ways: the eager pull path block by block, one kernel per node (fuse=False), the voice-program
interpreter, the voice program specialised for the graph, the engine's default route; and next to them what the graph had to be
before the node existed: seven osc.Sawtooth nodes and six Mix nodes per voice (13 kernels through HBM, more oscillators and
temporaries than a voice program has slots), on the engine's default route.  Its copies sit at fixed detunes with equal weights
(Mix at 1/2, 2/3, 3/4 ... gives the mean), so it is the same sound at spread = 1.  Then the per-node kernel sig_osc_bank_unison
alone at U = 1, 7, 16 against osc_bank_kernel[Sawtooth].  Prints one JSON object per shape and one per kernel.

    python tools/time_unison.py [blocks per batch] [block frames]        (needs a GPU)
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


def voice(V, filtered, by_hand=False):
    from signals_amd.chain import ext, fx, osc
    p = cfg.c2_params(V)
    if by_hand:
        # the mean of seven detuned saws out of binary Mix nodes: m_k = k / (k + 1) keeps the running mean
        copies = ext.UnisonSawtooth().get_state().copies
        top = None
        for k, (d, off) in enumerate(copies.tolist()):
            o = osc.Sawtooth(); o.hertz = cfg.fixed(p['hertz'] * (1.0 + d)); o.phase = cfg.fixed(p['phase'] + off)
            if top is None:
                top = o
            else:
                m = fx.Mix(); m.left = top; m.right = o; m.mix = cfg.fixed(np.array([[k / (k + 1.0)]]))
                top = m
    else:
        top = ext.UnisonSawtooth()
        top.hertz = cfg.fixed(p['hertz']); top.phase = cfg.fixed(p['phase']); top.spread = cfg.fixed(np.ones((1, 1)))
    if filtered:
        f = fx.LowPass(); f.input = top; f.cutoff = cfg.fixed(p['cutoff'])
        top = f
    b = ext.SumBus(); b.input = top; b.get_state().gains = np.ascontiguousarray(p['pan'])
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
    that is kept busy, as the engine's are"""
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


def kernel_rates(V=1024, rows=65536):
    """sig_osc_bank_unison alone, float32 out, next to osc_bank_kernel of the same kind in the same session"""
    from signals_amd import _native
    rng = np.random.default_rng(0)
    d = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0', dt)
    hz, ph, sp = d(rng.uniform(55, 1760, (1, V))), d(rng.uniform(0, 1, (1, V))), d(rng.uniform(0, 1, (1, V)))
    out = torch.empty((rows, V), dtype=torch.float32, device='cuda:0')
    line = lambda name, us, **more: dict({'kernel': name, 'voice_samples': V * rows, 'us': round(us, 1),
                                          'hbm_TB_per_s': round(4.0 * rows * V / us / 1e6, 2),
                                          'of_8_TB_per_s_roof': round(4.0 * rows * V / (us * 1e-6) / HBM_ROOF, 3)}, **more)
    for kind in ('Sawtooth', 'Sine'):
        plain = median_us(lambda: _native.osc_bank(kind, 0, RATE, hz, ph, out))
        yield line(f'sig_osc_bank[{kind}]', plain)
        for U in (1, 7, 16):
            copies = np.stack([rng.uniform(-0.12, 0.12, U), rng.uniform(0, 1, U)], axis=1)
            us = median_us(lambda: _native.osc_bank_unison(kind, 0, RATE, hz, ph, sp, copies, out))
            yield line(f'sig_osc_bank_unison[{kind},U={U}]', us, copy_samples_per_s_T=round(U * V * rows / us / 1e6, 3),
                       of_plain_kernel=round(plain / us, 3))


if __name__ == '__main__':
    from signals_amd import runtime, specialise
    runtime.set_device('cuda:0')
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    V = 1024
    for name, filtered in (('supersaw_voice', False), ('supersaw_voice_lowpass', True)):
        eager_T = eager(lambda: voice(V, filtered), V, N, 64)
        node_T, node = batched(lambda: voice(V, filtered), V, N, K, 4, fuse=False)
        prog_T, prog = batched(lambda: voice(V, filtered), V, N, K, 10, fuse_program='always')
        spec_T, spec = batched(lambda: voice(V, filtered), V, N, K, 10, fuse_program='always', specialise=True) if specialise.hipcc() else (None, {})
        dflt_T, dflt = batched(lambda: voice(V, filtered), V, N, K, 10)
        hand_T, hand = batched(lambda: voice(V, filtered, by_hand=True), V, N, K, 4)
        print(json.dumps({'shape': name, 'voices': V, 'copies': 7, 'block_frames': N, 'blocks_per_batch': K, 'eager_T': round(eager_T, 4),
                          'per_node_T': round(node_T, 3), 'per_node_launches_us': node,
                          'interpreter_T': round(prog_T, 3), 'interpreter_launches_us': prog,
                          'specialised_T': spec_T and round(spec_T, 3), 'specialised_launches_us': spec,
                          'default_T': round(dflt_T, 3), 'default_launches_us': dflt,
                          'seven_saws_six_mixes_T': round(hand_T, 3), 'seven_saws_six_mixes_launches_us': hand}), flush=True)
    for line in kernel_rates():
        print(json.dumps(line), flush=True)
