#!/usr/bin/env python3
"""Throughput of a two-operator phase-modulation voice -- (i) SumBus(Gain(PMSine(mod=Sine))) and (ii) the same carrier behind a
LowPass, 1024 voices, stereo bus, 48 kHz -- five ways: the carrier as a torch PLUGIN node pulled block by block (what a user could
do before ext.PMSine existed), one kernel per node (fuse=False), the voice-program interpreter, the voice program specialised
for the graph, and the per-node kernel sig_osc_bank_pm alone against the 8 TB/s HBM roof (4 B read + 4 B written per
voice-sample).  Prints one JSON object per shape and one for the kernel.

    python tools/time_pm.py [blocks per batch] [block frames]        (needs a GPU)
"""
import json
import math
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


def plugin_class():
    from signals_amd import SignalFlags
    from signals_amd.chain import BlockCachingEmitter, ImplicitChannels, port

    class TorchPM(BlockCachingEmitter, ImplicitChannels):
        """sin(2 pi (n / rate * hertz + phase + index * mod)) in eager torch: a class the engine has no schedule for"""
        hertz = port('hertz'); phase = port('phase'); index = port('index'); mod = port('mod')

        @classmethod
        def flags(cls):
            return super().flags() | SignalFlags.GENERATOR

        def _eval(self, request):
            loc = request.loc
            hz, ph, ix = (getattr(self, n).forward_at_block_rate(request).to(torch.float64) for n in ('hertz', 'phase', 'index'))
            m = self.mod.forward(request).to(torch.float64)
            n = torch.arange(loc.position, loc.position + loc.shape.frames, device=hz.device, dtype=torch.float64).reshape(-1, 1)
            return torch.sin((n / loc.rate * hz + ph + ix * m) * (2 * math.pi)).to(torch.float32)
    return TorchPM


def voice(V, filtered, plugin=False):
    from signals_amd.chain import ext, fx, osc
    p = cfg.c2_params(V)
    rng = np.random.default_rng(4)
    m = osc.Sine(); m.hertz = cfg.fixed(2.0 * p['hertz']); m.phase = cfg.fixed(rng.uniform(0, 1, (1, V)))
    c = (plugin_class() if plugin else ext.PMSine)()
    c.hertz = cfg.fixed(p['hertz']); c.phase = cfg.fixed(p['phase']); c.index = cfg.fixed(rng.uniform(0, 4, (1, V))); c.mod = m
    top = c
    if filtered:
        top = fx.LowPass(); top.input = c; top.cutoff = cfg.fixed(p['cutoff'])
    g = fx.Gain(); g.left = top; g.right = cfg.fixed(p['gain'])
    b = ext.SumBus(); b.input = g; b.get_state().gains = np.ascontiguousarray(p['pan'])
    return b


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


def kernel_rate(V, N, K, steps=20):
    """sig_osc_bank_pm alone: float32 modulator in, float32 out, event-timed"""
    from signals_amd import _native
    rng = np.random.default_rng(0)
    d = lambda a: torch.from_numpy(a).to('cuda:0')
    hz, ph, ix = d(rng.uniform(55, 1760, (1, V))), d(rng.uniform(0, 1, (1, V))), d(rng.uniform(0, 4, (1, V)))
    rows = N * K
    mod = torch.rand((rows, V), dtype=torch.float32, device='cuda:0') * 2 - 1
    out = torch.empty_like(mod)
    for _ in range(3):
        _native.osc_bank_pm('Sine', 0, RATE, hz, ph, ix, mod, out)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        _native.osc_bank_pm('Sine', 0, RATE, hz, ph, ix, mod, out)
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) / steps * 1e3
    rate = 8.0 * rows * V / (us * 1e-6)
    return us, rate


if __name__ == '__main__':
    from signals_amd import runtime, specialise
    runtime.set_device('cuda:0')
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    V = 1024
    for name, filtered in (('pm_voice', False), ('pm_voice_lowpass', True)):
        plug_T, plug = batched(lambda: voice(V, filtered, plugin=True), V, N, min(K, 64), 2)
        node_T, node = batched(lambda: voice(V, filtered), V, N, K, 4, fuse=False)
        prog_T, prog = batched(lambda: voice(V, filtered), V, N, K, 10, fuse_program='always')
        spec_T, spec = batched(lambda: voice(V, filtered), V, N, K, 10, fuse_program='always', specialise=True) if specialise.hipcc() else (None, {})
        print(json.dumps({'shape': name, 'voices': V, 'block_frames': N, 'blocks_per_batch': K,
                          'plugin_T': round(plug_T, 4), 'plugin_us_per_block': round(V * N / plug_T / 1e12 * 1e6, 1),
                          'per_node_T': round(node_T, 3), 'per_node_launches_us': node,
                          'interpreter_T': round(prog_T, 3), 'interpreter_launches_us': prog,
                          'specialised_T': spec_T and round(spec_T, 3), 'specialised_launches_us': spec}), flush=True)
    us, rate = kernel_rate(V, N, K)
    print(json.dumps({'kernel': 'sig_osc_bank_pm[Sine]', 'voice_samples': V * N * K, 'us': round(us, 1),
                      'hbm_TB_per_s': round(rate / 1e12, 2), 'of_8_TB_per_s_roof': round(rate / HBM_ROOF, 3)}), flush=True)
