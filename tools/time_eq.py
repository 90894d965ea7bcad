#!/usr/bin/env python3
"""Throughput of an equaliser voice -- Peaking(Sawtooth) by default, 1024 voices, 48 kHz, q dealt from {0.5, 1/sqrt2, 4} and gain from
{-12, 0, +12} dB -- (i) storing its rows and (ii) under a stereo SumBus, four ways: the eager pull path block by block, one kernel per
node (fuse=False), the voice-program interpreter (the RES+EQ kernels), and the voice program specialised for the graph.  The same voice
with ext.ResonantLowPass in place of the equaliser is timed in the same run, route by route and taking turns (tools/time_resonant.py's
method: the median of its REPEATS timed runs with the lowest and the highest), so that the general numerator's cost -- two taps more
per slot and chain, a third control -- can be read against the run's own spread.  Prints one JSON object per (shape, filter).

    python tools/time_eq.py [blocks per batch] [block frames] [Peaking | LowShelf | HighShelf | Notch | AllPass | ResonantBandPass]   (needs a GPU)
"""
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tools'))
import numpy as np

import bench_configs as cfg
import time_resonant as TR

QS, GAINS = (0.5, 2.0 ** -0.5, 4.0), (-12.0, 0.0, 12.0)


def voice(V, kind, bus):
    """`kind`: an ext.EqFilter class name, or None for the ResonantLowPass voice it is compared with"""
    from signals_amd.chain import ext, osc
    p = cfg.c2_params(V)
    o = osc.Sawtooth()
    o.hertz = cfg.fixed(p['hertz']); o.phase = cfg.fixed(p['phase'])
    f = getattr(ext, kind or 'ResonantLowPass')()
    f.resonance = cfg.fixed(np.array([QS[v % 3] for v in range(V)])[None, :])
    if getattr(f, 'gain_port', lambda: None)() is not None:
        f.gain = cfg.fixed(np.array([GAINS[(v // 3) % 3] for v in range(V)])[None, :])
    f.input = o; f.cutoff = cfg.fixed(p['cutoff'])
    if not bus:
        return f, V
    b = ext.SumBus(); b.input = f; b.get_state().gains = np.ascontiguousarray(p['pan'])
    return b, 2


if __name__ == '__main__':
    from signals_amd import runtime, specialise
    runtime.set_device('cuda:0')
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    kind = sys.argv[3] if len(sys.argv) > 3 else 'Peaking'
    V = 1024
    routes = [('per_node', {'fuse': False}), ('interpreter', {'fuse_program': 'always'})]
    if specialise.hipcc():
        routes.append(('specialised', {'fuse_program': 'always', 'specialise': True}))
    for bus in (False, True):
        builds = [lambda k=k: voice(V, k, bus) for k in (kind, None)]
        lines = [{'shape': 'voice_bus' if bus else 'voice', 'filter': name, 'voices': V, 'block_frames': N, 'blocks_per_batch': K,
                  'eager_T': round(TR.eager(build, V, N, 64), 4)} for name, build in zip((kind, 'ResonantLowPass'), builds)]
        for route, kw in routes:
            for line, (rates, launches) in zip(lines, TR.batched(builds, V, N, K, **kw)):
                line[route + '_T'], line[route + '_launches'] = rates, launches
        for line in lines:
            print(json.dumps(line), flush=True)
