#!/usr/bin/env python3
"""Throughput of the hard-sync sawtooth next to the band-limited one it sits on, 1024 voices under a stereo bus at 48 kHz, bare and
behind a LowPass, each on three routes (one kernel per node, the voice-program interpreter, the program specialised for the graph):

    BlepSawtooth, one copy                       the yardstick
    SyncSawtooth, one copy, ratio unplugged      what the sync handler costs at R = 1
    SyncSawtooth, one copy, ratio 2.75
    SyncSawtooth, seven copies, ratio 2.75

and SyncSawtooth -> ResonantLowPass with mixed_programs=True (one mixed launch) against one kernel per node.  Then the per-node kernel
sig_osc_bank_sync alone, both kinds at U = 1 and 7, against sig_osc_bank_blep of the same kind in the same session.  Prints one JSON
object per patch and one per kernel.  (batched, median_us: tools/time_unison.py's.)

    python tools/time_sync.py [blocks per batch] [block frames]        (needs a GPU)
    python tools/time_sync.py kernels                                  the kernel lines alone
"""
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tools'))
import numpy as np
import torch

import bench_configs as cfg
from time_unison import HBM_ROOF, RATE, batched, median_us

PATCHES = ('BlepSawtooth[U=1]', 'SyncSawtooth[U=1,unplugged]', 'SyncSawtooth[U=1,ratio=2.75]', 'SyncSawtooth[U=7,ratio=2.75]')


def voice(which, V, tail):
    """`tail`: None (bare), 'lowpass' or 'resonant'"""
    from signals_amd.chain import ext, fx
    p = cfg.c2_params(V)
    top = (ext.SyncSawtooth if which.startswith('Sync') else ext.BlepSawtooth)()
    top.get_state().copies = ext.UnisonSawtooth().get_state().copies if 'U=7' in which else np.zeros((1, 2))
    top.spread = cfg.fixed(np.ones((1, 1)))
    top.hertz = cfg.fixed(p['hertz']); top.phase = cfg.fixed(p['phase'])
    if 'ratio=' in which:
        top.ratio = cfg.fixed(np.full((1, 1), float(which.split('ratio=')[1].rstrip(']'))))
    if tail == 'lowpass':
        f = fx.LowPass(); f.input = top; f.cutoff = cfg.fixed(p['cutoff'])
        top = f
    elif tail == 'resonant':
        f = ext.ResonantLowPass(); f.input = top; f.cutoff = cfg.fixed(p['cutoff']); f.resonance = cfg.fixed(np.full((1, 1), 2.0))
        top = f
    b = ext.SumBus(); b.input = top; b.get_state().gains = np.ascontiguousarray(p['pan'])
    return b


def kernel_rates(V=1024, rows=65536, low=55.0, high=1760.0):
    """sig_osc_bank_sync alone, float32 out, next to sig_osc_bank_blep of the same kind and copies"""
    from signals_amd import _native
    rng = np.random.default_rng(0)
    d = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0', dt)
    hz, ph, sp = d(rng.uniform(low, high, (1, V))), d(rng.uniform(0, 1, (1, V))), d(rng.uniform(0, 1, (1, V)))
    ra = d(rng.uniform(1.0, 4.0, (1, V)))
    out = torch.empty((rows, V), dtype=torch.float32, device='cuda:0')
    for kind in ('Sawtooth', 'Square'):
        for U in (1, 7):
            copies = np.stack([rng.uniform(-0.12, 0.12, U), rng.uniform(0, 1, U)], axis=1)
            blep = median_us(lambda: _native.osc_bank_blep(kind, 0, RATE, hz, ph, sp, copies, out))
            us = median_us(lambda: _native.osc_bank_sync(kind, 0, RATE, hz, ph, sp, ra, copies, out))
            yield {'kernel': f'sig_osc_bank_sync[{kind},U={U}]', 'hertz': [low, high], 'voice_samples': V * rows, 'us': round(us, 1),
                   'sig_osc_bank_blep_us': round(blep, 1), 'of_blep_kernel': round(blep / us, 3),
                   'copy_samples_per_s_T': round(U * V * rows / us / 1e6, 3),
                   'of_8_TB_per_s_roof': round(4.0 * rows * V / (us * 1e-6) / HBM_ROOF, 3)}


if __name__ == '__main__':
    from signals_amd import runtime, specialise
    runtime.set_device('cuda:0')
    V = 1024

    def print_kernels():
        for line in kernel_rates():
            print(json.dumps(line), flush=True)
    if sys.argv[1:2] == ['kernels']:
        print_kernels()
        sys.exit(0)
    K = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1024
    N = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 256
    for tail in (None, 'lowpass'):
        for which in PATCHES:
            build = lambda: voice(which, V, tail)
            node_T, node = batched(build, V, N, K, 4, fuse=False)
            prog_T, prog = batched(build, V, N, K, 10, fuse_program='always')
            spec_T, spec = batched(build, V, N, K, 10, fuse_program='always', specialise=True) if specialise.hipcc() else (None, {})
            print(json.dumps({'patch': which + (' -> LowPass' if tail else ''), 'voices': V, 'block_frames': N, 'blocks_per_batch': K,
                              'per_node_T': round(node_T, 3), 'per_node_launches_us': node,
                              'interpreter_T': round(prog_T, 3), 'interpreter_launches_us': prog,
                              'specialised_T': spec_T and round(spec_T, 3), 'specialised_launches_us': spec}), flush=True)
    build = lambda: voice('SyncSawtooth[U=1,ratio=2.75]', V, 'resonant')
    node_T, node = batched(build, V, N, K, 4, fuse=False)
    mix_T, mix = batched(build, V, N, K, 10, fuse_program='always', mixed_programs=True)
    print(json.dumps({'patch': 'SyncSawtooth[U=1,ratio=2.75] -> ResonantLowPass', 'voices': V, 'block_frames': N, 'blocks_per_batch': K,
                      'per_node_T': round(node_T, 3), 'per_node_launches_us': node,
                      'mixed_interpreter_T': round(mix_T, 3), 'mixed_interpreter_launches_us': mix}), flush=True)
    print_kernels()
