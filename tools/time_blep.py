#!/usr/bin/env python3
"""Throughput of the band-limited sawtooth next to what it replaces, 1024 voices under a stereo bus at 48 kHz, bare and behind a
LowPass, each on three routes (one kernel per node, the voice-program interpreter, the program specialised for the graph):

    BlepSawtooth, one copy        against osc.Sawtooth
    BlepSawtooth, seven copies    against UnisonSawtooth (the supersaw)
    Wavetable                     one band-limited saw column of 2048 points: the workaround before the node existed

Then the per-node kernel sig_osc_bank_blep alone, all three kinds at U = 1, 7, 16, against sig_osc_bank_unison of the same kind in
the same session, at musical pitches (55 .. 1760 Hz) and at low ones (27.5 .. 110 Hz, where a wave-uniform skip of the residual
has its best case).  Prints one JSON object per patch and one per kernel.  (batched, median_us: tools/time_unison.py's.)

    python tools/time_blep.py [blocks per batch] [block frames]        (needs a GPU)
    python tools/time_blep.py kernels                                  the kernel lines alone (a tuning build: SIG_LIB_PATH)
    python tools/time_blep.py repeat PATCH ROUNDS                      one patch's routes ROUNDS times, bare and behind the LowPass
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

PATCHES = ('osc.Sawtooth', 'BlepSawtooth[U=1]', 'UnisonSawtooth[U=7]', 'BlepSawtooth[U=7]', 'Wavetable[2048]')


def saw_table(points=2048, partials=20):
    """a sawtooth of `partials` harmonics: one mip column (clean up to rate / 2 / partials = 1.2 kHz; above it a user swaps columns)"""
    n = np.arange(points) / points
    k = np.arange(1, partials + 1)[None, :]
    return (-2.0 / np.pi * (np.sin(2 * np.pi * k * (n[:, None] + 0.5)) / k).sum(axis=1))[:, None]


def voice(which, V, filtered):
    from signals_amd.chain import ext, fx, osc
    p = cfg.c2_params(V)
    if which == 'osc.Sawtooth':
        top = osc.Sawtooth()
    elif which == 'Wavetable[2048]':
        top = ext.Wavetable(); top.get_state().table = saw_table()
    else:
        top = (ext.BlepSawtooth if which.startswith('Blep') else ext.UnisonSawtooth)()
        top.get_state().copies = ext.UnisonSawtooth().get_state().copies if which.endswith('[U=7]') else np.zeros((1, 2))
        top.spread = cfg.fixed(np.ones((1, 1)))
    top.hertz = cfg.fixed(p['hertz']); top.phase = cfg.fixed(p['phase'])
    if filtered:
        f = fx.LowPass(); f.input = top; f.cutoff = cfg.fixed(p['cutoff'])
        top = f
    b = ext.SumBus(); b.input = top; b.get_state().gains = np.ascontiguousarray(p['pan'])
    return b


def kernel_rates(V=1024, rows=65536, low=55.0, high=1760.0):
    """sig_osc_bank_blep alone, float32 out, next to sig_osc_bank_unison of the same kind and copies"""
    from signals_amd import _native
    rng = np.random.default_rng(0)
    d = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0', dt)
    hz, ph, sp = d(rng.uniform(low, high, (1, V))), d(rng.uniform(0, 1, (1, V))), d(rng.uniform(0, 1, (1, V)))
    out = torch.empty((rows, V), dtype=torch.float32, device='cuda:0')
    for kind in ('Sawtooth', 'Square', 'Triangle'):
        for U in (1, 7, 16):
            copies = np.stack([rng.uniform(-0.12, 0.12, U), rng.uniform(0, 1, U)], axis=1)
            naive = median_us(lambda: _native.osc_bank_unison(kind, 0, RATE, hz, ph, sp, copies, out))
            us = median_us(lambda: _native.osc_bank_blep(kind, 0, RATE, hz, ph, sp, copies, out))
            yield {'kernel': f'sig_osc_bank_blep[{kind},U={U}]', 'hertz': [low, high], 'voice_samples': V * rows, 'us': round(us, 1),
                   'sig_osc_bank_unison_us': round(naive, 1), 'of_unison_kernel': round(naive / us, 3),
                   'copy_samples_per_s_T': round(U * V * rows / us / 1e6, 3),
                   'of_8_TB_per_s_roof': round(4.0 * rows * V / (us * 1e-6) / HBM_ROOF, 3)}


if __name__ == '__main__':
    from signals_amd import runtime, specialise
    runtime.set_device('cuda:0')
    V = 1024
    def print_kernels():
        for low, high in ((55.0, 1760.0), (27.5, 110.0)):
            for line in kernel_rates(low=low, high=high):
                print(json.dumps(line), flush=True)
    if sys.argv[1:2] == ['kernels']:
        print_kernels()
        sys.exit(0)
    K = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1024
    N = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 256
    patches, rounds = (PATCHES, 1) if sys.argv[1:2] != ['repeat'] else ((sys.argv[2],), int(sys.argv[3]))
    for filtered in (False, True) * rounds:
        for which in patches:
            build = lambda: voice(which, V, filtered)
            node_T, node = batched(build, V, N, K, 4, fuse=False)
            prog_T, prog = batched(build, V, N, K, 10, fuse_program='always')
            spec_T, spec = batched(build, V, N, K, 10, fuse_program='always', specialise=True) if specialise.hipcc() else (None, {})
            dflt_T, dflt = batched(build, V, N, K, 10)
            print(json.dumps({'patch': which + (' -> LowPass' if filtered else ''), 'voices': V, 'block_frames': N, 'blocks_per_batch': K,
                              'per_node_T': round(node_T, 3), 'per_node_launches_us': node,
                              'interpreter_T': round(prog_T, 3), 'interpreter_launches_us': prog,
                              'specialised_T': spec_T and round(spec_T, 3), 'specialised_launches_us': spec,
                              'default_T': round(dflt_T, 3), 'default_launches_us': dflt}), flush=True)
    if rounds == 1:
        print_kernels()
