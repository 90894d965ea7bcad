#!/usr/bin/env python3
"""Timing of the sample-playback node.  (i) sig_sampler_play alone -- 1024 voices, 1024 blocks of 256 frames, float32 out -- at ratios
0.5, 1 and 2, with every voice on its own column of a 64-column table (voice v reads column v mod 64) and with all voices on one
column at staggered offsets, next to osc_bank_table and elementwise[Gain] on the same shape in the same session.  The achieved bytes
per second are counted at 4 + 4 * max(ratio, 1/32) bytes per voice-sample (the store, and the table's 128-byte lines at the rate a
voice walks through them) against the 8 TB/s HBM roof; elementwise[Gain] moves 8 and osc_bank_table 4.  (ii) the chord voice of
scripts/example_sampler.py under a stereo bus, SumBus(RingMod(Sampler, ADSR)): the batched engine against the eager pull path.
Prints one JSON object per kernel line and one per shape.

    python tools/time_sampler.py [blocks per batch] [block frames]        (needs a GPU)
"""
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'scripts'))
import numpy as np
import torch

from time_delay import HBM_ROOF, RATE, batched, eager, median_us


def kernel_rates(V=1024, N=256, K=1024, T=1 << 18, W=64):
    """sig_sampler_play alone, float32 out, looped over the whole table so that every voice reads for the whole launch"""
    from signals_amd import _native
    rng = np.random.default_rng(0)
    d = lambda a, dt=torch.float64: torch.from_numpy(np.array(a)).to('cuda:0', dt)
    rows = N * K
    table = d(rng.uniform(-1.0, 1.0, (W, T)), torch.float32)                   # the device layout: every recording contiguous
    out = torch.empty((rows, V), dtype=torch.float32, device='cuda:0')
    x = d(rng.uniform(-1.0, 1.0, (rows, V)), torch.float32)
    gain = d(rng.uniform(0.2, 1.0, (1, V)))
    hertz, phase = d(rng.uniform(55.0, 1760.0, (1, V))), d(rng.uniform(0, 1, (1, V)))
    wavetable = d(rng.uniform(-1.0, 1.0, (2048, 8)), torch.float32)
    wsel = d(rng.uniform(0, 8, (1, V)))

    def line(name, stats, bytes_per_sample, **more):
        us, lo, hi = stats
        moved = bytes_per_sample * rows * V
        return dict({'kernel': name, 'voice_samples': V * rows, 'us': round(us, 1), 'us_min': round(lo, 1), 'us_max': round(hi, 1),
                     'bytes_per_voice_sample': round(bytes_per_sample, 3), 'hbm_TB_per_s': round(moved / us / 1e6, 2),
                     'of_8_TB_per_s_roof': round(moved / (us * 1e-6) / HBM_ROOF, 3)}, **more)
    yield line('sig_elementwise[Gain]', median_us(lambda: _native.elementwise('Gain', x, gain, None, out)), 8.0)
    yield line('sig_osc_bank_table', median_us(lambda: _native.osc_bank_table(0, RATE, hertz, phase, wsel, wavetable, out)), 4.0)
    del x
    gate = d(np.zeros((1, 1)))
    for ratio in (0.5, 1.0, 2.0):
        r = d(np.full((1, V), ratio))
        for what, select, offset in (('own column', d((np.arange(V) % W)[None, :].astype(float)), d(np.zeros((1, V)))),
                                     ('one column, staggered', d(np.zeros((1, V))), d((np.arange(V) * (T // V) + 0.25)[None, :]))):
            for loop, bounds in (('loop', (0, T)), ('one shot', (0, 0))):
                stats = median_us(lambda: _native.sampler_play(0, RATE, r, offset, gate, select, table, *bounds, out))
                yield line('sig_sampler_play', stats, 4.0 + 4.0 * max(ratio, 1.0 / 32.0), ratio=ratio, voices_read=what, mode=loop,
                           table=f'{T}x{W}')
        per_block = d(np.full((K, V), ratio))
        stats = median_us(lambda: _native.sampler_play(0, RATE, per_block, None, gate, None, table, 0, T, out, rows_per_param=N))
        yield line('sig_sampler_play', stats, 4.0 + 4.0 * max(ratio, 1.0 / 32.0), ratio=ratio, voices_read='one column, per-block ratio rows',
                   mode='loop', table=f'{T}x{W}')


if __name__ == '__main__':
    from signals_amd import runtime
    runtime.set_device('cuda:0')
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    V = 1024
    for line in kernel_rates(V, N, K):
        print(json.dumps(line), flush=True)
    import example_sampler
    table = example_sampler.recording()
    for name, loop in (('chord_voice', False), ('chord_voice_looped', True)):
        build = lambda: example_sampler.chord(V, table, loop)[0]
        eager_T = eager(build, V, N, 64)
        node_T, node = batched(build, V, N, K, 6, fuse=False)
        dflt_T, dflt = batched(build, V, N, K, 6)
        print(json.dumps({'shape': name, 'voices': V, 'block_frames': N, 'blocks_per_batch': K, 'eager_T': round(eager_T, 4),
                          'per_node_T': round(node_T, 3), 'per_node_launches_us': node,
                          'default_T': round(dflt_T, 3), 'default_launches_us': dflt}), flush=True)
