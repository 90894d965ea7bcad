#!/usr/bin/env python3
"""Timing of the modal resonator bank.  (i) sig_modal_bank alone -- 1024 voices, blocks of 256 frames, float32 out (4 B per
voice-sample), M = 1, 8, 32, 64 modes of a plucked string at pitches low enough that every mode is kept, struck at frame 0 -- next to
sig_osc_bank_additive at the same partial counts and elementwise[Gain] on the same shape in the same session, as microseconds, as a
fraction of the 8 TB/s HBM roof and as a fraction of the float64 vector rate at 7 M operations per voice-sample: the kernel's counted
operations per mode and sample are the complex step's four multiplies and two additions and the sum's addition, none fused; the
closed-form start per mode and run of 64 rows (a divide, two exp, two sine / cosine pairs) is not counted.  (ii) a bar voice under a
stereo bus, SumBus(Modal[bar(8)]): one kernel per node in the batched engine, with the per-launch figures, against the eager pull path
block by block.  Prints one JSON object per kernel line and one per shape.

    python tools/time_modal.py [blocks per batch] [block frames]        (needs a GPU)
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
from time_additive import F64_VECTOR_OPS, HBM_ROOF, RATE, batched, eager, median_us

OPS_PER_MODE = 7
ADDITIVE_OPS_PER_PARTIAL = 5


def voice(V, M=8):
    from signals_amd.chain import ext
    p = cfg.c2_params(V)
    m = ext.Modal(); m.get_state().modes = ext.Modal.bar(M, 1.0)
    m.hertz = cfg.fixed(np.minimum(p['hertz'], 0.45 * RATE / ext.Modal.bar(M)[-1, 0]))
    m.gate_on = cfg.fixed(np.linspace(0.0, 0.05, V).reshape(1, V))
    bus = ext.SumBus(); bus.input = m; bus.get_state().gains = np.ascontiguousarray(p['pan'])
    return bus


def kernel_rates(V=1024, N=256, K=1024):
    """sig_modal_bank alone, float32 out, next to sig_osc_bank_additive and elementwise[Gain] on the same shape in the same session"""
    from signals_amd import _native
    from signals_amd.chain.ext import Additive, Modal
    rng = np.random.default_rng(0)
    d = lambda a, dt=torch.float64: torch.from_numpy(np.array(a)).to('cuda:0', dt)
    rows = N * K
    hertz = d(rng.uniform(55.0, 0.98 * RATE / 2 / 65, (1, V)))                # below rate / (2 * 65): every mode and partial kept
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
    for M in (1, 8, 32, 64):
        tab = d(Additive.sawtooth(M), torch.float32)
        add = median_us(lambda: _native.osc_bank_additive(0, RATE, hertz, phase, None, tab, out))
        yield line(f'sig_osc_bank_additive[H={M}]', add, ops=ADDITIVE_OPS_PER_PARTIAL * M)
        from signals_amd.chain.ext import _mode_rates
        modes = d(_mode_rates(Modal.string(M, 2.0)))
        stats = median_us(lambda: _native.modal_bank(0, RATE, hertz, None, None, None, modes, out))
        yield line(f'sig_modal_bank[M={M}]', stats, ops=OPS_PER_MODE * M, of_gain_kernel=round(ew[0] / stats[0], 3),
                   times_additive=round(stats[0] / add[0], 3))


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
    print(json.dumps({'shape': 'modal_bar_voice', 'voices': V, 'block_frames': N, 'blocks_per_batch': K, 'eager_T': round(eager_T, 4),
                      'per_node_T': round(node_T, 3), 'per_node_launches_us': node,
                      'default_T': round(dflt_T, 3), 'default_launches_us': dflt}), flush=True)
