"""The scaffolding of the GPU test files, stated once: the device set-up behind every file's `_gpu` fixture, the host-array-to-
device copy, the loop over consecutive batches of one BatchRenderer, the block-rate LFO with its oracle twin, the 1e-6-of-full-scale
tolerance, and the two route tables most parity files share.  Needs torch with a GPU behind it; tests/helpers.py stays importable
without one."""
from collections import namedtuple

import numpy as np
import torch

from helpers import RATE, fix, maxerr, mkosc

# the engine's routes as BatchRenderer keywords: with the engine's own choice as a leg ...
ROUTES_WITH_DEFAULT = {'per_node': {'fuse': False}, 'default': {}, 'always': {'fuse_program': 'always'}, 'specialise': {'specialise': True}}
# ... and with the voice program forced on both of its legs
ROUTES_FORCED = {'per_node': {'fuse': False}, 'always': {'fuse_program': 'always'}, 'specialise': {'fuse_program': 'always', 'specialise': True}}

Rendered = namedtuple('Rendered', 'rows names renderer')


def gpu_ready(device='cuda:0'):
    """what every file's module-scoped `_gpu` fixture does before its tests run"""
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from signals_amd import _native, runtime
    runtime.set_device(device)
    _native.lib()      # fail loudly if the HIP library is missing


def dev(a, dtype=torch.float64, device='cuda:0'):
    """a host array on the device (through a contiguous copy: shared references are read-only); None stays None"""
    return None if a is None else torch.from_numpy(np.array(a, order='C')).to(device, dtype)


def render_batches(node, channels, position, N, ks, *, timer=None, names=False, check_status=False, **renderer_kw):
    """One BatchRenderer over consecutive batches of ks[0], ks[1], ... blocks of N frames from `position`: (.rows, the batches'
    rows concatenated; .names, the labels of the launches that rendered them, with `names`; .renderer).  `names` without a
    `timer` times the launches itself; the device is synchronised before the timer is read, and `check_status` then raises
    what a kernel left in the status word."""
    from signals_amd import runtime
    from signals_amd.engine import BatchRenderer, KernelTimer
    if names and timer is None:
        timer = KernelTimer()
    r = BatchRenderer(node, channels, RATE, timer=timer, **renderer_kw)
    parts, pos = [], position
    for k in ks:
        parts.append(r.render(pos, N, k).cpu().numpy())
        pos += N * k
    if names or check_status:
        torch.cuda.synchronize()
    if check_status:
        runtime.check_status()
    return Rendered(np.concatenate(parts), set(timer.summary()) if names else None, r)


def lfo(hz, depth, centre):
    """depth * sin + centre as Mix(Gain(Sine, 2 depth), 2 centre, 0.5): (GPU node, oracle node)"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    s = mkosc('Sine', [[hz]])
    g = fx.Gain(); g.left = s; g.right = fix(2.0 * np.asarray(depth))
    m = fx.Mix(); m.left = g; m.right = fix(2.0 * np.asarray(centre)); m.mix = fix([[0.5]])
    ref = R.Binary('Mix', R.Binary('Gain', R.Osc('Sine', R.Fixed([[hz]])), R.Fixed(2.0 * np.asarray(depth))),
                   R.Fixed(2.0 * np.asarray(centre)), R.Fixed([[0.5]]))
    return m, ref


def tolerance(want, rel=1e-6):
    """`rel` of full scale, never below `rel` itself: a float32 output of |x| < 1 is compared absolutely"""
    return rel * max(1.0, float(np.abs(want).max()))


def close(got, ref, what, rel=1e-6):
    scale = max(1.0, float(np.max(np.abs(ref))))
    err = maxerr(got, ref)
    assert err <= rel * scale, (what, err, scale)
