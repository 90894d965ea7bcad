"""Mixed voice programs on the GPU: the seven patches of tests/mixed_patches.py -- each combines two or three of the extension
families -- through BatchRenderer(mixed_programs=True) interpreted (fuse_program='always') and specialised, and with the option off,
against the oracle's render_stream; which kernels each route launched; the resonance status word; in-place edits of `copies` and of
a table between renders.

Geometry, the smallest at which the mixed kernel can go wrong: 70 voices (two waves at one voice per lane, the second partly dead,
odd: store alignment 1) and 128 voices at two voices per lane (forced through the tuning hook: the heuristic takes two only for
launches of 1024 waves and more); blocks of 256 frames as batches of 3 and 2 (history across two launches) and of 64 frames (every
patch has one filter in series: the `small` mode, blocks shorter than the 100-frame context); positions 0 and one hour.  Tables:
T = 64, W = 2 with a per-voice select.  Copies: the default seven, and three.  Controls: supersaw_bus and wah follow block-rate LFOs
(per-block rows of cutoff, resonance, low and high), the others hold still.

Tolerance: the project's bar as tests/test_gpu_resonant.py and tests/test_gpu_unison.py apply it, 1e-6 max(1, max|oracle|) on the
float32 output against float32(oracle); no sample is excluded.

With the option off no launch may be a program of two families: that is what the option gates.  A part of the graph that is a
program of ONE family may still run as one where the reader above it asks for no history rows, exactly as before the option existed
(the PM pair of `bell` in a batch that starts at position 0, Sawtooth -> ResonantLowPass under the Shaper of `overdrive`), so the
check is on the families of every voice_program launch, and on the per-node kernels that must be there."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import gpu_ready, tolerance
from helpers import HOUR, RATE, f32, maxerr
import mixed_patches as MP

pytestmark = pytest.mark.gpu

ROUTES = {'off': {'mixed_programs': False}, 'interpreted': {'mixed_programs': True, 'fuse_program': 'always'},
          'specialised': {'mixed_programs': True, 'specialise': True}}
PER_NODE = ('osc_bank', 'biquad', 'shaper', 'band')                           # launches of the per-node schedule
#            voices, voices per lane, block frames, batches, position
GEOMETRY = {'odd': (70, 1, 256, (3, 2), 0), 'pair_hour': (128, 2, 256, (3, 2), HOUR), 'short_hour': (70, 1, 64, (3, 2), HOUR),
            'short_pair': (128, 2, 64, (3, 2), 0)}
COPIES = {'supersaw': 'copies3', 'three': 'copies3'}                          # U = 3 here, the default seven in supersaw_bus


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    from signals_amd import _native
    gpu_ready()
    yield
    _native.set_voice_program_tuning(0, 0)


def build(which, V, **kw):
    p = MP.draw(V)
    if which in COPIES:
        kw.setdefault('copies', p[COPIES[which]])
    return MP.patch(which, p, **kw)


@functools.lru_cache(maxsize=None)
def wanted(which, geometry):
    """the oracle's rows of one case, shared by the three routes"""
    from oracle import chain_ref as R
    V, _, N, ks, pos = GEOMETRY[geometry]
    _, ref, C = build(which, V)
    want = R.render_stream(ref, pos, N, sum(ks), C)
    want.setflags(write=False)
    return want


@contextlib.contextmanager
def launching(route):
    """Attached images are process-wide and found by the program's words, whatever renderer asks: an 'interpreted' case after a
    'specialised' one of the same program would launch the image.  Attached kernels are used on the specialised route alone, so every
    other case runs the interpreter's own kernels (as tests/test_gpu_specialise.py does)"""
    from signals_amd import _native
    _native.voice_program_use_attached(route == 'specialised')
    try:
        yield
    finally:
        _native.voice_program_use_attached(True)


def batches(top, channels, position, N, ks, vpl, **kw):
    """(the rows of consecutive batches, the label of every launch in order, per batch)"""
    from signals_amd import _native, runtime
    from signals_amd.engine import BatchRenderer, KernelTimer
    _native.set_voice_program_tuning(vpl, 0)
    try:
        timer = KernelTimer()
        r = BatchRenderer(top, channels, RATE, timer=timer, **kw)
        parts, labels, pos = [], [], position
        for k in ks:
            before = len(timer.records)
            parts.append(r.render(pos, N, k).cpu().numpy())
            labels.append([rec[0] for rec in timer.records[before:]])
            pos += N * k
        torch.cuda.synchronize()
        runtime.check_status()
    finally:
        _native.set_voice_program_tuning(0, 0)
    return np.concatenate(parts), labels, set(timer.summary())


def program_words(label):
    """the words of a voice_program launch label `voice_program[_bus][A,B,...][*specialised]`"""
    return label[label.index('[') + 1:label.index(']')].split(',')


def check_launches(which, route, labels, names):
    from signals_amd import _native
    programs = [n for n in names if n.startswith('voice_program')]
    if route == 'off':
        for n in programs:                                                    # no combined program without the option
            assert len(_native.vp_families([(op, 0, 0, 0, 0) for op in program_words(n)])) < 2, (which, names)
        assert any(n.startswith(PER_NODE) for n in names), (which, names)
        return
    assert not any(n.startswith(PER_NODE) for n in names), (which, route, names)
    for batch in labels:                                                      # exactly one voice_program launch per batch
        ran = [n for n in batch if n.startswith('voice_program')]
        assert len(ran) == 1, (which, route, batch)
        assert len(_native.vp_families([(op, 0, 0, 0, 0) for op in program_words(ran[0])])) >= 2, ran
        assert ('*specialised' in ran[0]) == (route == 'specialised'), (which, route, ran)
        assert ran[0].startswith('voice_program_bus[') == (which in ('supersaw_bus', 'three')), ran


@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('geometry', list(GEOMETRY))
@pytest.mark.parametrize('which', MP.PATCHES)
def test_routes(which, geometry, route):
    from signals_amd import specialise
    from signals_amd.engine import NotBatchable
    V, vpl, N, ks, pos = GEOMETRY[geometry]
    if route == 'specialised':
        assert specialise.hipcc() is not None
    want = wanted(which, geometry)
    top, _, C = build(which, V)
    tol = tolerance(want)
    try:
        with launching(route):
            got, labels, names = batches(top, C, pos, N, ks, vpl, **ROUTES[route])
    except NotBatchable as e:
        # only the per-node schedule may refuse a batch (blocks shorter than the context: what it cannot batch keeps the eager path)
        print('mixed route', which, geometry, route, 'NOT BATCHABLE, nothing compared:', e)
        assert route == 'off' and N < 100, (which, geometry, route)
        return
    err = maxerr(got, f32(want))
    print('mixed route', which, geometry, route, 'max|err|', err, 'tol', tol, 'max|oracle|', float(np.abs(want).max()), sorted(names))
    check_launches(which, route, labels, names)
    assert err <= tol, (which, geometry, route, err, tol)


# ---------------------------------------------------------------------------------------------- the status word
@pytest.mark.parametrize('route', ['interpreted', 'specialised'])
def test_a_bad_resonance_in_a_mixed_program_raises(route):
    """one 0 and one NaN entry in the resonance row: NaN rows for those voices alone, SIG_STATUS_BAD_RESONANCE, check_status() raises.
    70 voices: the dead lanes of the second wave shadow a live voice and never report -- a clean row raises nothing"""
    from signals_amd import runtime
    from signals_amd.engine import BatchRenderer
    V, N = 70, 256
    runtime.check_status()                                                    # (nothing pending)
    clean, _, _ = build('supersaw', V)
    top, _, _ = build('supersaw', V)
    q = MP.draw(V)['q'].copy(); q[0, 3] = 0.0; q[0, 69] = np.nan              # the last live voice of the ragged wave among them
    top.resonance.sig.get_state().value = q
    with launching(route):
        r0 = BatchRenderer(clean, V, RATE, **ROUTES[route])
        assert not np.isnan(r0.render(0, N, 2).cpu().numpy()).any()
        runtime.check_status()                                                # no report from the padding lanes
        r = BatchRenderer(top, V, RATE, **ROUTES[route])                      # (kept: its status words live as long as it does)
        got = r.render(0, N, 2).cpu().numpy()
    bad = np.zeros(V, dtype=bool); bad[[3, 69]] = True
    assert np.isnan(got[:, bad]).all() and not np.isnan(got[:, ~bad]).any()
    with pytest.raises(ValueError, match=r'signals.chain.ext.ResonantLowPass: filter resonance must be finite and > 0'):
        runtime.check_status()
    runtime.check_status()


# ---------------------------------------------------------------------------------------------- state
@pytest.mark.parametrize('route', ['interpreted', 'specialised'])
def test_an_in_place_edit_of_copies_or_of_a_table_changes_the_next_render(route):
    """the copies travel by value with each launch and the device table follows its array: the second render reads the edit"""
    with launching(route):
        _edits(route)


def _edits(route):
    from oracle import chain_ref as R
    from signals_amd.engine import BatchRenderer
    V, N, K = 70, 256, 3
    p = MP.draw(V)
    copies = p['copies3'].copy()
    top, ref, C = MP.patch('three', p, copies=copies)
    r = BatchRenderer(top, C, RATE, **ROUTES[route])
    want = R.render_stream(ref, 0, N, K, C)
    tol = tolerance(want)
    assert maxerr(r.render(0, N, K).cpu().numpy(), f32(want)) <= tol, route
    copies[:, 0] *= 0.25                                                      # in place: the same array object
    copies[2, 1] = 0.125
    _, ref, _ = MP.patch('three', p, copies=copies)                           # (a fresh oracle graph: no cached blocks of the old layout)
    r.reset()
    want2 = R.render_stream(ref, 0, N, K, C)
    err = maxerr(r.render(0, N, K).cpu().numpy(), f32(want2))
    print('mixed copies edit', route, 'max|err|', err, 'tol', tol, 'moved', maxerr(want2, want))
    assert maxerr(want2, want) > 1e-3 and err <= tol, (route, err)            # the edit is audible, and the render follows it

    table = p['table'].copy()
    top, ref, C = MP.patch('pad', p, table=table)
    r = BatchRenderer(top, C, RATE, **ROUTES[route])
    want = R.render_stream(ref, 0, N, K, C)
    tol = tolerance(want)
    assert maxerr(r.render(0, N, K).cpu().numpy(), f32(want)) <= tol, route
    table[:, 1] *= -0.5                                                       # in place
    table[7, 0] = 0.25
    _, ref, _ = MP.patch('pad', p, table=table)
    r.reset()
    want2 = R.render_stream(ref, 0, N, K, C)
    err = maxerr(r.render(0, N, K).cpu().numpy(), f32(want2))
    print('mixed table edit', route, 'max|err|', err, 'tol', tol, 'moved', maxerr(want2, want))
    assert maxerr(want2, want) > 1e-3 and err <= tol, (route, err)
