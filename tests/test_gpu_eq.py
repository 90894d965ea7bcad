"""The RBJ equaliser biquads on the GPU: each of the six kinds against the numpy restatement (tests/eq_reference.py) on all four routes
-- one kernel per node (fuse=False: sig_biquad_coldstart_eq), the interpreted voice program (the RES+EQ kernels), the kernel
specialised for the program, and the mixed program behind a UnisonSawtooth (mixed_programs=True: the MIXED+EQ kernels).

Shape: 70 voices -- the last wave has padding lanes and the count is no multiple of the two-voices-per-lane tile; N = 128, three
blocks rendered one after the other from position 0 (a batch of one, then a batch of two: the context comes from the block before);
N = 32, shorter than the context; one block an hour into the stream.  Per voice: a sawtooth (or seven of them) of amplitude 0.25 with
hertz spread over 55 .. 1760, cutoffs spread over 200 .. 8000 Hz plus one voice each at 20 Hz and 23 kHz, q dealt from {0.5, 1/sqrt2,
4} and gain from {-12, 0, +12} dB so that all nine pairs occur.

Bound: the project's own, max|float32 output - float32(oracle)| <= 1e-6.  The input level keeps the outputs near 1
in magnitude or below: the largest is the low shelf's, 2.1, where +12 dB meets the 23 kHz cutoff (the whole band lifted fourfold).  References are rendered once per (kind, source, geometry) and shared by the routes."""
import functools
import math

import numpy as np
import pytest
import torch

from gpu_helpers import ROUTES_FORCED, dev, gpu_ready, render_batches
from helpers import HOUR, RATE, f32, fix, maxerr, mkosc
import eq_reference as EQ
import unison_reference as UR

pytestmark = pytest.mark.gpu

BOUND = 1e-6
ROUTES = {**ROUTES_FORCED, 'mixed': {'fuse_program': 'always', 'mixed_programs': True}}
FUSED = ('fused', 'latency', 'cascade', 'steady', 'walk', 'biquad_coldstart[', 'biquad_bus', 'biquad_coldstart_env', 'biquad_coldstart_q[')
QS, GAINS = (0.5, 1.0 / math.sqrt(2.0), 4.0), (-12.0, 0.0, 12.0)
V = 70
#            block frames, batches, position
GEOMETRY = {'blocks': (128, (1, 2), 0), 'short': (32, (1, 2), 0), 'hour': (128, (1,), HOUR)}


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


def classes():
    from signals_amd.chain import ext
    return {'bp': ext.ResonantBandPass, 'notch': ext.Notch, 'ap': ext.AllPass, 'peak': ext.Peaking, 'ls': ext.LowShelf, 'hs': ext.HighShelf}


def draw():
    rng = np.random.default_rng(7)
    cut = np.geomspace(200.0, 8000.0, V)
    cut[0], cut[1] = 20.0, 23000.0
    return dict(hertz=np.linspace(55.0, 1760.0, V)[None, :], phase=rng.uniform(0, 1, (1, V)), spread=rng.uniform(0, 1, (1, V)),
                cut=cut[None, :], q=np.array([QS[v % 3] for v in range(V)])[None, :],
                gain=np.array([GAINS[(v // 3) % 3] for v in range(V)])[None, :], level=np.full((1, V), 0.25))


def voice(kind, p, unison=False):
    """(GPU node, oracle node): Sawtooth (or UnisonSawtooth) -> Gain 0.25 -> the equaliser of `kind`"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    if unison:
        src = ext.UnisonSawtooth(); src.hertz = fix(p['hertz']); src.phase = fix(p['phase']); src.spread = fix(p['spread'])
        rsrc = UR.UnisonOsc('Sawtooth', UR.default_copies(), R.Fixed(p['hertz']), R.Fixed(p['phase']), R.Fixed(p['spread']))
    else:
        src, rsrc = mkosc('Sawtooth', p['hertz'], p['phase']), R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase']))
    g = fx.Gain(); g.left = src; g.right = fix(p['level'])
    f = classes()[kind](); f.input = g; f.cutoff = fix(p['cut']); f.resonance = fix(p['q'])
    gained = kind in EQ.GAIN_KINDS
    if gained:
        f.gain = fix(p['gain'])
    ref = EQ.oracle_node()(kind, R.Binary('Gain', rsrc, R.Fixed(p['level'])), R.Fixed(p['cut']), R.Fixed(p['q']), R.Fixed(p['gain']) if gained else None)
    return f, ref


@functools.lru_cache(maxsize=None)
def wanted(kind, unison, geometry):
    from oracle import chain_ref as R
    N, ks, pos = GEOMETRY[geometry]
    want = R.render_stream(voice(kind, draw(), unison)[1], pos, N, sum(ks), V)
    want.setflags(write=False)
    return want


def batches(top, position, N, ks, check=True, **kw):
    """(the rows of consecutive batches, the labels of the launches that rendered them, the renderer)"""
    return render_batches(top, V, position, N, ks, names=True, check_status=check, **kw)


def check_labels(names, route):
    assert not any(word in n for n in names for word in FUSED), (route, names)
    programs = [n for n in names if n.startswith('voice_program')]
    if route == 'per_node':
        assert not programs and any(n.startswith('biquad_coldstart_eq[') for n in names), names
        return
    assert programs and all('FilterEq' in n for n in programs) and len(names) == len(programs), (route, names)
    assert all('OscUni' in n for n in programs) == (route == 'mixed'), (route, names)
    assert all('*specialised' in n for n in programs) == (route == 'specialise'), (route, names)


@pytest.mark.parametrize('geometry', list(GEOMETRY))
@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('kind', EQ.KINDS)
def test_routes(kind, route, geometry):
    from signals_amd import specialise
    N, ks, pos = GEOMETRY[geometry]
    unison = route == 'mixed'
    want = wanted(kind, unison, geometry)
    if route == 'specialise':
        assert specialise.hipcc() is not None
    got, names, _ = batches(voice(kind, draw(), unison)[0], pos, N, ks, **ROUTES[route])
    check_labels(names, route)
    err = maxerr(got, f32(want))
    print('eq route', kind, route, geometry, 'max|err|', err, 'bound', BOUND, 'max|oracle|', float(np.abs(want).max()))
    assert err <= BOUND, (kind, route, geometry, err)


@pytest.mark.parametrize('route', list(ROUTES))
def test_peaking_at_zero_db_is_the_input(route):
    N, ks, pos = GEOMETRY['blocks']
    p = draw()
    p['gain'] = np.zeros((1, V))
    unison = route == 'mixed'
    top, ref = voice('peak', p, unison)
    got, names, _ = batches(top, pos, N, ks, **ROUTES[route])
    check_labels(names, route)
    from oracle import chain_ref as R
    dry = R.render_stream(ref.inputs['input'], pos, N, sum(ks), V)            # the oracle's Gain(Saw): what goes in
    err = maxerr(got, f32(dry))
    print('eq peaking 0 dB', route, 'max|err|', err)
    assert err <= BOUND, (route, err)


@pytest.mark.parametrize('route', list(ROUTES))
def test_bad_controls_in_live_voices(route):
    """one bad cutoff, one q = 0 and one gain = inf, each on its own voice: NaN rows for those voices alone, every other voice within
    the bound, exactly the three status bits, and check_status() raises"""
    from signals_amd import _native, runtime
    N, ks, pos = GEOMETRY['blocks']
    p = draw()
    p['cut'] = p['cut'].copy(); p['q'] = p['q'].copy(); p['gain'] = p['gain'].copy()
    p['cut'][0, 5], p['q'][0, 33], p['gain'][0, 69] = 0.0, 0.0, math.inf      # (69: the last live voice of the ragged tile)
    bad = [5, 33, 69]
    unison = route == 'mixed'
    runtime.check_status()                                                    # (nothing pending)
    top, ref = voice('peak', p, unison)
    got, names, r = batches(top, pos, N, ks, check=False, **ROUTES[route])
    check_labels(names, route)
    bits = int(r._status[top].tensor.item())
    assert bits == _native.STATUS_BAD_CUTOFF | _native.STATUS_BAD_RESONANCE | _native.STATUS_BAD_GAIN == 7, bits
    with pytest.raises(ValueError, match=r'signals.chain.ext.Peaking: Digital filter critical frequencies must be 0 < Wn < 1'):
        runtime.check_status()
    runtime.check_status()                                                    # (polled: cleared)
    assert np.isnan(got[:, bad]).all()
    good = [v for v in range(V) if v not in bad]
    assert not np.isnan(got[:, good]).any()
    want = wanted('peak', unison, 'blocks')                                   # the other voices' rows do not depend on the bad ones
    err = maxerr(got[:, good], f32(want)[:, good])
    print('eq bad controls', route, 'max|err| of the other voices', err)
    assert err <= BOUND, (route, err)


def test_kernel_status_bits_one_at_a_time():
    """sig_biquad_coldstart_eq: each refusal sets its own bit; a gain that is not finite is not read by the kinds without one"""
    from signals_amd import _native
    N, K = 128, 2
    p = draw()
    x = dev(f32(np.random.default_rng(1).uniform(-0.25, 0.25, (N * K, V))), torch.float32)
    out = torch.empty((N * K, V), dtype=torch.float32, device='cuda:0')
    status = torch.zeros(1, dtype=torch.int32, device='cuda:0')
    for name, bit, value in (('cut', _native.STATUS_BAD_CUTOFF, math.nan), ('q', _native.STATUS_BAD_RESONANCE, -1.0),
                             ('gain', _native.STATUS_BAD_GAIN, math.nan), ('gain', _native.STATUS_BAD_GAIN, -math.inf)):
        rows = {k: p[k].copy() for k in ('cut', 'q', 'gain')}
        rows[name][0, 69] = value
        status.zero_()
        _native.biquad_coldstart_eq('eqls', RATE, 0, N, K, 100, dev(rows['cut']), dev(rows['q']), dev(rows['gain']), x, 0, out, status=status)
        got = out.cpu().numpy()
        assert int(status.item()) == bit, (name, value)
        assert np.isnan(got[:, 69]).all() and not np.isnan(got[:, :69]).any(), (name, value)
    status.zero_()
    _native.biquad_coldstart_eq('eqnotch', RATE, 0, N, K, 100, dev(p['cut']), dev(p['q']), dev(rows['gain']), x, 0, out, status=status)
    assert int(status.item()) == 0 and not np.isnan(out.cpu().numpy()).any()
