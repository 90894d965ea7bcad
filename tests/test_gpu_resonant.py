"""The resonant low-pass / high-pass on the GPU: sig_biquad_coldstart_q against the numpy restatement (tests/resonant_reference.py),
and five voice shapes through the eager path and the engine's routes -- one kernel per node (fuse=False), the interpreted voice program
(fuse_program='always') and the kernel specialised for it (specialise=True) -- against the oracle's render_stream.

Geometry: 130 voices cross the 64-lane x 2-voices-per-lane tile and leave dead lanes, 1 and 4 voices take the scalar and the aligned
four-per-lane stores; blocks of 32 (shorter than the context), 128 and 256 frames; 1, 3 and 5 blocks, the 5 as batches of 2 and 3 so
that tails and history carry; positions 0, 50 (less than a full context) and one hour.  Cutoffs log-spaced from 40 Hz to 0.4 rate, q
from {0.5, 1/sqrt2, 2, 8} dealt across the voices.

Tolerance: 1e-6 max(1, max|oracle|) per case, the project's 1e-6 bar scaled the way float32 storage scales: at q = 8 the peak is
about 8 and the filter's L1 gain 10.2, so the per-node error is about 6e-8 (input rounding) x 10.2 + half an ulp at 8 = 1.1e-6.  The
swept controls follow Triangle LFOs (exact arithmetic on both sides), so the designs agree to rounding.  Every launch label is
checked: no closed-form, walker, cascade, latency or bus-over-filter kernel may render a resonant voice.  References are rendered
once per (case, geometry) and shared by the routes."""
import functools
import math

import numpy as np
import pytest
import torch

from gpu_helpers import ROUTES_FORCED as ROUTES, dev, gpu_ready, render_batches, tolerance
from helpers import HOUR, RATE, f32, fix, maxerr, mkosc, render, stream
import resonant_reference as RR

pytestmark = pytest.mark.gpu

FUSED = ('fused', 'latency', 'cascade', 'steady', 'walk', 'biquad_coldstart[', 'biquad_bus', 'biquad_coldstart_env')
QS = (0.5, 1.0 / math.sqrt(2.0), 2.0, 8.0)
#            voices, block frames, batches, position
GEOMETRY = {'tile': (130, 128, (2, 3), 0), 'hour': (130, 256, (3,), HOUR), 'four': (4, 128, (1,), 50),
            'short': (130, 32, (2, 3), HOUR), 'short_one': (1, 32, (2, 3), 0)}


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


def draw(V):
    """per-voice rows: cutoffs log-spaced over the band, q dealt from QS, everything else from a fixed generator"""
    rng = np.random.default_rng(5)
    th = rng.uniform(0, np.pi / 2, V)
    return dict(cut=np.geomspace(40.0, 0.4 * RATE, V)[None, :] if V > 1 else np.array([[1000.0]]),
                q=np.array([QS[(v + 3) % 4] for v in range(V)])[None, :],
                hertz=rng.uniform(55, 1760, (1, V)), phase=rng.uniform(0, 1, (1, V)), pan=np.stack([np.cos(th), np.sin(th)]))


# ---------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize('voices,N,K,pos', [(130, 128, 3, 0), (1, 32, 5, 50), (4, 256, 1, HOUR), (130, 32, 3, HOUR), (200, 128, 5, 50)])
def test_kernel_against_the_restatement(voices, N, K, pos):
    """float32 and float64 buffers, padded strides, a broadcast (1, 1) q, per-block rows of either control, and a null q"""
    from signals_amd import _native
    rng = np.random.default_rng(voices + N)
    p = draw(voices)
    hist = min(100, pos)
    x = f32(rng.uniform(-1, 1, (hist + N * K, voices)))
    cut_b = p['cut'] * rng.uniform(0.8, 1.2, (K, 1))
    q_b = p['q'] * rng.uniform(0.7, 1.3, (K, 1))
    rows = {'const': (p['cut'], p['q']), 'one_q': (p['cut'], np.array([[2.0]])), 'null_q': (p['cut'], None),
            'swept_cut': (cut_b, p['q']), 'swept_q': (p['cut'], q_b), 'swept_both': (cut_b, q_b)}
    for btype in ('lp', 'hp'):
        for name, (cut, q) in rows.items():
            want = RR.filter_blocks(btype, x.astype(np.float64), hist, N, K, cut, q, RATE)
            tol = tolerance(want)
            for t_buf, pad in ((torch.float32, 0), (torch.float32, 3), (torch.float64, 2)):
                xbuf = torch.zeros((hist + N * K, voices + pad), dtype=t_buf, device='cuda:0')
                xbuf[:, :voices] = dev(x, t_buf)
                obuf = torch.zeros((N * K, voices + pad), dtype=t_buf, device='cuda:0')
                status = torch.zeros(1, dtype=torch.int32, device='cuda:0')
                _native.biquad_coldstart_q(btype, RATE, pos, N, K, 100, dev(cut), None if q is None else dev(q), xbuf[:, :voices], hist,
                                           obuf[:, :voices], status=status)
                got = obuf.cpu().numpy()
                err = maxerr(got[:, :voices], want)
                print('resonant kernel', btype, name, voices, N, K, pos, t_buf, 'max|err|', err, 'tol', tol)
                assert not got[:, voices:].any() and int(status.item()) == 0, (btype, name)      # the padding stays, nothing is refused
                assert err <= tol, (btype, name, t_buf, pad, err, tol)
            if name == 'null_q':                                              # unplugged: what sig_biquad_coldstart computes, bit for bit
                a = torch.empty((N * K, voices), dtype=torch.float32, device='cuda:0')
                b = torch.empty_like(a)
                xin = dev(x, torch.float32)
                _native.biquad_coldstart_q(btype, RATE, pos, N, K, 100, dev(cut), None, xin, hist, a)
                _native.biquad_coldstart(btype, RATE, pos, N, K, 100, dev(cut), xin, hist, b)
                assert torch.equal(a, b), btype


@pytest.mark.parametrize('bad', [0.0, -1.0, math.nan, math.inf, -math.inf])
def test_kernel_status_bits(bad):
    """a bad q in a live voice: NaN rows for that voice alone and SIG_STATUS_BAD_RESONANCE; a bad cutoff keeps its own bit.  The same
    value past `voices` (the padding of a wider row): nothing -- the dead lanes of the last tile shadow voice 0 and never read those
    columns, so this shows that the kernel stays inside `voices`, not how a dead lane would report"""
    from signals_amd import _native
    voices, N, K = 130, 128, 2
    p = draw(voices)
    x = dev(f32(np.random.default_rng(1).uniform(-1, 1, (N * K, voices))), torch.float32)
    out = torch.empty((N * K, voices), dtype=torch.float32, device='cuda:0')
    status = torch.zeros(1, dtype=torch.int32, device='cuda:0')
    q = p['q'].copy(); q[0, 129] = bad
    _native.biquad_coldstart_q('lp', RATE, 0, N, K, 100, dev(p['cut']), dev(q), x, 0, out, status=status)
    got = out.cpu().numpy()
    assert int(status.item()) == _native.STATUS_BAD_RESONANCE
    assert np.isnan(got[:, 129]).all() and not np.isnan(got[:, :129]).any()
    wide = np.concatenate([p['q'], np.full((1, 4), bad)], axis=1)              # 134 columns, the bad ones past the 130 voices
    status.zero_()
    _native.biquad_coldstart_q('lp', RATE, 0, N, K, 100, dev(p['cut']), dev(wide)[:, :voices], x, 0, out, status=status)
    assert int(status.item()) == 0 and not np.isnan(out.cpu().numpy()).any()
    cut = p['cut'].copy(); cut[0, 0] = 0.0
    _native.biquad_coldstart_q('hp', RATE, 0, N, K, 100, dev(cut), dev(q), x, 0, out, status=status)
    assert int(status.item()) == _native.STATUS_BAD_CUTOFF | _native.STATUS_BAD_RESONANCE


# ---------------------------------------------------------------------------------------------- graphs
def lfo_row(row, depth, hz):
    """row * (1 + depth * triangle(hz t)) as a block-rate control: (GPU node, oracle node)"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    g = fx.Gain(); g.left = mkosc('Triangle', [[hz]]); g.right = fix(2.0 * depth * row)
    m = fx.Mix(); m.left = g; m.right = fix(2.0 * row); m.mix = fix([[0.5]])
    ref = R.Binary('Mix', R.Binary('Gain', R.Osc('Triangle', R.Fixed([[hz]])), R.Fixed(2.0 * depth * row)), R.Fixed(2.0 * row), R.Fixed([[0.5]]))
    return m, ref


def res(cls, input_, cutoff, q=None):
    f = cls(); f.input = input_
    f.cutoff = fix(cutoff) if isinstance(cutoff, np.ndarray) else cutoff
    if q is not None:
        f.resonance = fix(q) if isinstance(q, np.ndarray) else q
    return f


def graph(which, p):
    """(GPU node, oracle node, rendered width) of one voice shape over the rows `p`"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    RF = RR.oracle_node()
    V = p['cut'].shape[1]
    saw = lambda: mkosc('Sawtooth', p['hertz'], p['phase'])
    rsaw = lambda: R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase']))
    if which == 'const':                                                      # Saw -> ResonantLowPass
        return res(ext.ResonantLowPass, saw(), p['cut'], p['q']), RF('lp', rsaw(), R.Fixed(p['cut']), R.Fixed(p['q'])), V
    if which == 'swept':                                                      # cutoff and q follow block-rate LFOs: per-block rows
        (c, rc), (q, rq) = lfo_row(p['cut'], 0.2, 7.0), lfo_row(p['q'], 0.4, 11.0)
        return res(ext.ResonantLowPass, saw(), c, q), RF('lp', rsaw(), rc, rq), V
    if which == 'hp_lp':                                                      # ResonantHighPass -> ResonantLowPass
        inner = res(ext.ResonantHighPass, saw(), p['cut'], p['q'])
        rinner = RF('hp', rsaw(), R.Fixed(p['cut']), R.Fixed(p['q']))
        cut2, q2 = p['cut'][:, ::-1].copy(), np.roll(p['q'], 1, axis=1)
        return res(ext.ResonantLowPass, inner, cut2, q2), RF('lp', rinner, R.Fixed(cut2), R.Fixed(q2)), V
    if which == 'mix_lp':                                                     # ResonantLowPass(Mix(Saw, Square)) -> LowPass
        m = fx.Mix(); m.left = saw(); m.right = mkosc('Square', p['hertz'] * 0.5); m.mix = fix([[0.3]])
        rm = R.Binary('Mix', rsaw(), R.Osc('Square', R.Fixed(p['hertz'] * 0.5)), R.Fixed([[0.3]]))
        lp = fx.LowPass(); lp.input = res(ext.ResonantLowPass, m, p['cut'], p['q']); wide = np.minimum(p['cut'] * 1.5, 0.45 * RATE)
        lp.cutoff = fix(wide)
        return lp, R.Filter('lp', RF('lp', rm, R.Fixed(p['cut']), R.Fixed(p['q'])), R.Fixed(wide)), V
    if which == 'bus':                                                        # a resonant voice under a stereo SumBus
        b = ext.SumBus(); b.input = res(ext.ResonantLowPass, saw(), p['cut'], p['q']); b.get_state().gains = np.ascontiguousarray(p['pan'])
        return b, R.SumBus(RF('lp', rsaw(), R.Fixed(p['cut']), R.Fixed(p['q'])), p['pan']), 2
    raise KeyError(which)


@functools.lru_cache(maxsize=None)
def wanted(which, geometry):
    from oracle import chain_ref as R
    V, N, ks, pos = GEOMETRY[geometry]
    _, ref, C = graph(which, draw(V))
    want = R.render_stream(ref, pos, N, sum(ks), C)
    want.setflags(write=False)
    return want


def batches(top, channels, position, N, ks, **kw):
    """(the rows of consecutive batches, the labels of the launches that rendered them); the status word is checked"""
    return render_batches(top, channels, position, N, ks, names=True, check_status=True, **kw)[:2]


def check_labels(names, route, bus=False, plain_filter=False):
    """`plain_filter`: the graph also holds an fx.LowPass, whose own Butterworth kernel the per-node route launches"""
    allowed = ('biquad_coldstart[',) if plain_filter and route == 'per_node' else ()
    assert not any(word in n for n in names for word in FUSED if word not in allowed), (route, names)
    programs = [n for n in names if n.startswith('voice_program')]
    if route == 'per_node':
        assert not programs and any(n.startswith('biquad_coldstart_q[') for n in names), names
        return
    assert programs and all('FilterQ' in n for n in programs), (route, names)
    assert not any(n.startswith(('biquad_coldstart', 'osc_bank[Saw', 'sum_bus')) for n in names), (route, names)
    assert all(n.startswith('voice_program_bus[') for n in programs) == bus, names
    assert all('*specialised' in n for n in programs) == (route == 'specialise'), (route, names)


# every shape at the three long-block geometries; blocks shorter than the context: the single filter, and the cascade on the routes
# that render it there (the per-node schedule cannot batch a filter behind a filter at N <= 100: NotBatchable, as for fx.LowPass)
CASES = [(w, g, r) for w in ('const', 'swept', 'hp_lp', 'mix_lp', 'bus') for g in ('tile', 'hour', 'four') for r in ('eager', *ROUTES)]
CASES += [('const', g, r) for g in ('short', 'short_one') for r in ('eager', *ROUTES)]
CASES += [('hp_lp', g, r) for g in ('short', 'short_one') for r in ('eager', 'always', 'specialise')]


@pytest.mark.parametrize('which,geometry,route', CASES)
def test_routes(which, geometry, route):
    from signals_amd import runtime, specialise
    V, N, ks, pos = GEOMETRY[geometry]
    want = wanted(which, geometry)
    top, _, C = graph(which, draw(V))
    if route == 'eager':
        got, names = stream(top, pos, N, sum(ks), C), None
        runtime.check_status()
    else:
        if route == 'specialise':
            assert specialise.hipcc() is not None
        got, names = batches(top, C, pos, N, ks, **ROUTES[route])
        check_labels(names, route, bus=which == 'bus', plain_filter=which == 'mix_lp')
        if which == 'swept' and route == 'per_node' and max(ks) > 1:      # (one block: one row, the constant form)
            assert any(n.startswith('biquad_coldstart_q[lp,blocks]') for n in names), names
    err, tol = maxerr(got, f32(want)), tolerance(want)
    print('resonant route', which, geometry, route, 'max|err|', err, 'tol', tol, 'max|oracle|', float(np.abs(want).max()))
    assert err <= tol, (which, geometry, route, err, tol)


# ---------------------------------------------------------------------------------------------- behaviour
@pytest.mark.parametrize('route', ['eager', *ROUTES])
def test_unplugged_resonance_renders_the_butterworth_filter(route):
    from signals_amd.chain import ext, fx
    V, N, ks, pos = GEOMETRY['tile']
    p = draw(V)
    for cls, plain in ((ext.ResonantLowPass, fx.LowPass), (ext.ResonantHighPass, fx.HighPass)):
        ours = res(cls, mkosc('Sawtooth', p['hertz'], p['phase']), p['cut'])
        theirs = plain(); theirs.input = mkosc('Sawtooth', p['hertz'], p['phase']); theirs.cutoff = fix(p['cut'])
        off = res(cls, mkosc('Sawtooth', p['hertz'], p['phase']), p['cut'], np.full((1, V), 8.0))
        off.resonance.sig.get_state().enabled = False                         # a disabled source: unplugged too
        if route == 'eager':
            a, b, c = (stream(n, pos, N, sum(ks), V) for n in (ours, theirs, off))
        else:
            (a, names), (b, _), (c, _) = (batches(n, V, pos, N, ks, **ROUTES[route]) for n in (ours, theirs, off))
            check_labels(names, route)
        tol = tolerance(b)
        print('resonant unplugged', route, cls.__name__, 'max|err|', maxerr(a, b), 'tol', tol)
        assert maxerr(a, b) <= tol and np.array_equal(a, c), (route, cls.__name__)


@pytest.mark.parametrize('route', ['eager', *ROUTES])
@pytest.mark.parametrize('bad', [0.0, -1.0, math.nan, math.inf])
def test_a_bad_resonance_in_a_live_voice_raises(bad, route):
    from signals_amd import runtime
    from signals_amd.chain import ext
    from signals_amd.engine import BatchRenderer
    V, N = 130, 128
    p = draw(V)
    runtime.check_status()                                                    # (nothing pending)
    q = p['q'].copy(); q[0, 129] = bad                                        # the last live voice of the ragged tile
    top = res(ext.ResonantLowPass, mkosc('Sawtooth', p['hertz'], p['phase']), p['cut'], q)
    r = None if route == 'eager' else BatchRenderer(top, V, RATE, **ROUTES[route])    # (kept: its status words live as long as it does)
    got = stream(top, 0, N, 2, V) if r is None else r.render(0, N, 2).cpu().numpy()
    assert np.isnan(got[:, 129]).all() and not np.isnan(got[:, :129]).any()
    with pytest.raises(ValueError, match=r'signals.chain.ext.ResonantLowPass: filter resonance must be finite and > 0'):
        runtime.check_status()
    runtime.check_status()
    # the same value past the request's width (the padding of a wider row): the engine slices the rows to the request before any
    # launch and the dead lanes of the last tile shadow voice 0, so what this shows is that the slice is honoured on every route
    # (the eager path refuses a reply wider than its request, like the reference: BadShape)
    if route != 'eager':
        wide = np.concatenate([p['q'], np.full((1, 2), bad)], axis=1)
        top = res(ext.ResonantLowPass, mkosc('Sawtooth', p['hertz'], p['phase']), np.concatenate([p['cut'], p['cut'][:, :2]], axis=1), wide)
        r = BatchRenderer(top, V, RATE, **ROUTES[route])
        got = r.render(0, N, 2).cpu().numpy()
        runtime.check_status()
        assert not np.isnan(got).any()


@pytest.mark.parametrize('with_', ['band', 'shaper'])
def test_with_a_band_filter_or_a_shaper_the_node_renders_per_node(with_):
    """ResonantLowPass(BandPass(Saw)) and ResonantLowPass(Shaper(Saw)): no interpreter variant has both instructions, so on every
    route the resonant filter runs as its own kernel over its input's stored rows"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    import shaper_reference as SR
    V, N, ks, pos = GEOMETRY['tile']
    p = draw(V)
    RF = RR.oracle_node()
    curve = SR.tanh_curve(513, 3.0)
    low, high = p['cut'] * 0.5, p['cut'] * 1.1

    def build():
        if with_ == 'band':
            src = fx.BandPass(); src.input = mkosc('Sawtooth', p['hertz'], p['phase']); src.low = fix(low); src.high = fix(high)
        else:
            src = ext.Shaper(); src.get_state().table = curve; src.input = mkosc('Sawtooth', p['hertz'], p['phase'])
        return res(ext.ResonantLowPass, src, p['cut'], p['q'])
    rsaw = R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase']))
    rsrc = R.BandFilter('bp', rsaw, R.Fixed(low), R.Fixed(high)) if with_ == 'band' else SR.oracle_node()(curve, rsaw)
    want = R.render_stream(RF('lp', rsrc, R.Fixed(p['cut']), R.Fixed(p['q'])), pos, N, sum(ks), V)
    tol = tolerance(want)
    for route in ROUTES:
        got, names = batches(build(), V, pos, N, ks, **ROUTES[route])
        assert not any(word in n for n in names for word in FUSED), names
        assert any(n.startswith('biquad_coldstart_q[lp]') for n in names), (route, names)
        assert not any(n.startswith('voice_program') and 'FilterQ' in n for n in names), names
        err = maxerr(got, f32(want))
        print('resonant with', with_, route, 'max|err|', err, 'tol', tol)
        assert err <= tol, (with_, route, err, tol)


def test_inside_a_control_path_the_node_keeps_the_eager_path():
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    from signals_amd.engine import BatchRenderer, NotBatchable
    V, N = 4, 256
    p = draw(V)
    RF = RR.oracle_node()
    lfo = res(ext.ResonantLowPass, mkosc('Triangle', np.full((1, V), 30.0)), np.full((1, V), 2000.0), p['q'])
    g = fx.Gain(); g.left = mkosc('Sawtooth', p['hertz'], p['phase']); g.right = lfo
    with pytest.raises(NotBatchable, match='resonant filter'):
        BatchRenderer(g, V, RATE).render(0, N, 2)
    got = stream(g, 0, N, 3, V)
    rl = RF('lp', R.Osc('Triangle', R.Fixed(np.full((1, V), 30.0))), R.Fixed(np.full((1, V), 2000.0)), R.Fixed(p['q']))
    want = R.render_stream(R.Binary('Gain', R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase'])), rl), 0, N, 3, V)
    assert maxerr(got, f32(want)) <= tolerance(want)
