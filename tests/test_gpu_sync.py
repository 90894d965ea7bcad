"""Hard-sync oscillators on the GPU: sig_osc_bank_sync against tests/sync_reference.py in both stores, and every render route (the
eager nodes, fuse=False, the interpreted program, the specialised one, the mixed interpreter and the mixed specialised image for the
resonant patch) against the oracle graph, with the launch labels of each; the node in a control path, edits of `copies` and of the
ratio between renders, the one specialised image that serves every ratio, and the aliasing measurement of tests/test_sync_host.py on
what the GPU rendered.

Tolerances.  sig_osc_bank_sync shares the restatement's master phase t bit for bit (the unison oscillator's operations in its order,
-ffp-contract=off), its m = mod(t, 1), its s = m R (one rounded product on both sides), k = floor(s) and f = s - k (exact): the
phases differ by 0 ulp, so both sides choose the same window and the same conditions on k for every sample -- also where the last
interior edge's window is cut at the reset.  What is left of  phase ulps x R x (2 + 2 / ds)  is the kernel's rounded 1 / ds (and
1 / d) where the restatement divides: x = p fl(1 / ds) against p / ds is a relative error <= 3 x 2^-53, that is a phase error of at
most 3 x 2^-53 ds inside a window (p < ds), which the residual's slope 2 / ds turns into 6.7e-16 whatever ds and R are.  The Square
has two such residuals and the reset's (weight <= 1), the Sawtooth one and the reset's: <= 2e-15, and five roundings of sums of
values <= 2 add 1.1e-15; the mean over the copies cannot amplify.  1e-14 for the f64 store is three times that, derived and not
measured.  The f32 store adds one float32 rounding of a value in [-1, 1] (6e-8): within 2e-7 max(1, |ref|).  Graph routes: 1e-6
max(1, |ref|max), the project's bound; the program handlers take m by v_fract_f64, which differs from numpy's mod only for t in
(-2^-54, 0); no sample is excluded anywhere.

Inputs: tests/test_gpu_blep.py's SPECIAL pitches in every case's first voices (rate / 64 at phase 0: the reset and the interior
edges are hit exactly; a negative pitch, 0 Hz, 1e-3 Hz, 30 kHz, 13 kHz, then musical ones); the ratios cycle through 1, 1.5, 2.75,
3.25 and 7.77 across the voices, unplugged is a launch of its own, and with several blocks every row changes per block.

The interpreter's sync kernel sets have the OscSync handler and the earlier sets do not: a program with the word that reached another
set would skip the word and miss every bound here, so the route tests also show that the launch picks the sync set for the word
-- in the one or two kernels of each set that 97 voices and these sinks reach; tests/test_gpu_vp_variants.py renders all twelve of
`sync` and of `mixed_sync` (both register files, one and two voices per lane, the three sinks), and their short-block mode;
that programs without the word keep their kernels is what tools/compare_kernels.py shows at build time."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import dev, gpu_ready, lfo, render_batches, tolerance
from helpers import HOUR, RATE, f32, fix, maxerr, mkosc, stream
import resonant_reference as RR
import shaper_reference as SHR
import sync_reference as SR

pytestmark = pytest.mark.gpu

KINDS = ('Sawtooth', 'Square')
V = 97                                                                        # no multiple of 64, of 4 (the voice tile) or of 2
KS = (2, 1)                                                                   # K = 3 blocks in two consecutive batches
SPECIAL = (RATE / 64, -440.0, 0.0, 1e-3, 30000.0, 13000.0, 27.5, 261.6255653005986, 4186.009044809578)
RATIOS = (1.0, 1.5, 2.75, 3.25, 7.77)
ROUTES = {'per_node': {'fuse': False}, 'always': {'fuse_program': 'always'}, 'specialise': {'specialise': True},
          'mixed': {'mixed_programs': True, 'fuse_program': 'always'}, 'mixed_specialise': {'mixed_programs': True, 'specialise': True}}


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    from signals_amd import _native
    gpu_ready()
    yield
    _native.voice_program_use_attached(True)


def rows_of(rng, blocks, width):
    """hertz, phase, ratio rows (blocks, width): the special pitches first (rate / 64 at phase 0), random musical ones behind them, the
    ratios cycling through RATIOS; with several blocks every row is modulated a little (a per-block hertz and ratio)"""
    hz = rng.uniform(55, 1760, (blocks, width))
    ph = rng.uniform(0, 1, (blocks, width))
    n = min(len(SPECIAL), width)
    hz[:, :n] = np.array(SPECIAL[:n])[None, :] * (1.0 + 0.01 * np.arange(blocks))[:, None]
    hz[0, :n] = SPECIAL[:n]
    ph[:, 0] = 0.0
    ra = np.resize(np.array(RATIOS), (blocks, width)) * (1.0 + 0.07 * np.arange(blocks))[:, None]
    ra[0] = np.resize(np.array(RATIOS), width)
    return hz, ph, ra


def draw_copies(rng, U):
    c = np.stack([rng.uniform(-0.12, 0.12, U), rng.uniform(0, 1, U)], axis=1)
    c[0] = 0.0                                                                # copy 0 keeps the exact hits
    return c


# ---------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize('pos', [0, HOUR])
@pytest.mark.parametrize('kind', KINDS)
def test_osc_bank_sync_matches_the_restatement(kind, pos):
    """300 rows in 3 blocks of 100 (the parameter row changes inside a wave's 16 rows, the last wave is ragged) and 256 rows of one
    block; 1, 5 and 130 voices (one voice per lane, a partial last tile) and 132 (four per lane, vector stores), a padded leading
    dimension; one copy and seven; the ratio plugged and unplugged"""
    from signals_amd import _native
    for V_, pad, blocks, rows in ((1, 0, 3, 300), (5, 3, 3, 300), (130, 2, 3, 300), (132, 0, 3, 300), (130, 0, 1, 256)):
        for U in (1, 7):
            rng = np.random.default_rng(U)
            (hz, ph, ra), sp = rows_of(rng, blocks, V_), rng.uniform(0, 1, (blocks, V_))
            copies = draw_copies(rng, U)
            rpp = rows // blocks
            for plugged in (True, False):
                want = SR.sync(kind, copies, pos, rpp, hz, ph, sp, ra if plugged else 0.0, blocks=blocks)
                assert np.isfinite(want).all()
                for dtype in (torch.float64, torch.float32):
                    what = (kind, pos, V_, pad, blocks, U, plugged, dtype)
                    obuf = torch.zeros((rows, V_ + pad), dtype=dtype, device='cuda:0')
                    _native.osc_bank_sync(kind, pos, RATE, dev(hz), dev(ph), dev(sp), dev(ra) if plugged else None, copies, obuf[:, :V_],
                                          rows_per_param=rpp if blocks > 1 else 0)
                    got = obuf[:, :V_].cpu().numpy()
                    assert not obuf[:, V_:].any(), what                       # the padding is not written
                    if dtype == torch.float64:
                        err = maxerr(got, want)
                        print('sig_osc_bank_sync f64', what, 'max|err|', err, 'bound 1e-14')
                        assert err <= 1e-14, (what, err)
                    else:
                        err = float(np.max(np.abs(got.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))))
                        print('sig_osc_bank_sync f32', what, 'max|err| / max(1, |ref|)', err, 'bound 2e-7')
                        assert err <= 2e-7, (what, err)


@pytest.mark.parametrize('kind', KINDS)
def test_a_ratio_that_is_not_finite_gives_nan_rows_for_that_voice(kind):
    from signals_amd import _native
    hz, ra = np.full((1, 8), 440.0), np.array([[2.5, np.nan, np.inf, -np.inf, 0.5, -2.0, 1.0, 3.25]])
    want = SR.sync(kind, [[0, 0]], 0, 64, hz, ratio=ra)
    for dtype in (torch.float64, torch.float32):
        got = _native.osc_bank_sync(kind, 0, RATE, dev(hz), None, None, dev(ra), np.zeros((1, 2)),
                                    torch.empty((64, 8), dtype=dtype, device='cuda:0')).cpu().numpy()
        assert np.isnan(got[:, 1:4]).all() and np.isfinite(got[:, [0, 4, 5, 6, 7]]).all()
        assert maxerr(got, want if dtype == torch.float64 else f32(want)) <= 2e-7


# ---------------------------------------------------------------------------------------------- graphs
def node(kind, copies, hertz, phase=None, spread=None, ratio=None):
    from signals_amd.chain import ext
    u = getattr(ext, 'Sync' + kind)()
    if copies is not None:
        u.get_state().copies = copies
    u.hertz = hertz if not isinstance(hertz, np.ndarray) else fix(hertz)
    if phase is not None:
        u.phase = fix(phase)
    if spread is not None:
        u.spread = spread if not isinstance(spread, np.ndarray) else fix(spread)
    if ratio is not None:
        u.ratio = ratio if not isinstance(ratio, np.ndarray) else fix(ratio)
    return u


def draw(seed=3):
    rng = np.random.default_rng(seed)
    th = rng.uniform(0, np.pi / 2, V)
    hz, ph, ra = rows_of(rng, 1, V)
    return dict(hertz=hz, phase=ph, ratio=ra, spread=rng.uniform(0, 1, (1, V)), cut=rng.uniform(200, 8000, (1, V)),
                q=rng.uniform(0.6, 2.0, (1, V)), pan=np.stack([np.cos(th), np.sin(th)]), copies16=draw_copies(rng, 16),
                curve=SHR.tanh_curve(257, 2.0))


def graph(which, p, kind='Sawtooth', copies=None, ratio='rows'):
    """(GPU node, oracle node, rendered width); `copies`: the array both sides read (default: the node's one clean copy); `ratio`:
    'rows' (p['ratio']), None (unplugged) or an array"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    held = SR.default_copies() if copies is None else copies
    ra = p['ratio'] if isinstance(ratio, str) else ratio
    u = node(kind, copies, p['hertz'], p['phase'], p['spread'], ra)
    ru = SR.SyncOsc(kind, held, R.Fixed(p['hertz']), R.Fixed(p['phase']), R.Fixed(p['spread']), None if ra is None else R.Fixed(ra))
    if which == 'swept':                                                      # the ratio sweeps 1 -> 4 on a block-rate LFO, a Gain on top
        rat, rrat = lfo(3.1, 1.5 * np.ones((1, V)), 2.5 * np.ones((1, V)))
        u = node(kind, copies, p['hertz'], p['phase'], p['spread'], rat)
        ru = SR.SyncOsc(kind, held, R.Fixed(p['hertz']), R.Fixed(p['phase']), R.Fixed(p['spread']), rrat)
        g = fx.Gain(); g.left = u; g.right = fix(p['q'])
        return g, R.Binary('Gain', ru, R.Fixed(p['q'])), V
    if which == 'bus':                                                        # bare under a stereo SumBus
        b = ext.SumBus(); b.input = u; b.get_state().gains = np.ascontiguousarray(p['pan'])
        return b, R.SumBus(ru, p['pan']), 2
    if which == 'lowpass':
        f = fx.LowPass(); f.input = u; f.cutoff = fix(p['cut'])
        return f, R.Filter('lp', ru, R.Fixed(p['cut'])), V
    if which in ('resonant', 'shaped'):                                       # two (three) families: a mixed program, or one kernel per node
        f = ext.ResonantLowPass(); f.input = u; f.cutoff = fix(p['cut']); f.resonance = fix(p['q'])
        rf = RR.oracle_node()('lp', ru, R.Fixed(p['cut']), R.Fixed(p['q']))
        if which == 'resonant':
            return f, rf, V
        s = ext.Shaper(); s.get_state().table = p['curve']; s.input = f
        return s, SHR.oracle_node()(p['curve'], rf), V
    raise KeyError(which)


@functools.lru_cache(maxsize=None)
def wanted(which, kind, pos, N, U):
    """(the oracle's rows, the eager path's rows) of one case, shared by its routes"""
    from oracle import chain_ref as R
    p = draw()
    copies = None if U == 1 else p['copies16'][:U]
    _, ref, C = graph(which, p, kind, copies)
    want = R.render_stream(ref, pos, N, sum(KS), C)
    eager = stream(graph(which, p, kind, copies)[0], pos, N, sum(KS), C)
    want.setflags(write=False); eager.setflags(write=False)
    return want, eager


@contextlib.contextmanager
def launching(route):
    """attached images are process-wide and found by the program's words: only the specialised routes may launch them, so that the
    interpreted ones run the interpreter's own kernels (as tests/test_gpu_mixed.py does)"""
    from signals_amd import _native
    _native.voice_program_use_attached(route.endswith('specialise'))
    try:
        yield
    finally:
        _native.voice_program_use_attached(True)


def batches(top, channels, position, N, ks, route):
    with launching(route):
        return render_batches(top, channels, position, N, ks, names=True, check_status=True, **ROUTES[route])[:2]


#        patch, kind, block frames, copies, position, routes
THREE = ('per_node', 'always', 'specialise')
CASES = ([('bus', kind, N, 1, 0, THREE) for kind in KINDS for N in (64, 100, 256)]
         + [('lowpass', kind, N, U, HOUR, THREE) for kind, N, U in (('Sawtooth', 64, 7), ('Square', 100, 1), ('Sawtooth', 256, 1), ('Square', 256, 7))]
         + [('swept', 'Sawtooth', 256, 1, 0, THREE), ('swept', 'Square', 64, 7, HOUR, ('per_node', 'always')),
            ('resonant', 'Sawtooth', 256, 7, 0, ('per_node', 'always', 'mixed', 'mixed_specialise')),
            ('resonant', 'Sawtooth', 64, 1, HOUR, ('mixed', 'mixed_specialise')),
            ('resonant', 'Sawtooth', 100, 1, 0, ('mixed',)),
            ('shaped', 'Sawtooth', 256, 1, HOUR, ('per_node', 'mixed', 'mixed_specialise')),
            ('shaped', 'Sawtooth', 64, 7, 0, ('mixed',))])
LABEL = {'bus': 'voice_program_bus[OscSync]', 'lowpass': 'voice_program[OscSync,Filter]', 'swept': 'voice_program[OscSync,',
         'resonant': 'voice_program[OscSync,FilterQ]', 'shaped': 'voice_program[OscSync,FilterQ,Shape]'}


@pytest.mark.parametrize('which,kind,N,U,pos,route', [(*c[:5], r) for c in CASES for r in c[5]])
def test_routes(which, kind, N, U, pos, route):
    from signals_amd import specialise
    if route.endswith('specialise'):
        assert specialise.hipcc() is not None
    want, eager = wanted(which, kind, pos, N, U)
    p = draw()
    top, _, C = graph(which, p, kind, None if U == 1 else p['copies16'][:U])
    what = (which, kind, N, U, pos, route)
    tol = tolerance(want)
    err = maxerr(eager, f32(want))
    print('sync eager', what, 'max|err|', err, 'tol', tol)
    assert err <= tol, (what, err)
    got, names = batches(top, C, pos, N, KS, route)
    err = maxerr(got, f32(want))
    print('sync route', what, 'max|err|', err, 'tol', tol, sorted(names))
    programs = {n for n in names if n.startswith('voice_program')}
    if route == 'per_node' or (which in ('resonant', 'shaped') and route == 'always'):    # (two families without mixed_programs: one kernel per node)
        assert not programs and any(n.startswith('osc_bank_sync[' + kind) for n in names), (what, names)
        assert not any(n.startswith(('osc_bank_unison', 'osc_bank_blep')) for n in names), (what, names)
        if route == 'per_node':
            assert np.array_equal(got, eager), what                           # as the docstring of fuse=False promises
    else:
        assert len(programs) == 1 and next(iter(programs)).startswith(LABEL[which]), (what, names)          # ONE program, with the word
        assert ('*specialised' in next(iter(programs))) == route.endswith('specialise'), (what, names)
        assert not any(n.startswith(('osc_bank', 'biquad', 'shaper')) for n in names), (what, names)
    assert err <= tol, (what, err, tol)                                       # no sample excluded


def test_launches_of_each_route():
    from signals_amd.engine import BatchRenderer, KernelTimer
    p = draw()
    for route in ('per_node', 'default', 'always', 'specialise'):
        timer = KernelTimer()
        with launching(route):
            _, names, r = render_batches(graph('bus', p)[0], 2, 0, 256, (4,), timer=timer, names=True, **ROUTES.get(route, {}))
        if route == 'per_node':
            assert names == {'osc_bank_sync[Sawtooth]', 'sum_bus'}, names     # the per-node schedule: one kernel per node
        else:
            assert len(timer.records) == 1 and len(names) == 1, (route, names)            # ONE launch
            name = next(iter(names))
            assert name.startswith('voice_program_bus[OscSync]'), (route, names)
            assert ('*specialised' in name) == bool(r.specialise), (route, names)
    names = render_batches(graph('swept', p, 'Square')[0], V, 0, 256, (4,), names=True, fuse=False).names      # a swept ratio: per-block rows on the per-node schedule
    assert any(n.startswith('osc_bank_sync[Square,per-block]') for n in names), names
    timer = KernelTimer()                                                     # the resonant patch as ONE mixed launch
    with launching('mixed'):
        BatchRenderer(graph('resonant', p)[0], V, RATE, timer=timer, **ROUTES['mixed']).render(0, 256, 4)
        torch.cuda.synchronize()
    assert len(timer.records) == 1 and next(iter(timer.summary())).startswith('voice_program[OscSync,FilterQ]'), set(timer.summary())
    # a program without the word keeps its label and its family: the band-limited oscillator beside it
    from signals_amd.chain import ext
    b = ext.BlepSawtooth(); b.hertz = fix(p['hertz']); b.phase = fix(p['phase'])
    bus = ext.SumBus(); bus.input = b; bus.get_state().gains = np.ascontiguousarray(p['pan'])
    timer = KernelTimer()
    with launching('always'):
        BatchRenderer(bus, 2, RATE, timer=timer, fuse_program='always').render(0, 256, 4)
        torch.cuda.synchronize()
    assert set(timer.summary()) == {'voice_program_bus[OscBlep]'}, set(timer.summary())


def test_the_node_in_a_control_path_keeps_the_eager_path():
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    from signals_amd.engine import BatchRenderer, NotBatchable
    p = draw()
    slow = node('Square', None, np.array([[3.0]]), ratio=np.array([[2.5]]))
    g = fx.Gain(); g.left = mkosc('Sawtooth', p['hertz'], p['phase']); g.right = slow
    with pytest.raises(NotBatchable, match='SyncSquare in a control path: a unison oscillator'):
        BatchRenderer(g, V, RATE).render(0, 256, 2)
    got = stream(g, 0, 256, 2, V)                                             # the eager node serves the one-frame reads in float64
    ctl = np.concatenate([SR.sync('Square', [[0, 0]], b * 256, 1, [[3.0]], ratio=[[2.5]]) for b in range(2)])
    want = np.concatenate([f32(R.osc('Sawtooth', b * 256, 256, RATE, p['hertz'], p['phase'])).astype(np.float64) * ctl[b] for b in range(2)])
    assert maxerr(got, f32(want)) <= 1e-6


# ---------------------------------------------------------------------------------------------- state
@pytest.mark.parametrize('route', ['per_node', 'always', 'specialise'])
def test_edits_of_copies_and_of_the_ratio_change_the_next_render(route):
    from oracle import chain_ref as R
    from signals_amd.engine import BatchRenderer
    p = draw()
    N, K = 256, 3
    copies = p['copies16'][:7].copy()
    ratio = p['ratio'].copy()
    top, ref, C = graph('lowpass', p, 'Sawtooth', copies, ratio)
    source = top.input.sig.ratio.sig                                          # the Fixed that holds the ratio rows
    with launching(route):
        r = BatchRenderer(top, C, RATE, **ROUTES[route])
        first = r.render(0, N, K).cpu().numpy()
        want = R.render_stream(ref, 0, N, K, C)
        tol = tolerance(want)
        assert maxerr(first, f32(want)) <= tol, route
        copies[:, 0] *= 0.25                                                  # in place: the same array object
        copies[2, 1] = 0.125
        _, ref, _ = graph('lowpass', p, 'Sawtooth', copies, ratio)            # (a fresh oracle graph: no cached blocks of the old layout)
        r.reset()
        second = r.render(0, N, K).cpu().numpy()
        want2 = R.render_stream(ref, 0, N, K, C)
        ratio2 = ratio[:, ::-1].copy() + 0.5                                  # another ratio for every voice
        source.get_state().value = ratio2
        _, ref, _ = graph('lowpass', p, 'Sawtooth', copies, ratio2)
        r.reset()
        third = r.render(0, N, K).cpu().numpy()
    want3 = R.render_stream(ref, 0, N, K, C)
    assert maxerr(want2, want) > 1e-3 and maxerr(want3, want2) > 1e-3         # the edits are audible ...
    assert maxerr(second, f32(want2)) <= tol, (route, maxerr(second, f32(want2)))         # ... and the renders follow them
    assert maxerr(third, f32(want3)) <= tol, (route, maxerr(third, f32(want3)))


def test_one_specialised_image_serves_two_ratios(tmp_path, monkeypatch):
    from oracle import chain_ref as R
    from signals_amd import specialise
    from signals_amd.engine import BatchRenderer, KernelTimer
    assert specialise.hipcc() is not None
    specialise.forget()
    monkeypatch.setattr(specialise, 'CACHE', tmp_path)                        # an empty cache: every image built here is a file in it
    builds, real_build = [], specialise.build

    def counted(code, *rest):
        builds.append((tuple(code), *rest))
        return real_build(code, *rest)
    monkeypatch.setattr(specialise, 'build', counted)
    p = draw()
    N, K = 256, 3
    built = []
    for ratio in (p['ratio'], np.full((1, V), 5.125)):
        top, ref, C = graph('bus', p, 'Sawtooth', None, ratio)
        timer = KernelTimer()
        got = BatchRenderer(top, C, RATE, timer=timer, specialise=True).render(0, N, K).cpu().numpy()
        torch.cuda.synchronize()
        want = R.render_stream(ref, 0, N, K, C)
        assert maxerr(got, f32(want)) <= tolerance(want)
        assert set(timer.summary()) == {'voice_program_bus[OscSync]*specialised'}, set(timer.summary())
        built.append(sorted(f.name for f in tmp_path.glob('vp_*.hsaco')))
        assert len(builds) == 1 and [w[0] for w in builds[0][0]] == ['OscSync'], builds     # one build, at the first render
    assert len(built[0]) >= 1 and built[1] == built[0], built
    specialise.forget()


# ---------------------------------------------------------------------------------------------- the point of it
@pytest.mark.parametrize('ratio', [1.5, 2.0, 2.7, 3.3])
@pytest.mark.parametrize('kind', KINDS)
def test_the_aliasing_measurement_on_the_rendered_output(kind, ratio):
    """tests/test_sync_host.py's measurement (4096 frames, hertz = 48000 * 37 / 1024, phase 0.1234) on what the default route renders:
    at least 12 dB below the naive hard-synced waveform's ratio, and within 0.5 dB of the restatement's"""
    from signals_amd.engine import BatchRenderer
    hz, ph, ra = np.array([[RATE * 37 / 1024]]), np.array([[0.1234]]), np.array([[ratio]])
    got = BatchRenderer(node(kind, None, hz, ph, None, ra), 1, RATE).render(0, 256, 16).cpu().numpy()
    assert got.shape == (4096, 1) and got.dtype == np.float32
    want = SR.sync(kind, [[0, 0]], 0, 4096, hz, ph, ratio=ra)
    naive = SR.sync(kind, [[0, 0]], 0, 4096, hz, ph, ratio=ra, naive=True)
    got_db, ref_db, naive_db = SR.alias_ratio_db(got[:, 0]), SR.alias_ratio_db(want[:, 0]), SR.alias_ratio_db(naive[:, 0])
    print('alias / harmonic on the GPU', kind, ratio, got_db, 'restatement', ref_db, 'naive', naive_db)
    assert got_db <= naive_db - 12.0, (kind, ratio, got_db, naive_db)
    assert abs(got_db - ref_db) <= 0.5, (kind, ratio, got_db, ref_db)
    assert np.abs(got).max() <= 1.0 + 1e-6
