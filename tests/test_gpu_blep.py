"""Band-limited oscillators on the GPU: sig_osc_bank_blep against tests/blep_reference.py in both stores, one undetuned copy
against sig_osc_bank's bits outside the correction windows, and every render route (the eager nodes, fuse=False, the interpreted
program, the specialised one, the mixed interpreter and the mixed specialised image) against the oracle graph, with the launch
labels of each; the node in a control path, edits of `copies` between renders, the one specialised image that serves every copies
array, and the aliasing measurement of tests/test_blep_host.py on what the GPU rendered.

Tolerances.  sig_osc_bank_blep shares the restatement's phase t bit for bit (the unison oscillator's operations in its order,
-ffp-contract=off) and its m = mod(t, 1), so both choose the same window for every sample.  Inside one the kernel multiplies by a
rounded 1 / d where the restatement divides: a relative error <= 3e-16 on x in [0, 1]; the polynomials have slope <= 3, and the
mean over the copies cannot amplify: 1e-14 for the f64 store is about 45 ulp of headroom, derived and not measured.  The f32 store
adds one float32 rounding of a value in [-1, 1] (6e-8): within 2e-7 max(1, |ref|), the unison Sine's bound.  Graph routes: 1e-6
max(1, |ref|max), the neighbouring files' bar; the corrected waveform is continuous, so no sample is excluded anywhere.

Inputs that reach where the kernel can go wrong, in every case's first voices: rate / 64 at phase 0 (m = 0 and m = 1/2 hit exactly),
a negative pitch, 0 Hz (d = 0: no window, 1 / d = inf behind a select), 1e-3 Hz (1 / d = 4.8e7), 30 kHz (above rate / 2: d clamped),
13 kHz (the Square's windows overlap), then musical pitches."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import dev, gpu_ready, lfo, render_batches, tolerance
from helpers import HOUR, RATE, f32, fix, maxerr, mkosc, stream
import blep_reference as BR
import resonant_reference as RR

pytestmark = pytest.mark.gpu

KINDS = ('Square', 'Sawtooth', 'Triangle')
V = 97                                                                        # no multiple of 64, of 4 (the voice tile) or of 2
KS = (2, 1)                                                                   # K = 3 blocks in two consecutive batches
NEAR_2_31 = 2 ** 31 - 100                                                     # just under 2^31: the rows cross it
SPECIAL = (RATE / 64, -440.0, 0.0, 1e-3, 30000.0, 13000.0, 27.5, 261.6255653005986, 4186.009044809578)
ROUTES = {'per_node': {'fuse': False}, 'always': {'fuse_program': 'always'}, 'specialise': {'specialise': True},
          'mixed': {'mixed_programs': True, 'fuse_program': 'always'}, 'mixed_specialise': {'mixed_programs': True, 'specialise': True}}


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    from signals_amd import _native
    gpu_ready()
    yield
    _native.voice_program_use_attached(True)


def rows_of(rng, blocks, width):
    """hertz, phase rows (blocks, width): the special pitches first (rate / 64 at phase 0), random musical ones behind them; with
    several blocks every row is modulated a little (a per-block hertz)"""
    hz = rng.uniform(55, 1760, (blocks, width))
    ph = rng.uniform(0, 1, (blocks, width))
    hz[:, :len(SPECIAL)] = np.array(SPECIAL)[None, :] * (1.0 + 0.01 * np.arange(blocks))[:, None]
    hz[0, :len(SPECIAL)] = SPECIAL
    ph[:, 0] = 0.0
    return hz, ph


def draw_copies(rng, U):
    c = np.stack([rng.uniform(-0.12, 0.12, U), rng.uniform(0, 1, U)], axis=1)
    c[0] = 0.0                                                                # copy 0 keeps the exact hits
    return c


# ---------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize('pos', [0, NEAR_2_31, HOUR])
@pytest.mark.parametrize('kind', KINDS)
def test_osc_bank_blep_matches_the_restatement(kind, pos):
    """300 rows in 3 blocks of 100: the parameter row changes inside a wave's 16 rows and the last wave is ragged; 97 voices with a
    padded leading dimension (one voice per lane) and 96 (four per lane, vector stores)"""
    from signals_amd import _native
    for V_, pad, blocks, rows in ((97, 3, 3, 300), (96, 0, 3, 300), (97, 0, 1, 256)):
        for U in (1, 7, 16):
            rng = np.random.default_rng(U)
            (hz, ph), sp = rows_of(rng, blocks, V_), rng.uniform(0, 1, (blocks, V_))
            copies = draw_copies(rng, U)
            rpp = rows // blocks
            want = BR.blep(kind, copies, pos, rpp, hz, ph, sp, blocks=blocks)
            assert np.isfinite(want).all()
            for dtype in (torch.float64, torch.float32):
                what = (kind, pos, V_, pad, blocks, U, dtype)
                obuf = torch.zeros((rows, V_ + pad), dtype=dtype, device='cuda:0')
                _native.osc_bank_blep(kind, pos, RATE, dev(hz), dev(ph), dev(sp), copies, obuf[:, :V_], rows_per_param=rpp if blocks > 1 else 0)
                got = obuf[:, :V_].cpu().numpy()
                assert not obuf[:, V_:].any(), what                           # the padding is not written
                if dtype == torch.float64:
                    err = maxerr(got, want)
                    print('sig_osc_bank_blep f64', what, 'max|err|', err, 'bound 1e-14')
                    assert err <= 1e-14, (what, err)
                else:
                    err = float(np.max(np.abs(got.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))))
                    print('sig_osc_bank_blep f32', what, 'max|err| / max(1, |ref|)', err, 'bound 2e-7')
                    assert err <= 2e-7, (what, err)


@pytest.mark.parametrize('kind', KINDS)
def test_one_copy_outside_every_window_gives_sig_osc_bank_bits(kind):
    from oracle import chain_ref as R
    from signals_amd import _native
    rng = np.random.default_rng(1)
    rows, W = 304, 256
    hz, ph = rows_of(rng, 1, W)
    one = np.array([[0.0, 0.0]])
    for pos in (0, NEAR_2_31, HOUR):
        inside = BR.in_window(kind, R.frame_range(pos, rows) / RATE * hz + ph, BR.increment(hz, RATE))
        assert 0.005 < inside.mean() < 0.5
        for dt in (torch.float32, torch.float64):
            new = lambda: torch.empty((rows, W), dtype=dt, device='cuda:0')
            plain = _native.osc_bank(kind, pos, RATE, dev(hz), dev(ph), new()).cpu().numpy()
            got = _native.osc_bank_blep(kind, pos, RATE, dev(hz), dev(ph), None, one, new()).cpu().numpy()
            assert np.array_equal(got[~inside], plain[~inside]), (kind, pos, dt)
            assert not np.array_equal(got[inside], plain[inside]), (kind, pos, dt)
            spread = _native.osc_bank_blep(kind, pos, RATE, dev(hz), dev(ph), dev(rng.uniform(0, 1, (1, W))), one, new()).cpu().numpy()
            assert np.array_equal(spread, got), (kind, pos, dt)               # no detune: the spread multiplies a zero


# ---------------------------------------------------------------------------------------------- graphs
def node(kind, copies, hertz, phase=None, spread=None):
    from signals_amd.chain import ext
    u = getattr(ext, 'Blep' + kind)()
    if copies is not None:
        u.get_state().copies = copies
    u.hertz = hertz if not isinstance(hertz, np.ndarray) else fix(hertz)
    if phase is not None:
        u.phase = fix(phase)
    if spread is not None:
        u.spread = spread if not isinstance(spread, np.ndarray) else fix(spread)
    return u


def draw(seed=3):
    rng = np.random.default_rng(seed)
    th = rng.uniform(0, np.pi / 2, V)
    hz, ph = rows_of(rng, 1, V)
    return dict(hertz=hz, phase=ph, spread=rng.uniform(0, 1, (1, V)), cut=rng.uniform(200, 8000, (1, V)), q=rng.uniform(0.6, 2.0, (1, V)),
                pan=np.stack([np.cos(th), np.sin(th)]), copies16=draw_copies(rng, 16))


def graph(which, p, kind='Sawtooth', copies=None):
    """(GPU node, oracle node, rendered width); `copies`: the array both sides read (default: the node's one clean copy)"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    held = BR.default_copies() if copies is None else copies
    u = node(kind, copies, p['hertz'], p['phase'], p['spread'])
    ru = BR.BlepOsc(kind, held, R.Fixed(p['hertz']), R.Fixed(p['phase']), R.Fixed(p['spread']))
    if which == 'swept':                                                      # spread and hertz on block-rate LFOs, a Gain on top
        (sp, rsp), (hz, rhz) = lfo(3.1, 0.4 * np.ones((1, V)), 0.5 * np.ones((1, V))), lfo(2.3, 0.02 * p['hertz'], p['hertz'])
        u = node(kind, copies, hz, p['phase'], sp)
        ru = BR.BlepOsc(kind, held, rhz, R.Fixed(p['phase']), rsp)
        g = fx.Gain(); g.left = u; g.right = fix(p['q'])
        return g, R.Binary('Gain', ru, R.Fixed(p['q'])), V
    if which == 'bus':                                                        # bare under a stereo SumBus
        b = ext.SumBus(); b.input = u; b.get_state().gains = np.ascontiguousarray(p['pan'])
        return b, R.SumBus(ru, p['pan']), 2
    if which == 'lowpass':
        f = fx.LowPass(); f.input = u; f.cutoff = fix(p['cut'])
        return f, R.Filter('lp', ru, R.Fixed(p['cut'])), V
    if which == 'resonant':                                                   # two families: a mixed program, or one kernel per node
        f = ext.ResonantLowPass(); f.input = u; f.cutoff = fix(p['cut']); f.resonance = fix(p['q'])
        return f, RR.oracle_node()('lp', ru, R.Fixed(p['cut']), R.Fixed(p['q'])), V
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
CASES = ([('bus', kind, 256, 1, 0, ('per_node', 'always', 'specialise')) for kind in KINDS]
         + [('lowpass', kind, 256, 7, HOUR, ('per_node', 'always', 'specialise')) for kind in KINDS]
         + [('lowpass', 'Sawtooth', 64, 16, NEAR_2_31, ('per_node', 'always', 'specialise')),     # N below the filter context
            ('bus', 'Square', 64, 7, HOUR, ('always', 'specialise')),
            ('swept', 'Triangle', 256, 7, 0, ('per_node', 'always', 'specialise')),
            ('swept', 'Sawtooth', 64, 1, HOUR, ('per_node', 'always')),
            ('resonant', 'Sawtooth', 256, 7, 0, ('per_node', 'always', 'mixed', 'mixed_specialise')),
            ('resonant', 'Square', 64, 1, HOUR, ('mixed', 'mixed_specialise')),
            ('resonant', 'Triangle', 256, 16, NEAR_2_31, ('mixed', 'mixed_specialise'))])
LABEL = {'bus': 'voice_program_bus[OscBlep]', 'lowpass': 'voice_program[OscBlep,Filter]', 'swept': 'voice_program[OscBlep,',
         'resonant': 'voice_program[OscBlep,FilterQ]'}


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
    print('blep eager', what, 'max|err|', err, 'tol', tol)
    assert err <= tol, (what, err)
    got, names = batches(top, C, pos, N, KS, route)
    err = maxerr(got, f32(want))
    print('blep route', what, 'max|err|', err, 'tol', tol, sorted(names))
    programs = {n for n in names if n.startswith('voice_program')}
    if route == 'per_node' or (which == 'resonant' and route == 'always'):    # (two families without mixed_programs: one kernel per node)
        assert not programs and any(n.startswith('osc_bank_blep[' + kind) for n in names), (what, names)
        assert not any(n.startswith('osc_bank_unison') for n in names), (what, names)
        if route == 'per_node':
            assert np.array_equal(got, eager), what                           # as the docstring of fuse=False promises
    else:
        assert len(programs) == 1 and next(iter(programs)).startswith(LABEL[which]), (what, names)          # ONE program, with the word
        assert ('*specialised' in next(iter(programs))) == route.endswith('specialise'), (what, names)
        assert not any(n.startswith(('osc_bank_blep', 'osc_bank_unison', 'biquad')) for n in names), (what, names)
    assert err <= tol, (what, err, tol)                                       # no sample excluded


def test_launches_of_each_route():
    from signals_amd.engine import BatchRenderer, KernelTimer
    p = draw()
    for route in ('per_node', 'default', 'always', 'specialise'):
        timer = KernelTimer()
        with launching(route):
            _, names, r = render_batches(graph('bus', p)[0], 2, 0, 256, (4,), timer=timer, names=True, **ROUTES.get(route, {}))
        if route == 'per_node':
            assert names == {'osc_bank_blep[Sawtooth]', 'sum_bus'}, names     # the per-node schedule
        else:
            assert len(timer.records) == 1 and len(names) == 1, (route, names)            # ONE launch
            name = next(iter(names))
            assert name.startswith('voice_program_bus[OscBlep]'), (route, names)
            assert ('*specialised' in name) == bool(r.specialise), (route, names)
    names = render_batches(graph('swept', p, 'Square')[0], V, 0, 256, (4,), names=True, fuse=False).names      # swept controls: per-block rows on the per-node schedule
    assert any(n.startswith('osc_bank_blep[Square,per-block]') for n in names), names


def test_the_node_in_a_control_path_keeps_the_eager_path():
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    from signals_amd.engine import BatchRenderer, NotBatchable
    p = draw()
    slow = node('Triangle', None, np.array([[3.0]]))
    g = fx.Gain(); g.left = mkosc('Sawtooth', p['hertz'], p['phase']); g.right = slow
    with pytest.raises(NotBatchable, match='unison oscillator'):
        BatchRenderer(g, V, RATE).render(0, 256, 2)
    got = stream(g, 0, 256, 2, V)                                             # the eager node serves the one-frame reads in float64
    ctl = np.concatenate([BR.blep('Triangle', [[0, 0]], b * 256, 1, [[3.0]]) for b in range(2)])
    want = np.concatenate([f32(R.osc('Sawtooth', b * 256, 256, RATE, p['hertz'], p['phase'])).astype(np.float64) * ctl[b] for b in range(2)])
    assert maxerr(got, f32(want)) <= 1e-6                                     # (the control is within 1e-14 of the restatement's)


# ---------------------------------------------------------------------------------------------- state
@pytest.mark.parametrize('route', ['per_node', 'always', 'specialise'])
def test_an_in_place_edit_of_copies_changes_the_next_render(route):
    from oracle import chain_ref as R
    from signals_amd.engine import BatchRenderer
    p = draw()
    N, K = 256, 3
    copies = p['copies16'][:7].copy()
    top, ref, C = graph('lowpass', p, 'Sawtooth', copies)
    with launching(route):
        r = BatchRenderer(top, C, RATE, **ROUTES[route])
        first = r.render(0, N, K).cpu().numpy()
        want = R.render_stream(ref, 0, N, K, C)
        tol = tolerance(want)
        assert maxerr(first, f32(want)) <= tol, route
        copies[:, 0] *= 0.25                                                  # in place: the same array object
        copies[2, 1] = 0.125
        _, ref, _ = graph('lowpass', p, 'Sawtooth', copies)                   # (a fresh oracle graph: no cached blocks of the old layout)
        r.reset()
        second = r.render(0, N, K).cpu().numpy()
    want2 = R.render_stream(ref, 0, N, K, C)
    assert maxerr(want2, want) > 1e-3                                         # the edit is audible ...
    assert maxerr(second, f32(want2)) <= tol, (route, maxerr(second, f32(want2)))         # ... and the render follows it


def test_one_specialised_image_serves_two_copies_arrays(tmp_path, monkeypatch):
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
    for copies in (p['copies16'][:7].copy(), p['copies16'][7:10].copy()):     # another layout, another count
        top, ref, C = graph('bus', p, 'Sawtooth', copies)
        timer = KernelTimer()
        got = BatchRenderer(top, C, RATE, timer=timer, specialise=True).render(0, N, K).cpu().numpy()
        torch.cuda.synchronize()
        want = R.render_stream(ref, 0, N, K, C)
        assert maxerr(got, f32(want)) <= tolerance(want)
        assert set(timer.summary()) == {'voice_program_bus[OscBlep]*specialised'}, set(timer.summary())
        built.append(sorted(f.name for f in tmp_path.glob('vp_*.hsaco')))
        assert len(builds) == 1 and builds[0][0] == (('OscBlep', 2, 0, 0, 0),), builds     # one build, at the first render
    assert len(built[0]) >= 1 and built[1] == built[0], built
    specialise.forget()


# ---------------------------------------------------------------------------------------------- the point of it
@pytest.mark.parametrize('kind', KINDS)
def test_the_aliasing_measurement_on_the_rendered_output(kind):
    """tests/test_blep_host.py's measurement (4096 frames from position 1000, hertz = 48000 * 37 / 1024, phase 0.1234) on what the
    default route renders, against the restatement's ratio: within 0.5 dB"""
    from signals_amd.engine import BatchRenderer
    hz, ph = np.array([[RATE * 37 / 1024]]), np.array([[0.1234]])
    got = BatchRenderer(node(kind, None, hz, ph), 1, RATE).render(1000, 256, 16).cpu().numpy()
    assert got.shape == (4096, 1) and got.dtype == np.float32
    want = BR.blep(kind, [[0, 0]], 1000, 4096, hz, ph)
    ratio, ref_ratio = BR.alias_ratio_db(got[:, 0]), BR.alias_ratio_db(want[:, 0])
    print('alias / harmonic on the GPU', kind, ratio, 'restatement', ref_ratio)
    assert abs(ratio - ref_ratio) <= 0.5, (kind, ratio, ref_ratio)
    assert np.abs(got).max() <= 1.0
