"""Unison oscillators on the GPU: sig_osc_bank_unison against tests/unison_reference.py, one undetuned copy against sig_osc_bank's
bits, the eager node against the reference node, and the engine's routes (fuse=False, default, fuse_program='always',
specialise=True) on six voice shapes with fixed controls, two of them again with `spread` unplugged, and two with a swept spread / hertz, from position 0 and from one hour,
over two consecutive batches; which kernels each route launches, graphs the program refuses, edits of `copies` between renders and
the one specialised image that serves every detune layout.

Tolerances.  Every route computes the copies' phases with the definition's operations in the definition's order in float64
(-ffp-contract=off), so Square, Sawtooth and Triangle see the reference's own phase and no jump is crossed: no sample is excluded
anywhere.  The per-node kernel's float64 value in front of the store is numpy's for those three (bit-equal in both stores).  Sine:
the f64 store sums the f64 polynomial (< 1e-15, test_gpu_eager.py's bound for one oscillator; the mean cannot exceed it); the f32
store sums sig_osc_bank's hardware sine per copy, 1.3e-7 each (the project's bound for osc_sine_f32), the mean cannot exceed it,
and one more float32 rounding of a value in [-1, 1] adds 6e-8: <= 2e-7.  Graph routes: fuse=False is bit-equal to the eager path;
everything else within 1e-6 max(1, |ref|max), the neighbouring files' bar (test_gpu_wavetable.py, test_gpu_pm.py).
Inputs keep r = 1 + spread d > 0 and t >= 0 (hertz in [55, 1760], phase and p in [0, 1), d in [-0.12, 0.12], spread in [0, 1]),
which keeps v_fract_f64's corner (t in (-2^-54, 0)) out of every route."""
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import ROUTES_WITH_DEFAULT as ROUTES, dev, gpu_ready, lfo, render_batches, tolerance
from helpers import HOUR, RATE, f32, fix, maxerr, mkosc, render, stream
import unison_reference as UR

pytestmark = pytest.mark.gpu

KINDS = ('Sine', 'Square', 'Sawtooth', 'Triangle')
V = 96
KS = (4, 3)                                                                   # two consecutive batches


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


def draw_copies(rng, U):
    return np.stack([rng.uniform(-0.12, 0.12, U), rng.uniform(0, 1, U)], axis=1)


# ---------------------------------------------------------------------------------------------- C ABI
# (voices, padding of the leading dimension, parameter rows, rows): 500 rows in 5 blocks of 100: the parameter row changes inside a
# wave's 16 rows, and the last wave is ragged
ABI_SHAPES = ((256, 0, 1, 512), (256, 4, 4, 512), (97, 3, 1, 512), (97, 0, 4, 512), (256, 0, 5, 500), (97, 3, 5, 500))


@pytest.mark.parametrize('pos', [0, 50, HOUR])
@pytest.mark.parametrize('kind', KINDS)
def test_osc_bank_unison_matches_the_reference(kind, pos):
    from signals_amd import _native
    for V_, pad, blocks, rows in ABI_SHAPES:
        for U in (1, 2, 7, 16):
            rng = np.random.default_rng(U)
            hz, ph, sp = rng.uniform(55, 1760, (blocks, V_)), rng.uniform(0, 1, (blocks, V_)), rng.uniform(0, 1, (blocks, V_))
            copies = draw_copies(rng, U)
            rpp = rows // blocks
            want = UR.unison(kind, copies, pos, rpp, hz, ph, sp, blocks=blocks)
            for dtype in (torch.float64, torch.float32):
                what = (kind, pos, V_, pad, blocks, rows, U, dtype)
                obuf = torch.zeros((rows, V_ + pad), dtype=dtype, device='cuda:0')
                _native.osc_bank_unison(kind, pos, RATE, dev(hz), dev(ph), dev(sp), copies, obuf[:, :V_],
                                        rows_per_param=rpp if blocks > 1 else 0)
                got = obuf[:, :V_].cpu().numpy()
                assert not obuf[:, V_:].any(), what                           # the padding is not written
                if kind == 'Sine':
                    err, bound = maxerr(got, want), (1e-15 if dtype == torch.float64 else 2e-7)
                    print('sig_osc_bank_unison Sine', what, 'max|err|', err, 'bound', bound)
                    assert err < bound if dtype == torch.float64 else err <= bound, (what, err)
                else:
                    assert np.array_equal(got, want if dtype == torch.float64 else f32(want)), what


@pytest.mark.parametrize('kind', KINDS)
def test_one_undetuned_copy_gives_sig_osc_bank_bits(kind):
    from signals_amd import _native
    rng = np.random.default_rng(1)
    rows = 384
    hz, ph = dev(rng.uniform(55, 1760, (1, 256))), dev(rng.uniform(0, 1, (1, 256)))
    sp = dev(rng.uniform(0, 1, (1, 256)))
    one = np.array([[0.0, 0.0]])
    seven = draw_copies(rng, 7)
    for pos in (0, 50, HOUR):
        for dt in (torch.float32, torch.float64):
            new = lambda: torch.empty((rows, 256), dtype=dt, device='cuda:0')
            plain = _native.osc_bank(kind, pos, RATE, hz, ph, new())
            assert torch.equal(plain, _native.osc_bank_unison(kind, pos, RATE, hz, ph, sp, one, new())), (kind, pos, dt)
            assert torch.equal(plain, _native.osc_bank_unison(kind, pos, RATE, hz, ph, None, one, new())), (kind, pos, dt)
            unplugged = _native.osc_bank_unison(kind, pos, RATE, hz, ph, None, seven, new())
            zeros = _native.osc_bank_unison(kind, pos, RATE, hz, ph, dev(np.zeros((1, 256))), seven, new())
            assert torch.equal(unplugged, zeros), (kind, pos, dt)             # an unplugged spread is a spread of zeros


# ---------------------------------------------------------------------------------------------- the eager node
def node(kind, copies, hertz, phase=None, spread=None):
    from signals_amd.chain import ext
    u = getattr(ext, 'Unison' + kind)()
    if copies is not None:
        u.get_state().copies = copies
    u.hertz = hertz if not isinstance(hertz, np.ndarray) else fix(hertz)
    if phase is not None:
        u.phase = fix(phase)
    if spread is not None:
        u.spread = spread if not isinstance(spread, np.ndarray) else fix(spread)
    return u


@pytest.mark.parametrize('pos', [0, 50, HOUR])
@pytest.mark.parametrize('kind', KINDS)
def test_eager_node_against_the_reference(kind, pos):
    from oracle import chain_ref as R
    rng = np.random.default_rng(8)
    W = 200
    hz, ph, sp = rng.uniform(55, 1760, (1, W)), rng.uniform(0, 1, (1, W)), rng.uniform(0, 1, (1, W))
    for copies in (None, draw_copies(rng, 16)):                               # the default seven, and the most there can be
        ref = UR.UnisonOsc(kind, UR.default_copies() if copies is None else copies, R.Fixed(hz), R.Fixed(ph), R.Fixed(sp))
        for frames in (256, 1):                                               # a block (float32) and a one-frame request (float64)
            got = render(node(kind, copies, hz, ph, sp), pos, frames, W)
            want = R.render(ref, pos, frames, W)
            assert got.shape == (frames, W) and got.dtype == (np.float32 if frames > 1 else np.float64)
            if kind == 'Sine':
                assert maxerr(got, want) <= (2e-7 if frames > 1 else 1e-15), (kind, pos, frames)
            else:
                assert np.array_equal(got, f32(want) if frames > 1 else want), (kind, pos, frames)
    plain = render(node(kind, None, hz, ph), pos, 256, W)                     # unplugged spread: zeros, like every port
    assert np.array_equal(plain, render(node(kind, None, hz, ph, np.zeros((1, 1))), pos, 256, W))
    assert np.array_equal(render(node(kind, np.array([[0, 0]]), hz, ph, sp), pos, 256, W), render(mkosc(kind, hz, ph), pos, 256, W))


# ---------------------------------------------------------------------------------------------- graphs
def draw(seed=3):
    rng = np.random.default_rng(seed)
    th = rng.uniform(0, np.pi / 2, V)
    return dict(hertz=rng.uniform(55, 1760, (1, V)), phase=rng.uniform(0, 1, (1, V)), spread=rng.uniform(0, 1, (1, V)),
                cut1=rng.uniform(200, 8000, (1, V)), cut2=rng.uniform(200, 8000, (1, V)),
                gain=rng.uniform(0.2, 1.0, (1, V)), pan=np.stack([np.cos(th), np.sin(th)]), copies16=draw_copies(rng, 16),
                env=dict(attack=rng.uniform(0.002, 0.02, (1, V)), decay=rng.uniform(0.01, 0.05, (1, V)), sustain=rng.uniform(0.3, 0.9, (1, V)),
                         release=rng.uniform(0.01, 0.05, (1, V)), gate_on=rng.uniform(0.0, 0.01, (1, V)), gate_off=rng.uniform(0.04, 0.07, (1, V))))


def graph(which, p, kind='Sawtooth', copies=None):
    """(GPU node, oracle node, rendered width) of one voice shape; `copies`: the array both sides read (default: the node's seven)"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    held = UR.default_copies() if copies is None else copies                  # (the oracle reads the same array: edits reach both)
    u = node(kind, copies, p['hertz'], p['phase'], p['spread'])
    ru = UR.UnisonOsc(kind, held, R.Fixed(p['hertz']), R.Fixed(p['phase']), R.Fixed(p['spread']))
    if which == 'stored':                                                     # the bare node
        return u, ru, V
    if which in ('bus_unplugged', 'lowpass_unplugged'):                       # `spread` unplugged: zeros, the word's c = -1
        u = node(kind, copies, p['hertz'], p['phase'])
        ru = UR.UnisonOsc(kind, held, R.Fixed(p['hertz']), R.Fixed(p['phase']))
        which = which.split('_')[0]
    if which == 'bus':                                                        # under a stereo SumBus
        b = ext.SumBus(); b.input = u; b.get_state().gains = np.ascontiguousarray(p['pan'])
        return b, R.SumBus(ru, p['pan']), 2
    if which == 'lowpass':
        f = fx.LowPass(); f.input = u; f.cutoff = fix(p['cut1'])
        return f, R.Filter('lp', ru, R.Fixed(p['cut1'])), V
    if which == 'adsr':                                                       # RingMod with an ADSR
        env = ext.ADSR()
        for name, row in p['env'].items():
            setattr(env, name, fix(row))
        x = fx.RingMod(); x.left = u; x.right = env
        return x, R.Binary('RingMod', ru, R.Adsr(**p['env'])), V
    if which == 'cascade':                                                    # LowPass(LowPass(.))
        f1 = fx.LowPass(); f1.input = u; f1.cutoff = fix(p['cut1'])
        f2 = fx.LowPass(); f2.input = f1; f2.cutoff = fix(p['cut2'])
        return f2, R.Filter('lp', R.Filter('lp', ru, R.Fixed(p['cut1'])), R.Fixed(p['cut2'])), V
    if which == 'mix':                                                        # Mix with a plain osc.Sine
        mix = np.linspace(0.0, 1.0, V)[None, :]
        m = fx.Mix(); m.left = u; m.right = mkosc('Sine', p['hertz'] * 0.5, p['phase']); m.mix = fix(mix)
        return m, R.Binary('Mix', ru, R.Osc('Sine', R.Fixed(p['hertz'] * 0.5), R.Fixed(p['phase'])), R.Fixed(mix)), V
    if which in ('lfo_spread', 'lfo_hertz'):                                  # a control on a block-rate LFO, a Gain on top: two nodes, a program
        if which == 'lfo_spread':
            ctl, rctl = lfo(3.1, 0.4 * np.ones((1, V)), 0.5 * np.ones((1, V)))            # spread in [0.1, 0.9]
            u = node(kind, copies, p['hertz'], p['phase'], ctl)
            ru = UR.UnisonOsc(kind, held, R.Fixed(p['hertz']), R.Fixed(p['phase']), rctl)
        else:
            ctl, rctl = lfo(3.1, 0.02 * p['hertz'], p['hertz'])               # a vibrato of 2 %
            u = node(kind, copies, ctl, p['phase'], p['spread'])
            ru = UR.UnisonOsc(kind, held, rctl, R.Fixed(p['phase']), R.Fixed(p['spread']))
        g = fx.Gain(); g.left = u; g.right = fix(p['gain'])
        return g, R.Binary('Gain', ru, R.Fixed(p['gain'])), V
    raise KeyError(which)


@functools.lru_cache(maxsize=None)
def wanted(which, kind, pos, N):
    """(the oracle's rows, the eager path's rows) of one case, shared by the four routes"""
    from oracle import chain_ref as R
    p = draw()
    _, ref, C = graph(which, p, kind)
    want = R.render_stream(ref, pos, N, sum(KS), C)
    eager = stream(graph(which, p, kind)[0], pos, N, sum(KS), C)
    want.setflags(write=False); eager.setflags(write=False)
    return want, eager


FIXED = ([('stored', kind, N) for kind in KINDS for N in (64, 256)]
         + [(which, kind, N) for which, kind in (('bus', 'Sawtooth'), ('lowpass', 'Sawtooth'), ('adsr', 'Square'), ('mix', 'Triangle'))
            for N in (64, 256)] + [('cascade', 'Sawtooth', 256), ('bus_unplugged', 'Sawtooth', 256), ('lowpass_unplugged', 'Square', 256)])
SWEPT = [(which, kind, N) for which in ('lfo_spread', 'lfo_hertz') for kind in ('Sine', 'Triangle') for N in (64, 256)]


@pytest.mark.parametrize('pos', [0, HOUR])
@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('which,kind,N', FIXED + SWEPT)
def test_routes(which, kind, N, route, pos):
    from signals_amd import specialise
    if route == 'specialise':
        assert specialise.hipcc() is not None
    want, eager = wanted(which, kind, pos, N)
    top, _, C = graph(which, draw(), kind)
    got, names, _ = render_batches(top, C, pos, N, KS, names=True, **ROUTES[route])
    what = (which, kind, N, route, pos)
    program = any(n.startswith('voice_program') for n in names)
    tol = tolerance(want)
    err = maxerr(eager, f32(want))
    print('unison eager', what, 'max|err|', err, 'tol', tol)
    assert err <= tol, (what, err)
    if route == 'per_node':
        assert not program and any(n.startswith('osc_bank_unison') for n in names), (what, names)
        assert np.array_equal(got, eager), what                               # as the docstring of fuse=False promises
        if which == 'stored' and kind != 'Sine':
            assert np.array_equal(got, f32(want)), what                       # the kernel's float64 value is numpy's
        return
    if which != 'stored':                                                     # (a single node stays its own kernel on every route)
        assert program or route == 'default', (what, names)                   # forced routes run the program; the default follows worthwhile()
    if which.endswith('_unplugged'):
        assert program, (what, names)                                         # small programs: the handler's c = -1 branch ran
    err = maxerr(got, f32(want))
    print('unison route', what, 'max|err|', err, 'tol', tol, 'program' if program else 'per node')
    assert err <= tol, (what, err, tol)                                       # no sample excluded


# ---------------------------------------------------------------------------------------------- what ran
def test_launches_of_each_route():
    from signals_amd.engine import KernelTimer
    p = draw()
    for route, kw in ROUTES.items():
        timer = KernelTimer()
        _, names, r = render_batches(graph('bus', p)[0], 2, 0, 256, (4,), timer=timer, names=True, **kw)
        if route == 'per_node':
            assert names == {'osc_bank_unison[Sawtooth]', 'sum_bus'}, names   # the per-node schedule
        else:
            assert len(timer.records) == 1 and len(names) == 1, (route, names)            # ONE launch
            name = next(iter(names))
            assert name.startswith('voice_program_bus[OscUni]'), (route, names)
            assert ('*specialised' in name) == bool(r.specialise), (route, names)         # (SIG_SPECIALISE=1 turns it on for every route)
    names = render_batches(graph('lfo_spread', p, 'Sine')[0], V, 0, 256, (4,), names=True, fuse=False).names      # a swept spread: per-block rows on the per-node schedule
    assert any(n.startswith('osc_bank_unison[Sine,per-block]') for n in names), names


@pytest.mark.parametrize('pos', [0, HOUR])
def test_a_band_filter_behind_a_unison_oscillator_renders_per_node(pos):
    """no interpreter variant has both instructions: the engine keeps the graph one kernel per node, on every route"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    p = draw()
    low, high = p['cut1'] * 0.5, p['cut1'] * 0.5 + 900.0

    def build():
        bp = fx.BandPass(); bp.input = graph('stored', p)[0]; bp.low = fix(low); bp.high = fix(high)
        return bp
    want = R.render_stream(R.BandFilter('bp', graph('stored', p)[1], R.Fixed(low), R.Fixed(high)), pos, 256, sum(KS), V)
    tol = tolerance(want)
    for route, kw in ROUTES.items():
        got, names, _ = render_batches(build(), V, pos, 256, KS, names=True, **kw)
        assert any(n.startswith('osc_bank_unison') for n in names) and not any(n.startswith('voice_program') for n in names), (route, names)
        err = maxerr(got, f32(want))
        assert err <= tol, (route, pos, err, tol)


def test_a_unison_oscillator_in_a_control_path_keeps_the_eager_path():
    from signals_amd.chain import fx
    from signals_amd.engine import BatchRenderer, NotBatchable
    p = draw()
    slow = node('Triangle', None, np.array([[3.0]]))
    g = fx.Gain(); g.left = mkosc('Sawtooth', p['hertz'], p['phase']); g.right = slow
    with pytest.raises(NotBatchable, match='unison oscillator'):
        BatchRenderer(g, V, RATE).render(0, 256, 2)
    got = stream(g, 0, 256, 2, V)                                             # the eager node serves the one-frame reads in float64
    from oracle import chain_ref as R
    ctl = np.concatenate([UR.unison('Triangle', UR.default_copies(), b * 256, 1, [[3.0]]) for b in range(2)])
    want = np.concatenate([f32(R.osc('Sawtooth', b * 256, 256, RATE, p['hertz'], p['phase'])).astype(np.float64) * ctl[b] for b in range(2)])
    assert np.array_equal(got, f32(want))


# ---------------------------------------------------------------------------------------------- state
@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('which', ['bus', 'lowpass'])
def test_an_in_place_edit_of_copies_changes_the_next_render(which, route):
    """the copies travel by value with each launch: the second render reads the edited array, on every route"""
    from oracle import chain_ref as R
    from signals_amd.engine import BatchRenderer
    p = draw()
    N, K = 256, 3
    copies = p['copies16'][:7].copy()
    top, ref, C = graph(which, p, 'Sawtooth', copies)
    r = BatchRenderer(top, C, RATE, **ROUTES[route])
    first = r.render(0, N, K).cpu().numpy()
    want = R.render_stream(ref, 0, N, K, C)
    tol = tolerance(want)
    assert maxerr(first, f32(want)) <= tol, (which, route)
    copies[:, 0] *= 0.25                                                      # in place: the same array object
    copies[2, 1] = 0.125
    _, ref, _ = graph(which, p, 'Sawtooth', copies)                           # (a fresh oracle graph: no cached blocks of the old layout)
    r.reset()
    second = r.render(0, N, K).cpu().numpy()
    want2 = R.render_stream(ref, 0, N, K, C)
    assert maxerr(want2, want) > 1e-3                                         # the edit is audible ...
    assert maxerr(second, f32(want2)) <= tol, (which, route, maxerr(second, f32(want2)))  # ... and the render follows it
    # a replaced array likewise
    other = p['copies16'][7:12].copy()
    top.input.sig.get_state().copies = other
    _, ref, _ = graph(which, p, 'Sawtooth', other)
    r.reset()
    third = r.render(0, N, K).cpu().numpy()
    assert maxerr(third, f32(R.render_stream(ref, 0, N, K, C))) <= tol, (which, route)


def test_one_specialised_image_serves_every_detune_layout(tmp_path, monkeypatch):
    """the image is built from the program's words, not from the copies: two layouts of equal U -- and one of another U -- share it:
    specialise.build runs once, for the first render"""
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
    for copies in (p['copies16'][:7].copy(), p['copies16'][7:14].copy(), p['copies16'][:3].copy()):
        top, ref, C = graph('bus', p, 'Sawtooth', copies)
        timer = KernelTimer()
        got = BatchRenderer(top, C, RATE, timer=timer, specialise=True).render(0, N, K).cpu().numpy()
        torch.cuda.synchronize()
        want = R.render_stream(ref, 0, N, K, C)
        assert maxerr(got, f32(want)) <= tolerance(want)
        assert set(timer.summary()) == {'voice_program_bus[OscUni]*specialised'}, set(timer.summary())     # the launch log: the image ran
        built.append(sorted(f.name for f in tmp_path.glob('vp_*.hsaco')))
        assert len(builds) == 1 and builds[0][0] == (('OscUni', 2, 0, 0, 0),), builds      # one build, at the first render, none after
    assert len(built[0]) >= 1 and built[1] == built[0] and built[2] == built[0], built    # no new image after the first render
    specialise.forget()
