"""The table-lookup waveshaper on the GPU: sig_shaper_table against the numpy formula bit for bit, the eager node against
tests/shaper_reference.py, and the engine's routes (fuse=False, default, fuse_program='always', specialise=True) on six voice
shapes (and the bare Gain(Shaper(Sawtooth)), which pins the plain path bit for bit) from position 0 and from one hour, over two consecutive batches, blocks of 64 and 256 frames.

Tolerances.  The lookup is the definition's arithmetic, so the C ABI and the eager node (given its input's stored rows) are
compared with array_equal (float64, and float32(want) for the float32 store), no tolerance and no mask; steep and random tables
are used there, exactness does not depend on the slope.  fuse=False is bit-equal to the eager path everywhere.  The map is
piecewise linear and Lipschitz with L = max_i |tbl[i+1, w] - tbl[i, w]| (T - 1) / 2, so an error e on the shaper's input leaves at
most L e behind it: the eager path and the program routes are held to 1e-6 max(1, L) max(1, |want|_max) of float32(oracle), the
neighbouring tests' 1e-6 bar on the input (test_gpu_wavetable.py) carried through the map; L is computed here from the test
tables (tanh(3x)/tanh(3): about 3; the degree-3 Chebyshev polynomial: about 9; the folder: 2.5).  Program routes on graphs whose
shaper input is bit-exact (Sawtooth, Wavetable, Gain of those, the ADSR product; no filter, no bus, no LFO) are bit-equal to
float32(oracle) wherever the whole graph is one launch: the forced routes always; the default route renders the enveloped voice
as a program for Shaper(Gain(Sawtooth)) plus the envelope's own kernel (an envelope is outside the interpreter's small register
file), stores float32 between the two like the eager path, and is held to the tolerance there.  The LFO that sweeps `select` is read through floor(): the test asserts that no reference value lies within 1e-9
of an integer, so a last-bit difference of the LFO cannot pick another column.  The references are rendered once per
(graph, position, block size) and shared by the four routes."""
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import ROUTES_WITH_DEFAULT as ROUTES, dev, gpu_ready, render_batches
from helpers import HOUR, RATE, f32, fix, maxerr, mkosc, render, stream
import shaper_reference as SR
import wavetable_reference as WR

pytestmark = pytest.mark.gpu

V, KS = 200, (3, 3)


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


def inputs(rng, rows, voices, T, dtype, turn=0):
    """(rows, voices) of `dtype`: random values in [-1.5, 1.5], and in front of them as many of the special values as fit -- first
    the nine fixed ones (+-1 and their neighbours outside, +-inf, NaN, +-0), started at the `turn`-th so that shapes too small for
    all of them take different ones from call to call, then every knot"""
    x = rng.uniform(-1.5, 1.5, rows * voices).astype(dtype)
    one = dtype(1.0)
    fixed = np.array([1.0, -1.0, np.nextafter(one, dtype(2.0)), -np.nextafter(one, dtype(2.0)), np.inf, -np.inf, np.nan, 0.0, -0.0], dtype=dtype)
    special = np.concatenate([np.roll(fixed, -(turn % fixed.size)), SR.knots(T).astype(dtype)])
    n = min(special.size, x.size)
    x[:n] = special[:n]
    return x.reshape(rows, voices)


def select_rows(rng, blocks, width, W):
    s = rng.uniform(-1.5, W + 1.5, (blocks, width))                           # negatives, values >= W, fractional values ...
    s[:, ::7] = np.nan                                                        # ... and NaN
    s[:, 1::7] = np.floor(s[:, 1::7])
    return s


def same(got, want):
    return np.array_equal(got, want, equal_nan=True)


# ---------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize('T,W', [(2, 1), (5, 3), (2049, 7), (2, 8192)])
def test_shaper_table_matches_the_formula_bit_for_bit(T, W):
    """voices: one lane, a tail that is no multiple of 4, more than one 256-voice tile; rows: one, one row group, ragged"""
    from signals_amd import _native
    rng = np.random.default_rng(T + W)
    table = rng.uniform(-4, 4, (T, W))                                        # steep and random
    tab = dev(table, torch.float32)
    turn = 4 * T                                                              # (the one-sample shapes start at another fixed special from call to call)
    for voices in (1, 5, 260):
        sel = select_rows(rng, 1, voices, W)
        for rows in (1, 16, 300):
            for np_in, t_in in ((np.float32, torch.float32), (np.float64, torch.float64)):
                x = inputs(rng, rows, voices, T, np_in, turn)
                turn += 1
                want = SR.shaper(table, x.astype(np.float64), sel)
                assert np.isnan(want).any() == np.isnan(x).any()
                for t_out, cast in ((torch.float64, lambda a: a), (torch.float32, f32)):
                    out = torch.zeros((rows, voices), dtype=t_out, device='cuda:0')
                    _native.shaper_table(dev(x, t_in), dev(sel), tab, out)
                    assert same(out.cpu().numpy(), cast(want)), (T, W, voices, rows, np_in, t_out)


def test_shaper_table_broadcast_input_per_block_select_and_padding():
    from signals_amd import _native
    rng = np.random.default_rng(11)
    T, W = 2049, 7
    table = rng.uniform(-4, 4, (T, W))
    tab = dev(table, torch.float32)
    # a one-column input broadcast over the voices (vector stores, scalar loads), float32 and float64
    for voices in (5, 260):
        sel = select_rows(rng, 1, voices, W)
        for np_in, t_in in ((np.float32, torch.float32), (np.float64, torch.float64)):
            x = inputs(rng, 300, 1, T, np_in)
            out = torch.empty((300, voices), dtype=torch.float32, device='cuda:0')
            _native.shaper_table(dev(x, t_in), dev(sel), tab, out)
            assert same(out.cpu().numpy(), f32(SR.shaper(table, x.astype(np.float64), sel))), (voices, np_in)
    # per-block select rows (NaN, negative and >= W values): 500 rows in 5 blocks of 100, so the select row changes inside a wave's
    # 16 rows and the last wave is ragged; a padded output whose padding stays untouched; an input with a padded leading dimension
    for voices, pad in ((260, 4), (97, 3), (256, 0)):
        blocks, rows = 5, 500
        sel = select_rows(rng, blocks, voices, W)
        x = inputs(rng, rows, voices, T, np.float32)
        xbuf = torch.zeros((rows, voices + pad), dtype=torch.float32, device='cuda:0')
        xbuf[:, :voices] = dev(x, torch.float32)
        want = SR.shaper(table, x.astype(np.float64), sel, blocks=blocks)
        for t_out, cast in ((torch.float64, lambda a: a), (torch.float32, f32)):
            obuf = torch.zeros((rows, voices + pad), dtype=t_out, device='cuda:0')
            _native.shaper_table(xbuf[:, :voices], dev(sel), tab, obuf[:, :voices], rows_per_select=rows // blocks)
            assert not obuf[:, voices:].any(), (voices, pad)                  # the padding is not written
            assert same(obuf[:, :voices].cpu().numpy(), cast(want)), (voices, pad, t_out)
    # select unplugged (NULL): column 0; a one-column select row
    x = inputs(rng, 64, 96, T, np.float32)
    out = torch.empty((64, 96), dtype=torch.float32, device='cuda:0')
    _native.shaper_table(dev(x, torch.float32), None, tab, out)
    assert same(out.cpu().numpy(), f32(SR.shaper(table, x.astype(np.float64), 0.0)))
    _native.shaper_table(dev(x, torch.float32), dev([[3.0]]), tab, out)
    assert same(out.cpu().numpy(), f32(SR.shaper(table, x.astype(np.float64), [[3.0]])))


def test_many_row_groups_per_workgroup():
    """enough rows that a workgroup walks several row groups per wave with per-block select rows (the staging is paid once)"""
    from signals_amd import _native
    rng = np.random.default_rng(12)
    T, W, voices, N, K = 513, 3, 97, 100, 700                                # two voice tiles x 547 passes: two row groups per wave
    table = rng.uniform(-4, 4, (T, W))
    sel = select_rows(rng, K, voices, W)
    x = rng.uniform(-1.5, 1.5, (N * K, voices)).astype(np.float32)
    out = torch.empty((N * K, voices), dtype=torch.float32, device='cuda:0')
    _native.shaper_table(dev(x, torch.float32), dev(sel), dev(table, torch.float32), out, rows_per_select=N)
    assert same(out.cpu().numpy(), f32(SR.shaper(table, x.astype(np.float64), sel, blocks=K)))


# ---------------------------------------------------------------------------------------------- the eager node
def node(table, input_, select=None):
    from signals_amd.chain import ext
    s = ext.Shaper()
    if table is not None:
        s.get_state().table = table
    s.input = input_
    if select is not None:
        s.select = select if not isinstance(select, np.ndarray) else fix(select)
    return s


def driven_saw(hz, ph, drive):
    from signals_amd.chain import fx
    g = fx.Gain(); g.left = mkosc('Sawtooth', hz, ph); g.right = fix(drive)
    return g


def driven_saw_rows(pos, frames, hz, ph, drive):
    """the rows the eager Gain(Sawtooth) stores: float32 blocks, float64 one-frame replies"""
    from oracle import chain_ref as R
    cast = (lambda a: f32(a).astype(np.float64)) if frames > 1 else (lambda a: a)
    return cast(cast(R.osc('Sawtooth', pos, frames, RATE, hz, ph)) * drive)


@pytest.mark.parametrize('pos', [0, 50, HOUR])
def test_eager_node_against_the_reference(pos):
    rng = np.random.default_rng(8)
    hz, ph, drive = rng.uniform(55, 1760, (1, V)), rng.uniform(0, 1, (1, V)), np.array([[1.4]])
    for T, W in ((513, 3), (2, 1), (48, 5)):
        table = rng.uniform(-4, 4, (T, W))
        sel = select_rows(rng, 1, V, W)
        for frames in (256, 1):                                               # a block (float32) and a one-frame request (float64)
            x = driven_saw_rows(pos, frames, hz, ph, drive)
            got = render(node(table, driven_saw(hz, ph, drive), sel), pos, frames, V)
            want = SR.shaper(table, x, sel)
            assert got.shape == (frames, V) and got.dtype == (np.float32 if frames > 1 else np.float64)
            assert same(got, f32(want) if frames > 1 else want), (T, W, pos, frames)
            plain = render(node(table, driven_saw(hz, ph, drive)), pos, frames, V)          # unplugged select: column 0
            assert same(plain, render(node(table, driven_saw(hz, ph, drive), np.zeros((1, 1))), pos, frames, V))
            assert same(plain, f32(SR.shaper(table, x, 0.0)) if frames > 1 else SR.shaper(table, x, 0.0))


def test_an_integer_table_an_in_place_edit_and_the_default_hard_clip():
    hz, ph, drive = np.full((1, 8), 1000.0), np.zeros((1, 1)), np.array([[1.5]])
    table = np.array([[-2, -1], [0, 0], [2, 1]])                              # int64, what a .sigs value arrives as
    sel = np.array([[0.0, 1.0] * 4])
    s = node(table, driven_saw(hz, ph, drive), sel)
    assert same(render(s, 0, 128, 8), f32(SR.shaper(table, driven_saw_rows(0, 128, hz, ph, drive), sel)))
    table[1, 0] = 5                                                           # seen at the next reply (HostSnapshot)
    assert same(render(s, 128, 128, 8), f32(SR.shaper(table, driven_saw_rows(128, 128, hz, ph, drive), sel)))
    x = driven_saw_rows(0, 128, hz, ph, drive)
    got = render(node(None, driven_saw(hz, ph, drive)), 0, 128, 8)            # the default table: the identity on [-1, 1]
    assert same(got, f32(SR.shaper(np.array([[-1.0], [1.0]]), x)))
    assert np.abs(x).max() > 1.2 and np.abs(got).max() == 1.0
    assert maxerr(got, f32(np.clip(x, -1.0, 1.0))) <= 2.0 ** -24              # a hard clip: (c + 1) - 1 rounds at 2^-53, then the store


# ---------------------------------------------------------------------------------------------- graphs
def draw(seed=3):
    rng = np.random.default_rng(seed)
    th = rng.uniform(0, np.pi / 2, V)
    return dict(hertz=rng.uniform(55, 1760, (1, V)), phase=rng.uniform(0, 1, (1, V)), select=rng.uniform(-1, 4, (1, V)),
                wsel=rng.uniform(-1, 5, (1, V)), drive=rng.uniform(0.5, 1.6, (1, V)),
                cut1=rng.uniform(200, 8000, (1, V)), gain=rng.uniform(0.2, 1.0, (1, V)), pan=np.stack([np.cos(th), np.sin(th)]),
                env=dict(attack=rng.uniform(0.002, 0.02, (1, V)), decay=rng.uniform(0.01, 0.05, (1, V)), sustain=rng.uniform(0.3, 0.9, (1, V)),
                         release=rng.uniform(0.01, 0.05, (1, V)), gate_on=rng.uniform(0.0, 0.01, (1, V)), gate_off=rng.uniform(0.04, 0.07, (1, V))))


CURVES = np.concatenate([SR.tanh_curve(513, 3.0), SR.chebyshev_curve(513, 3), SR.fold_curve(513, 2.5)], axis=1)     # (513, 3)
L = SR.lipschitz(CURVES)
WAVES = np.concatenate([np.random.default_rng(0).uniform(-1, 1, (512, 3)), (2.0 * np.arange(512) / 512 - 1.0)[:, None]], axis=1)   # (512, 4)
LFO_HZ, LFO_DEPTH, LFO_CENTRE = 131.0, 1.2, 1.5          # (fast enough that six blocks of 64 frames visit every column)


def test_the_slopes_of_the_test_curves():
    assert abs(SR.lipschitz(CURVES[:, :1]) - 3.0 / np.tanh(3.0)) < 0.01 and 8.9 < SR.lipschitz(CURVES[:, 1:2]) <= 9.0
    assert abs(SR.lipschitz(CURVES[:, 2:]) - 2.5) < 1e-5 and L == SR.lipschitz(CURVES[:, 1:2])


def graph(which, p):
    """(GPU node, oracle node, rendered width, exact on the program routes) of one voice shape"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    RS = SR.oracle_node()
    saw = lambda: mkosc('Sawtooth', p['hertz'], p['phase'])
    rsaw = lambda: R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase']))
    if which in ('bus', 'lowpass_bus'):                                       # SumBus(Gain(Shaper(Sawtooth))), SumBus(Gain(Shaper(LowPass(Sawtooth)))), stereo
        src, rsrc = saw(), rsaw()
        if which == 'lowpass_bus':
            src = fx.LowPass(); src.input = saw(); src.cutoff = fix(p['cut1'])
            rsrc = R.Filter('lp', rsaw(), R.Fixed(p['cut1']))
        g = fx.Gain(); g.left = node(CURVES, src, p['select']); g.right = fix(p['gain'])
        b = ext.SumBus(); b.input = g; b.get_state().gains = np.ascontiguousarray(p['pan'])
        return b, R.SumBus(R.Binary('Gain', RS(CURVES, rsrc, R.Fixed(p['select'])), R.Fixed(p['gain'])), p['pan']), 2, False
    if which == 'plain':                                                      # Gain(Shaper(Sawtooth)), no bus: the plain Sawtooth path, bit for bit
        g = fx.Gain(); g.left = node(CURVES, saw(), p['select']); g.right = fix(p['gain'])
        return g, R.Binary('Gain', RS(CURVES, rsaw(), R.Fixed(p['select'])), R.Fixed(p['gain'])), V, True
    if which == 'filtered':                                                   # LowPass(Shaper(Sine)): the shaper supplies the filter's history rows
        f = fx.LowPass(); f.input = node(CURVES, mkosc('Sine', p['hertz'], p['phase']), p['select']); f.cutoff = fix(p['cut1'])
        rs = RS(CURVES, R.Osc('Sine', R.Fixed(p['hertz']), R.Fixed(p['phase'])), R.Fixed(p['select']))
        return f, R.Filter('lp', rs, R.Fixed(p['cut1'])), V, False
    if which == 'adsr':                                                       # Shaper(Gain(Sawtooth)) x ADSR: overdriven past +-1
        env = ext.ADSR()
        for name, row in p['env'].items():
            setattr(env, name, fix(row))
        g = fx.Gain(); g.left = saw(); g.right = fix(p['drive'])
        x = fx.RingMod(); x.left = node(CURVES, g, p['select']); x.right = env
        rs = RS(CURVES, R.Binary('Gain', rsaw(), R.Fixed(p['drive'])), R.Fixed(p['select']))
        return x, R.Binary('RingMod', rs, R.Adsr(**p['env'])), V, True
    if which == 'wavetable':                                                  # Shaper(Wavetable): both tables in one launch
        w = ext.Wavetable(); w.get_state().table = WAVES
        w.hertz = fix(p['hertz']); w.phase = fix(p['phase']); w.select = fix(p['wsel'])
        rw = WR.oracle_node()(WAVES, R.Fixed(p['hertz']), R.Fixed(p['phase']), R.Fixed(p['wsel']))
        return node(CURVES, w, p['select']), RS(CURVES, rw, R.Fixed(p['select'])), V, True
    if which == 'lfo':                                                        # select swept by an LFO: per-block rows, the control program
        def sweep():
            s = mkosc('Sine', [[LFO_HZ]])
            g = fx.Gain(); g.left = s; g.right = fix([[2.0 * LFO_DEPTH]])
            m = fx.Mix(); m.left = g; m.right = fix(2.0 * LFO_CENTRE + 0.01 * p['select']); m.mix = fix([[0.5]])
            return m
        rm = R.Binary('Mix', R.Binary('Gain', R.Osc('Sine', R.Fixed([[LFO_HZ]])), R.Fixed([[2.0 * LFO_DEPTH]])),
                      R.Fixed(2.0 * LFO_CENTRE + 0.01 * p['select']), R.Fixed([[0.5]]))
        g2 = fx.Gain(); g2.left = node(CURVES, saw(), sweep()); g2.right = fix(p['gain'])
        return g2, R.Binary('Gain', RS(CURVES, rsaw(), rm), R.Fixed(p['gain'])), V, False
    raise KeyError(which)


@functools.lru_cache(maxsize=None)
def wanted(which, pos, N):
    """(the oracle's rows, the eager path's rows) of one case, shared by the four routes"""
    from oracle import chain_ref as R
    p = draw()
    _, ref, C, _ = graph(which, p)
    want = R.render_stream(ref, pos, N, sum(KS), C)
    eager = stream(graph(which, p)[0], pos, N, sum(KS), C)
    want.setflags(write=False); eager.setflags(write=False)
    return want, eager


CASES = [(which, N) for which in ('bus', 'plain', 'lowpass_bus', 'filtered', 'adsr', 'wavetable', 'lfo') for N in (64, 256)]


@pytest.mark.parametrize('pos', [0, HOUR])
def test_the_swept_select_stays_clear_of_the_integers(pos):
    """what lets the 'lfo' graph be compared at all: floor(select) is the same for any value within 1e-9 of the reference's"""
    p = draw()
    for N in (64, 256):
        t = (pos + N * np.arange(sum(KS)))[:, None] / RATE
        sel = 0.5 * (2.0 * LFO_DEPTH * np.sin(2.0 * np.pi * LFO_HZ * t)) + 0.5 * (2.0 * LFO_CENTRE + 0.01 * p['select'])
        assert np.abs(sel - np.round(sel)).min() > 1e-9
        assert len(np.unique(np.clip(np.floor(sel), 0, 2))) == 3              # the sweep visits every column


@pytest.mark.parametrize('pos', [0, HOUR])
@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('which,N', CASES)
def test_routes(which, N, route, pos):
    from signals_amd import specialise
    if route == 'specialise':
        assert specialise.hipcc() is not None
    want, eager = wanted(which, pos, N)
    top, _, C, exact = graph(which, draw())
    got, names, _ = render_batches(top, C, pos, N, KS, names=True, **ROUTES[route])
    what = (which, N, route, pos)
    program = any(n.startswith('voice_program') for n in names)
    whole = program and all(n.startswith(('voice_program', 'control_program')) for n in names)     # one audio-rate launch, oscillator to stored rows
    tol = 1e-6 * max(1.0, L) * max(1.0, float(np.abs(want).max()))
    err = maxerr(eager, f32(want))
    print('shaper eager', what, 'max|err|', err, 'tol', tol)
    assert err <= tol, (what, err)                                            # (float32 between its nodes: never bit-equal to the oracle)
    if route == 'per_node':
        assert not program and np.array_equal(got, eager), what               # as the docstring of fuse=False promises
        assert any(n.startswith('shaper_table[Shaper') for n in names), names
        return
    assert program or route == 'default', (what, names)                       # forced routes run the program; the default follows worthwhile()
    if program:
        assert any('Shape' in n for n in names if n.startswith('voice_program')), names
    err = maxerr(got, f32(want))
    assert whole or route == 'default', (what, names)                         # forced routes: nothing per node beside the program
    print('shaper route', what, 'max|err|', err, 'tol', tol, 'exact' if exact and whole else '', 'program' if program else 'per node')
    if exact and whole:                                                       # (a kernel boundary stores float32 between the nodes)
        assert np.array_equal(got, f32(want)), (what, err)
    else:
        assert err <= tol, (what, err, tol)


def test_launches_of_each_route():
    p = draw()
    for route, kw in ROUTES.items():
        _, names, r = render_batches(graph('bus', p)[0], 2, 0, 256, (4,), names=True, **kw)
        if route == 'per_node':
            assert any(n.startswith('shaper_table[Shaper]') for n in names) and not any(n.startswith('voice_program') for n in names), names
        else:
            assert any(n.startswith('voice_program_bus[') and 'Shape' in n for n in names), (route, names)
            assert not any(n.startswith(('shaper_table', 'osc_bank', 'sum_bus')) for n in names), (route, names)
            assert any('*specialised' in n for n in names) == bool(r.specialise), (route, names)
    names = render_batches(graph('lfo', p)[0], V, 0, 256, (4,), names=True, fuse=False).names      # a swept select: per-block rows on the per-node schedule
    assert any(n.startswith('shaper_table[Shaper,per-block]') for n in names), names


@pytest.mark.parametrize('pos', [0, HOUR])
def test_a_band_filter_behind_a_shaper_renders_per_node(pos):
    """no interpreter variant has both instructions: no program holds the band filter, which runs as its own kernel over the shaper's
    stored rows on every route.  Those rows come from shaper_table wherever the filter needs history rows with them; a batch that
    needs none (the first one from position 0) may render the filter's input Shaper(Sawtooth) as a program of its own, as the
    engine does for any input subgraph"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    p = draw()
    RS = SR.oracle_node()
    low, high = p['cut1'] * 0.5, p['cut1'] * 0.5 + 900.0

    def build():
        bp = fx.BandPass(); bp.input = node(CURVES, mkosc('Sawtooth', p['hertz'], p['phase']), p['select']); bp.low = fix(low); bp.high = fix(high)
        return bp
    ref = R.BandFilter('bp', RS(CURVES, R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase'])), R.Fixed(p['select'])),
                       R.Fixed(low), R.Fixed(high))
    want = R.render_stream(ref, pos, 256, sum(KS), V)
    tol = 1e-6 * max(1.0, L) * max(1.0, float(np.abs(want).max()))
    for route in ROUTES:
        got, names, _ = render_batches(build(), V, pos, 256, (3, 3), names=True, **ROUTES[route])
        assert any(n.startswith('band_coldstart') for n in names) and any(n.startswith('shaper_table') for n in names), names
        assert not any(n.startswith('voice_program') and 'Band' in n for n in names), names
        if pos or route == 'per_node':
            assert not any(n.startswith('voice_program') for n in names), names
        err = maxerr(got, f32(want))
        print('shaper band', route, pos, 'max|err|', err, 'tol', tol)
        assert err <= tol, (route, pos, err, tol)


def test_a_shaper_in_a_control_path_keeps_the_eager_path():
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    from signals_amd.engine import BatchRenderer, NotBatchable
    p = draw()
    curve = SR.tanh_curve(513, 3.0)
    lfo = node(curve, mkosc('Sawtooth', [[3.0]]))                              # (a sawtooth LFO: exact arithmetic, so are the bits below)
    g = fx.Gain(); g.left = mkosc('Sawtooth', p['hertz'], p['phase']); g.right = lfo
    with pytest.raises(NotBatchable, match='waveshaper'):
        BatchRenderer(g, V, RATE).render(0, 256, 2)
    got = stream(g, 0, 256, 2, V)                                             # the eager node serves the one-frame reads in float64
    ctl = np.concatenate([SR.shape(curve, R.osc('Sawtooth', b * 256, 1, RATE, np.array([[3.0]]), np.zeros((1, 1)))) for b in range(2)])
    want = np.concatenate([f32(R.osc('Sawtooth', b * 256, 256, RATE, p['hertz'], p['phase'])).astype(np.float64) * ctl[b] for b in range(2)])
    assert np.array_equal(got, f32(want))
