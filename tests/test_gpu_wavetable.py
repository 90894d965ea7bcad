"""The wavetable oscillator on the GPU: sig_osc_bank_table against the numpy formula bit for bit, the eager node against
tests/wavetable_reference.py, and the engine's routes (fuse=False, default, fuse_program='always', specialise=True) on six voice
shapes from position 0 and from one hour, over two consecutive batches, blocks of 64 and 256 frames.

Tolerances.  The lookup is the definition's arithmetic, so the C ABI and the eager node are compared with array_equal (float64,
and float32(want) for the float32 store), no tolerance and no mask.  fuse=False is bit-equal to the eager path everywhere.  The
program routes are compared with float32(reference): bit-equal where there is neither a filter nor an LFO nor the bus in the
graph (where the default route keeps a graph one kernel per node -- an envelope is outside the interpreter's small register file --
it stores float32 between the nodes like the eager path and is held to the tolerance instead), within the neighbouring tests' 1e-6 max(1, |ref|) behind filters, under the bus and under an LFO
(test_gpu_program_engine.py).  The LFO-driven voice reads a continuous table (a band-limited saw of 16 harmonics), so a last-bit
difference in `hertz` cannot cross a jump: no sample is masked anywhere in this file.  The references are rendered once per
(graph, position, block size) and shared by the four routes."""
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import ROUTES_WITH_DEFAULT as ROUTES, dev, gpu_ready, render_batches, tolerance
from helpers import HOUR, RATE, f32, fix, maxerr, mkosc, render, stream
import wavetable_reference as WR

pytestmark = pytest.mark.gpu

V, KS = 200, (3, 3)


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


def tables(T, W, seed=0):
    """a random table and a discontinuous one (naive saws of alternating sign: a jump of 2 across the wrap)"""
    rng = np.random.default_rng(seed)
    ramp = (2.0 * np.arange(T) / T - 1.0)[:, None] * np.where(np.arange(W) % 2, -1.0, 1.0)[None, :]
    return {'random': rng.uniform(-1, 1, (T, W)), 'jump': ramp}


def select_rows(rng, blocks, width, W):
    s = rng.uniform(-1.5, W + 1.5, (blocks, width))                           # negatives, values >= W, fractional values ...
    s[:, ::7] = np.nan                                                        # ... and NaN
    s[:, 1::7] = np.floor(s[:, 1::7])
    return s


# ---------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize('pos', [0, 50, HOUR])
@pytest.mark.parametrize('T,W', [(2, 1), (64, 3), (2048, 8)])
def test_osc_bank_table_matches_the_formula_bit_for_bit(T, W, pos):
    from signals_amd import _native
    rng = np.random.default_rng(T + W)
    # (voices, padding of the leading dimension, parameter rows, rows, negative phase); 500 rows in 5 blocks of 100: the parameter
    # row changes inside a wave's 16 rows and the last wave is ragged
    for voices, pad, blocks, rows, negative in ((256, 0, 1, 512, False), (256, 4, 5, 500, False), (97, 3, 1, 512, False),
                                                (97, 0, 5, 500, True), (256, 0, 1, 512, True)):
        hz = rng.uniform(55, 1760, (blocks, voices))
        ph = rng.uniform(-3, -1, (blocks, voices)) if negative else rng.uniform(0, 1, (blocks, voices))      # t < 0 over the first rows
        if negative:
            ph[:, ::5] = -0.25                                                # with hertz 0: t on a table point, below zero
            hz[:, ::5] = 0.0
        sel = select_rows(rng, blocks, voices, W)
        for name, table in tables(T, W).items():
            tab = dev(table, torch.float32)
            for dt, cast in ((torch.float64, lambda a: a), (torch.float32, f32)):
                obuf = torch.zeros((rows, voices + pad), dtype=dt, device='cuda:0')
                _native.osc_bank_table(pos, RATE, dev(hz), dev(ph), dev(sel), tab, obuf[:, :voices],
                                       rows_per_param=rows // blocks if blocks > 1 else 0)
                want = WR.wavetable(table, pos, rows // blocks, hz, ph, sel, blocks=blocks)
                what = (T, W, pos, voices, pad, blocks, negative, name, dt)
                assert not obuf[:, voices:].any(), what                       # the padding is not written
                assert np.array_equal(obuf[:, :voices].cpu().numpy(), cast(want)), what


def test_osc_bank_table_broadcast_rows_and_block_rate():
    """one-column hertz / phase / select rows, an unplugged select and phase, and a block-rate launch (one row per block)"""
    from signals_amd import _native
    rng = np.random.default_rng(5)
    table = tables(64, 3)['random']
    tab = dev(table, torch.float32)
    hz, sel = rng.uniform(55, 1760, (1, 96)), np.array([[1.0]])
    out = torch.empty((300, 96), dtype=torch.float32, device='cuda:0')
    _native.osc_bank_table(HOUR, RATE, dev(hz), None, dev(sel), tab, out)
    assert np.array_equal(out.cpu().numpy(), f32(WR.wavetable(table, HOUR, 300, hz, 0.0, sel)))
    _native.osc_bank_table(HOUR, RATE, dev(hz), None, None, tab, out)
    assert np.array_equal(out.cpu().numpy(), f32(WR.wavetable(table, HOUR, 300, hz, 0.0, 0.0)))
    one = torch.empty((300, 1), dtype=torch.float64, device='cuda:0')
    _native.osc_bank_table(50, RATE, dev([[440.0]]), dev([[0.125]]), dev([[2.0]]), tab, one)
    assert np.array_equal(one.cpu().numpy(), WR.wavetable(table, 50, 300, [[440.0]], [[0.125]], [[2.0]]))
    K, N = 9, 256                                                             # what a control port would see for K blocks
    hzk = rng.uniform(1, 20, (K, 96))
    ctl = torch.empty((K, 96), dtype=torch.float64, device='cuda:0')
    _native.osc_bank_table(HOUR, RATE, dev(hzk), None, dev(sel), tab, ctl, step=N, rows_per_param=1)
    assert np.array_equal(ctl.cpu().numpy(), WR.wavetable(table, HOUR, 1, hzk, 0.0, sel, blocks=K, step=N))


def test_the_table_lives_in_lds_for_many_row_groups():
    """enough rows that a workgroup walks several row groups per wave with per-block rows (the staging is paid once per workgroup)"""
    from signals_amd import _native
    rng = np.random.default_rng(6)
    T, W, voices, N, K = 2048, 8, 97, 100, 700                               # two voice tiles x 547 passes: two row groups per wave
    table = tables(T, W)['random']
    hz, sel = rng.uniform(55, 1760, (K, voices)), select_rows(rng, K, voices, W)
    out = torch.empty((N * K, voices), dtype=torch.float32, device='cuda:0')
    _native.osc_bank_table(0, RATE, dev(hz), None, dev(sel), dev(table, torch.float32), out, rows_per_param=N)
    assert np.array_equal(out.cpu().numpy(), f32(WR.wavetable(table, 0, N, hz, 0.0, sel, blocks=K)))


def test_the_widest_table_fills_the_most_lds():
    """T = 2, W = 8192: the cap on the points admits it, and with the guard entries it is the largest staging there is,
    (T + 1) W 4 = 98304 bytes of LDS for the per-node kernel -- and the same on top of the bus tiles in a voice program"""
    from signals_amd import _native
    from signals_amd.chain import ext, fx
    rng = np.random.default_rng(7)
    T, W, voices, rows = 2, 8192, 256, 300
    table = rng.uniform(-1, 1, (T, W))
    hz, ph, sel = rng.uniform(55, 1760, (1, voices)), rng.uniform(0, 1, (1, voices)), rng.uniform(-2, W + 2, (1, voices))
    sel[0, :4] = (0.0, W - 1, W, 4095.5)
    out = torch.empty((rows, voices), dtype=torch.float32, device='cuda:0')
    _native.osc_bank_table(HOUR, RATE, dev(hz), dev(ph), dev(sel), dev(table, torch.float32), out)
    want = WR.wavetable(table, HOUR, rows, hz, ph, sel)
    assert np.array_equal(out.cpu().numpy(), f32(want))
    N, ks = 128, (2, 1)                                                       # the same voices as a program: stored, and under a mono bus
    stored, names, _ = render_batches(node(table, hz, ph, sel), voices, HOUR, N, ks, names=True, fuse_program='always')
    gain = rng.uniform(0.2, 1.0, (1, voices))
    g = fx.Gain(); g.left = node(table, hz, ph, sel); g.right = fix(gain)
    bus = ext.SumBus(); bus.input = g
    summed, bus_names, _ = render_batches(bus, 1, HOUR, N, ks, names=True, fuse_program='always')
    assert any(n.startswith('voice_program_bus[OscTable') for n in bus_names), bus_names
    block = WR.wavetable(table, HOUR, N * sum(ks), hz, ph, sel)
    if any(n.startswith('voice_program') for n in names):                     # (a single node may stay its own kernel)
        assert np.array_equal(stored, f32(block))
    ref = np.sum(block * gain, axis=1, keepdims=True)
    assert maxerr(summed, f32(ref)) <= tolerance(ref)


# ---------------------------------------------------------------------------------------------- the eager node
def node(table, hertz, phase=None, select=None):
    from signals_amd.chain import ext
    w = ext.Wavetable()
    w.get_state().table = table
    w.hertz = hertz if not isinstance(hertz, np.ndarray) else fix(hertz)
    if phase is not None:
        w.phase = fix(phase)
    if select is not None:
        w.select = fix(select)
    return w


@pytest.mark.parametrize('pos', [0, 50, HOUR])
def test_eager_node_against_the_reference(pos):
    rng = np.random.default_rng(8)
    hz, ph = rng.uniform(55, 1760, (1, V)), rng.uniform(0, 1, (1, V))
    for (T, W), which in (((64, 3), 'random'), ((2048, 8), 'jump'), ((2, 1), 'random')):
        table = tables(T, W)[which]
        sel = select_rows(rng, 1, V, W)
        for frames in (256, 1):                                               # a block (float32) and a one-frame request (float64)
            got = render(node(table, hz, ph, sel), pos, frames, V)
            want = WR.wavetable(table, pos, frames, hz, ph, sel)
            assert got.shape == (frames, V) and got.dtype == (np.float32 if frames > 1 else np.float64)
            assert np.array_equal(got, f32(want) if frames > 1 else want), (T, W, which, pos, frames)
            plain = render(node(table, hz, ph), pos, frames, V)               # unplugged select: column 0
            assert np.array_equal(plain, render(node(table, hz, ph, np.zeros((1, 1))), pos, frames, V))
            assert np.array_equal(plain, f32(WR.wavetable(table, pos, frames, hz, ph, 0.0)) if frames > 1
                                  else WR.wavetable(table, pos, frames, hz, ph, 0.0))


def test_an_integer_table_and_an_in_place_edit():
    table = np.array([[0, 0], [2, 1], [0, 0], [-2, -1]])                      # int64, what a .sigs value arrives as
    hz = np.full((1, 8), 1000.0)
    w = node(table, hz, select=np.array([[0.0, 1.0] * 4]))
    assert np.array_equal(render(w, 0, 128, 8), f32(WR.wavetable(table, 0, 128, hz, 0.0, [[0.0, 1.0] * 4])))
    table[1, 0] = 5                                                           # seen at the next reply (HostSnapshot)
    assert np.array_equal(render(w, 128, 128, 8), f32(WR.wavetable(table, 128, 128, hz, 0.0, [[0.0, 1.0] * 4])))


def test_a_sine_table_is_the_sine_oscillator_within_the_lerp_bound():
    """checks the orientation of the table: (T, 1) filled from sin(2 pi k / T) along the first axis, T = 16384, stays within the
    interpolation bound pi^2 / (2 T^2) (= h^2 / 8 max|f''|, h = 1 / T) + 1e-7 (the float32 table entries) of osc.Sine.  Compared
    where osc.Sine is itself accurate enough for that bound to mean something: one-frame requests, which both nodes answer in
    float64 (osc.Sine within 1e-15).  On float32 blocks osc.Sine's own contract is 1.3e-7 (the hardware sine) and both sides round
    their store to float32, so two correct outputs near +-1 can sit one float32 step apart: measured 1.19e-7 = 2^-23 against the
    bound's 1.18e-7.  The float32 block is therefore held to the same bound against numpy's float64 sine of the same phase
    (table entries 2^-25 + interpolation 1.8e-8 + the store's 2^-25 = 7.8e-8)."""
    from oracle import chain_ref as R
    T = 16384
    table = np.sin(2.0 * np.pi * np.arange(T) / T)[:, None]
    rng = np.random.default_rng(9)
    hz, ph = rng.uniform(55, 1760, (1, V)), rng.uniform(0, 1, (1, V))
    bound = np.pi ** 2 / (2.0 * T ** 2) + 1e-7
    w, s = node(table, hz, ph), mkosc('Sine', hz, ph)
    for start in (0, HOUR):
        worst = 0.0
        for pos in range(start, start + 48 * 37, 37):
            got, ref = render(w, pos, 1, V), render(s, pos, 1, V)
            assert got.dtype == ref.dtype == np.float64
            worst = max(worst, maxerr(got, ref))
        err32 = maxerr(render(w, start, 256, V), np.sin(R.osc_cycles(start, 256, RATE, hz, ph) * 2 * np.pi))
        print('sine table against osc.Sine, float64 requests from', start, worst, '; float32 block against numpy', err32, 'bound', bound)
        assert worst <= bound and err32 <= bound, (start, worst, err32)


# ---------------------------------------------------------------------------------------------- graphs
def draw(seed=3):
    rng = np.random.default_rng(seed)
    th = rng.uniform(0, np.pi / 2, V)
    return dict(hertz=rng.uniform(55, 1760, (1, V)), phase=rng.uniform(0, 1, (1, V)), select=rng.uniform(-1, 5, (1, V)),
                cut1=rng.uniform(200, 8000, (1, V)), cut2=rng.uniform(200, 8000, (1, V)),
                gain=rng.uniform(0.2, 1.0, (1, V)), pan=np.stack([np.cos(th), np.sin(th)]),
                env=dict(attack=rng.uniform(0.002, 0.02, (1, V)), decay=rng.uniform(0.01, 0.05, (1, V)), sustain=rng.uniform(0.3, 0.9, (1, V)),
                         release=rng.uniform(0.01, 0.05, (1, V)), gate_on=rng.uniform(0.0, 0.01, (1, V)), gate_off=rng.uniform(0.04, 0.07, (1, V))))


TABLE = np.concatenate([tables(512, 3)['random'], tables(512, 1)['jump']], axis=1)     # (512, 4): three random columns and a naive saw
SAW16 = WR.band_limited_saw(2048, 16)


def graph(which, p):
    """(GPU node, oracle node, rendered width, exact on the program routes) of one voice shape"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    RW = WR.oracle_node()
    w = node(TABLE, p['hertz'], p['phase'], p['select'])
    rw = RW(TABLE, R.Fixed(p['hertz']), R.Fixed(p['phase']), R.Fixed(p['select']))
    if which in ('bus', 'lowpass_bus'):                                       # SumBus(Gain(Wavetable)), SumBus(Gain(LowPass(Wavetable))), stereo
        src, rsrc = w, rw
        if which == 'lowpass_bus':
            src = fx.LowPass(); src.input = w; src.cutoff = fix(p['cut1'])
            rsrc = R.Filter('lp', rw, R.Fixed(p['cut1']))
        g = fx.Gain(); g.left = src; g.right = fix(p['gain'])
        b = ext.SumBus(); b.input = g; b.get_state().gains = np.ascontiguousarray(p['pan'])
        return b, R.SumBus(R.Binary('Gain', rsrc, R.Fixed(p['gain'])), p['pan']), 2, False
    if which == 'adsr':                                                       # Wavetable x ADSR
        env = ext.ADSR()
        for name, row in p['env'].items():
            setattr(env, name, fix(row))
        x = fx.RingMod(); x.left = w; x.right = env
        return x, R.Binary('RingMod', rw, R.Adsr(**p['env'])), V, True
    if which == 'cascade':                                                    # LowPass(LowPass(Wavetable))
        f1 = fx.LowPass(); f1.input = w; f1.cutoff = fix(p['cut1'])
        f2 = fx.LowPass(); f2.input = f1; f2.cutoff = fix(p['cut2'])
        return f2, R.Filter('lp', R.Filter('lp', rw, R.Fixed(p['cut1'])), R.Fixed(p['cut2'])), V, False
    if which == 'lfo':                                                        # hertz = centre + depth sin(2 pi 3.1 t), through the control program
        s = mkosc('Sine', [[3.1]])
        g = fx.Gain(); g.left = s; g.right = fix(0.04 * p['hertz'])
        m = fx.Mix(); m.left = g; m.right = fix(2.0 * p['hertz']); m.mix = fix([[0.5]])
        rm = R.Binary('Mix', R.Binary('Gain', R.Osc('Sine', R.Fixed([[3.1]])), R.Fixed(0.04 * p['hertz'])), R.Fixed(2.0 * p['hertz']),
                      R.Fixed([[0.5]]))
        g2 = fx.Gain(); g2.left = node(SAW16, m, p['phase']); g2.right = fix(p['gain'])        # (two nodes: a program of its own)
        return g2, R.Binary('Gain', RW(SAW16, rm, R.Fixed(p['phase'])), R.Fixed(p['gain'])), V, False
    if which == 'mix':                                                        # Mix of two Wavetables on different columns of ONE table
        a, b = node(TABLE, p['hertz'], p['phase'], [[1.0]]), node(TABLE, p['hertz'], p['phase'], [[3.0]])
        mix = np.linspace(0.0, 1.0, V)[None, :]
        m = fx.Mix(); m.left = a; m.right = b; m.mix = fix(mix)
        ra, rb = (RW(TABLE, R.Fixed(p['hertz']), R.Fixed(p['phase']), R.Fixed([[c]])) for c in (1.0, 3.0))
        return m, R.Binary('Mix', ra, rb, R.Fixed(mix)), V, True
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


CASES = [(which, N) for which in ('bus', 'lowpass_bus', 'adsr', 'lfo', 'mix') for N in (64, 256)] + [('cascade', 256)]


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
    tol = tolerance(want)
    err = maxerr(eager, f32(want))
    print('wavetable eager', what, 'max|err|', err, 'tol', tol)
    assert err <= tol, (what, err)                                            # (float32 between its nodes: never bit-equal to the oracle)
    if route == 'per_node':
        assert not program and np.array_equal(got, eager), what               # as the docstring of fuse=False promises
        return
    assert program or route == 'default', (what, names)                       # forced routes run the program; the default follows worthwhile()
    err = maxerr(got, f32(want))
    print('wavetable route', what, 'max|err|', err, 'tol', tol, 'exact' if exact and program else '', 'program' if program else 'per node')
    if exact and program:                                                     # (one kernel per node stores float32 between the nodes)
        assert np.array_equal(got, f32(want)), (what, err)
    else:
        assert err <= tol, (what, err, tol)


def test_launches_of_each_route():
    p = draw()
    for route, kw in ROUTES.items():
        _, names, r = render_batches(graph('bus', p)[0], 2, 0, 256, (4,), names=True, **kw)
        if route == 'per_node':
            assert any(n.startswith('osc_bank_table[Table]') for n in names) and not any(n.startswith('voice_program') for n in names), names
        else:
            assert any(n.startswith('voice_program_bus[OscTable') for n in names), (route, names)
            assert not any(n.startswith(('osc_bank', 'sum_bus')) for n in names), (route, names)
            assert any('*specialised' in n for n in names) == bool(r.specialise), (route, names)
    names = render_batches(graph('lfo', p)[0], V, 0, 256, (4,), names=True, fuse=False).names      # a swept hertz: per-block rows on the per-node schedule
    assert any(n.startswith('osc_bank_table[Table,per-block]') for n in names), names


@pytest.mark.parametrize('pos', [0, HOUR])
def test_a_band_filter_behind_a_wavetable_renders_per_node(pos):
    """no interpreter variant has both instructions: the engine keeps the graph one kernel per node, on every route"""
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    p = draw()
    RW = WR.oracle_node()
    low, high = p['cut1'] * 0.5, p['cut1'] * 0.5 + 900.0

    def build():
        bp = fx.BandPass(); bp.input = node(TABLE, p['hertz'], p['phase'], p['select']); bp.low = fix(low); bp.high = fix(high)
        return bp
    ref = R.BandFilter('bp', RW(TABLE, R.Fixed(p['hertz']), R.Fixed(p['phase']), R.Fixed(p['select'])), R.Fixed(low), R.Fixed(high))
    want = R.render_stream(ref, pos, 256, sum(KS), V)
    tol = tolerance(want)
    for route in ('default', 'always'):
        got, names, _ = render_batches(build(), V, pos, 256, (3, 3), names=True, **ROUTES[route])
        assert any(n.startswith('osc_bank_table') for n in names) and not any(n.startswith('voice_program') for n in names), names
        assert maxerr(got, f32(want)) <= tol, (route, pos, maxerr(got, f32(want)), tol)


def test_a_wavetable_in_a_control_path_keeps_the_eager_path():
    from signals_amd.chain import fx
    from signals_amd.engine import BatchRenderer, NotBatchable
    p = draw()
    lfo = node(SAW16, np.array([[3.0]]))
    g = fx.Gain(); g.left = mkosc('Sawtooth', p['hertz'], p['phase']); g.right = lfo
    with pytest.raises(NotBatchable, match='wavetable oscillator'):
        BatchRenderer(g, V, RATE).render(0, 256, 2)
    got = stream(g, 0, 256, 2, V)                                             # the eager node serves the one-frame reads in float64
    from oracle import chain_ref as R
    ctl = np.concatenate([WR.wavetable(SAW16, b * 256, 1, [[3.0]]) for b in range(2)])
    want = np.concatenate([f32(R.osc('Sawtooth', b * 256, 256, RATE, p['hertz'], p['phase'])).astype(np.float64) * ctl[b] for b in range(2)])
    assert np.array_equal(got, f32(want))
