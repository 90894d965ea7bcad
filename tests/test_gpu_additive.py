"""The additive oscillator on the GPU: sig_osc_bank_additive against the numpy restatement (tests/additive_reference.py) over the
shared case table, the eager node against the batched engine bit for bit, the engine's routes against an oracle built from the
restatement and oracle/chain_ref.py, one-frame requests, and the node on a filter's cutoff.

Tolerance.  Because of the sine the kernel is held to a bound, not to bits: every sample within 1e-6 * max(1, A) of the restatement,
A the largest column sum of |a| -- the project's bar against the oracle (gpu_helpers.tolerance) scaled by the gain bound.  NaN
placement is compared exactly, and the lanes without a partial (k = 0) to exactly 0.0.  The largest error seen is printed per test.
The restatement's rows are rendered once per case and shared."""
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import ROUTES_FORCED, dev, gpu_ready, render_batches, tolerance
from helpers import HOUR, RATE, f32, fix, maxerr, mkosc, render, stream
import additive_reference as AR

pytestmark = pytest.mark.gpu

CASES = AR.cases()
V = 70


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


@functools.lru_cache(maxsize=None)
def wanted(index):
    want = AR.render_case(CASES[index])
    want.setflags(write=False)
    return want


def launch(c, dtype, pad=0):
    from signals_amd import _native
    rows, voices = c['N'] * c['K'], c['voices']
    buf = torch.full((rows, voices + pad), 7.0, dtype=dtype, device='cuda:0')
    _native.osc_bank_additive(c['position'], RATE, dev(c['hertz']), dev(c['phase']), dev(c['select']), dev(c['table'], torch.float32),
                              buf[:, :voices], rows_per_param=c['N'] if c['K'] > 1 else 0)
    got = buf.cpu().numpy()
    assert (got[:, voices:] == 7.0).all(), (c['name'], 'the padding is not written')
    return got[:, :voices]


def check(c, got, want, what):
    """NaN placement exactly, k = 0 voices exactly 0.0, everything else within the bound; returns the largest error"""
    k = AR.band_limit(np.broadcast_to(c['hertz'], (c['hertz'].shape[0], c['voices'])), c['H'])[1]
    silent = np.repeat(k == 0.0, c['N'], axis=0) if k.shape[0] > 1 else np.broadcast_to(k == 0.0, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, 'NaN placement')
    assert (got[silent] == 0.0).all() and (want[silent] == 0.0).all(), (what, 'k = 0 is exactly 0.0')
    err, tol = maxerr(got, want), AR.tolerance(c['table'])
    print('additive kernel', what, 'max|err|', err, 'tol', tol)
    assert err <= tol, (what, err, tol)
    return err


# ---------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize('index', range(len(CASES)), ids=[c['name'] for c in CASES])
def test_kernel_against_the_restatement(index):
    c, want = CASES[index], wanted(index)
    worst32 = check(c, launch(c, torch.float32, pad=0 if index % 2 else 4), want, (c['name'], 'float32'))
    worst64 = check(c, launch(c, torch.float64), want, (c['name'], 'float64'))
    print('additive worst', c['name'], 'float32', worst32, 'float64', worst64, 'A', AR.gain_bound(c['table']))


def test_broadcast_rows_unplugged_ports_and_a_block_rate_launch():
    """one-column hertz / phase / select rows, an unplugged select and phase, a (rows, 1) launch, and one row per block (step = N)"""
    from signals_amd import _native
    rng = np.random.default_rng(5)
    table = AR.spectra(24, 3)
    tab, tol = dev(table, torch.float32), AR.tolerance(table)
    hz, sel = rng.uniform(55, 1760, (1, 96)), np.array([[1.0]])
    out = torch.empty((300, 96), dtype=torch.float32, device='cuda:0')
    _native.osc_bank_additive(HOUR, RATE, dev(hz), None, dev(sel), tab, out)
    assert maxerr(out.cpu().numpy(), AR.additive(table, HOUR, 300, hz, 0.0, sel)) <= tol
    _native.osc_bank_additive(HOUR, RATE, dev(hz), None, None, tab, out)
    assert maxerr(out.cpu().numpy(), AR.additive(table, HOUR, 300, hz, 0.0, 0.0)) <= tol
    one = torch.empty((300, 1), dtype=torch.float64, device='cuda:0')
    _native.osc_bank_additive(50, RATE, dev([[440.0]]), dev([[0.125]]), dev([[2.0]]), tab, one)
    assert maxerr(one.cpu().numpy(), AR.additive(table, 50, 300, [[440.0]], [[0.125]], [[2.0]])) <= tol
    K, N = 9, 256                                                             # what a control port would see for K blocks
    hzk = rng.uniform(1, 20, (K, 96))
    ctl = torch.empty((K, 96), dtype=torch.float64, device='cuda:0')
    _native.osc_bank_additive(HOUR, RATE, dev(hzk), None, dev(sel), tab, ctl, step=N, rows_per_param=1)
    assert maxerr(ctl.cpu().numpy(), AR.additive(table, HOUR, 1, hzk, 0.0, sel, blocks=K, step=N)) <= tol


def test_the_largest_tables_and_many_row_groups():
    """H * W at the cap both ways (64 x 256: the even column stride; 1 x 16384), and enough rows that a wave walks several row groups
    with per-block rows"""
    from signals_amd import _native
    rng = np.random.default_rng(6)
    for H, W, voices, N, K in ((64, 256, 64, 64, 2), (1, 16384, 65, 64, 2), (5, 2, 97, 100, 300)):
        table = AR.spectra(H, W)
        hz = rng.uniform(200, 900, (K, voices))
        sel = rng.uniform(-2, W + 2, (K, voices))
        sel[:, :3] = (0.0, W - 1, W)
        out = torch.empty((N * K, voices), dtype=torch.float32, device='cuda:0')
        _native.osc_bank_additive(0, RATE, dev(hz), None, dev(sel), dev(table, torch.float32), out, rows_per_param=N)
        err = maxerr(out.cpu().numpy(), AR.additive(table, 0, N, hz, 0.0, sel, blocks=K))
        print('additive table', (H, W, voices, N, K), 'max|err|', err)
        assert err <= AR.tolerance(table), (H, W, err)


# ---------------------------------------------------------------------------------------------- the node, eager and batched
HARMONICS = np.arange(1, 41)[:, None]
TABLE = np.hstack([AR.spectra(40, 2), 2.0 / (np.pi * HARMONICS) * np.where(HARMONICS % 2, 1.0, -1.0)])     # two random spectra and a saw


def draw(seed=3):
    rng = np.random.default_rng(seed)
    th = rng.uniform(0, np.pi / 2, V)
    hertz = rng.uniform(55, 1760, (1, V))
    hertz[0, :6] = (0.0, -440.0, 0.01, 700.0, 23000.0, 30000.0)               # every partial; mirrored; sub-audio; 34; one; none
    return dict(hertz=hertz, phase=rng.uniform(0, 1, (1, V)), select=rng.uniform(-1, 4, (1, V)),
                cut=rng.uniform(200, 8000, (1, V)), pan=np.stack([np.cos(th), np.sin(th)]),
                env=dict(attack=rng.uniform(0.002, 0.02, (1, V)), decay=rng.uniform(0.01, 0.05, (1, V)), sustain=rng.uniform(0.3, 0.9, (1, V)),
                         release=rng.uniform(0.01, 0.05, (1, V)), gate_on=rng.uniform(0.0, 0.01, (1, V)), gate_off=rng.uniform(0.04, 0.07, (1, V))))


def node(table, hertz, phase=None, select=None):
    from signals_amd.chain import ext
    a = ext.Additive()
    a.get_state().table = table
    a.hertz = hertz if not isinstance(hertz, np.ndarray) else fix(hertz)
    if phase is not None:
        a.phase = fix(phase)
    if select is not None:
        a.select = fix(select)
    return a


def graph(which, p):
    """(GPU node, oracle node, rendered width) of one voice shape"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    RA = AR.oracle_node()
    a = node(TABLE, p['hertz'], p['phase'], p['select'])
    ra = RA(TABLE, R.Fixed(p['hertz']), R.Fixed(p['phase']), R.Fixed(p['select']))
    if which == 'alone':
        return a, ra, V
    if which == 'lowpass_bus':                                                # SumBus(LowPass(Additive)), stereo
        lp = fx.LowPass(); lp.input = a; lp.cutoff = fix(p['cut'])
        b = ext.SumBus(); b.input = lp; b.get_state().gains = np.ascontiguousarray(p['pan'])
        return b, R.SumBus(R.Filter('lp', ra, R.Fixed(p['cut'])), p['pan']), 2
    if which == 'adsr_bus':                                                   # SumBus(RingMod(Additive, ADSR)), mono
        env = ext.ADSR()
        for name, r in p['env'].items():
            setattr(env, name, fix(r))
        x = fx.RingMod(); x.left = a; x.right = env
        b = ext.SumBus(); b.input = x
        rb = R.SumBus(R.Binary('RingMod', ra, R.Adsr(**p['env'])))
        rb.in_channels = V
        return b, rb, 1
    if which == 'sweep':                                                      # a pitch envelope: hertz through the control program
        s = mkosc('Sine', [[3.1]])
        g = fx.Gain(); g.left = s; g.right = fix(0.5 * p['hertz'])
        m = fx.Mix(); m.left = g; m.right = fix(2.0 * p['hertz']); m.mix = fix([[0.5]])
        rm = R.Binary('Mix', R.Binary('Gain', R.Osc('Sine', R.Fixed([[3.1]])), R.Fixed(0.5 * p['hertz'])), R.Fixed(2.0 * p['hertz']),
                      R.Fixed([[0.5]]))
        return node(TABLE, m, p['phase'], p['select']), RA(TABLE, rm, R.Fixed(p['phase']), R.Fixed(p['select'])), V
    raise KeyError(which)


def bound(want):
    """the kernel's bound carried through the graph: 1e-6 of full scale (gpu_helpers.tolerance) times the gain bound of the table, the
    way tests/random_ext_graphs.py scales by G"""
    return tolerance(want) * max(1.0, AR.gain_bound(TABLE))


@pytest.mark.parametrize('pos,ks', [(0, (1, 2, 3)), (8192, (1, 2, 3))])
@pytest.mark.parametrize('which', ['alone', 'sweep'])
def test_eager_rows_equal_batched_rows_bit_for_bit(which, pos, ks):
    """the same kernel on both paths: a fresh batch at position 0 and at 8192, and batches of 1, 2 and 3 blocks"""
    p = draw()
    N = 128
    eager = stream(graph(which, p)[0], pos, N, sum(ks), V)
    got, names, _ = render_batches(graph(which, p)[0], V, pos, N, ks, names=True)
    label = 'osc_bank_additive[Additive40' + (',per-block]' if which == 'sweep' else ']')
    assert label in names and not any(n.startswith(('voice_program', 'osc_bank_table')) for n in names), names
    assert got.dtype == np.float32 and np.array_equal(got, eager, equal_nan=True), (which, pos)
    if which == 'sweep':
        from oracle import chain_ref as R
        want = R.render_stream(graph(which, p)[1], pos, N, sum(ks), V)
        err = maxerr(got, f32(want))
        print('additive sweep', pos, 'max|err|', err, 'tol', bound(want))
        assert err <= bound(want)


@functools.lru_cache(maxsize=None)
def oracle_rows(which, pos, N, blocks):
    from oracle import chain_ref as R
    _, ref, C = graph(which, draw())
    want = R.render_stream(ref, pos, N, blocks, C)
    want.setflags(write=False)
    return want


ROUTES = dict(default={}, **{k: v for k, v in ROUTES_FORCED.items() if k != 'per_node'}, mixed={'fuse_program': 'always', 'mixed_programs': True})


@pytest.mark.parametrize('pos', [0, HOUR])
@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('which', ['alone', 'lowpass_bus', 'adsr_bus'])
def test_routes(which, route, pos):
    N, ks = 128, (2, 1)
    want = oracle_rows(which, pos, N, sum(ks))
    top, _, C = graph(which, draw())
    got, names, _ = render_batches(top, C, pos, N, ks, names=True, **ROUTES[route])
    what = (which, route, pos)
    banks = sorted(n for n in names if n.startswith('osc_bank'))
    assert banks == ['osc_bank_additive[Additive40]'], (what, names)          # one kernel per batch for the oscillator, under one label
    # no voice program and no fused voice kernel holds the oscillator; the nodes around it keep their routes (the filter-and-bus pass
    # reads the oscillator's stored rows, like the cold-start filter)
    assert not any(word in n for n in names for word in ('voice_program', 'fused', 'cascade', 'walk', 'steady', 'latency')), (what, names)
    err, tol = maxerr(got, f32(want)), bound(want)
    print('additive route', what, 'max|err|', err, 'tol', tol, sorted(names))
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize('pos', [0, 37, HOUR])
def test_one_frame_requests_are_float64_and_within_the_bound(pos):
    p = draw()
    worst = 0.0
    for frames in (1, 256):
        got = render(node(TABLE, p['hertz'], p['phase'], p['select']), pos, frames, V)
        want = AR.additive(TABLE, pos, frames, p['hertz'], p['phase'], p['select'])
        assert got.shape == (frames, V) and got.dtype == (np.float64 if frames == 1 else np.float32)
        worst = max(worst, maxerr(got, want))
    plain = render(node(TABLE, p['hertz'], p['phase']), pos, 1, V)            # unplugged select: column 0
    assert np.array_equal(plain, render(node(TABLE, p['hertz'], p['phase'], np.zeros((1, 1))), pos, 1, V))
    print('additive eager', pos, 'max|err|', worst)
    assert worst <= AR.tolerance(TABLE)


def test_an_integer_table_and_an_in_place_edit():
    table = np.array([[2, 1], [0, 1], [1, 0]])                                # int64, what a .sigs value arrives as
    hz, sel = np.full((1, 8), 1000.0), [[0.0, 1.0] * 4]
    a = node(table, hz, select=np.array(sel))
    assert maxerr(render(a, 0, 128, 8), AR.additive(table, 0, 128, hz, 0.0, sel)) <= AR.tolerance(table)
    table[1, 0] = 5                                                           # seen at the next reply
    assert maxerr(render(a, 128, 128, 8), AR.additive(table, 128, 128, hz, 0.0, sel)) <= AR.tolerance(table)


def test_a_cutoff_modulated_by_the_node_renders_eagerly_and_equals_the_oracle():
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    from signals_amd.engine import BatchRenderer, NotBatchable
    p = draw()
    organ = np.array([[1.0], [0.5], [0.0], [0.25]])
    RA = AR.oracle_node()

    cut = p['cut'][:, 6:]

    def build():
        lfo = node(organ, np.array([[2.0]]))                                  # a 2 Hz four-partial LFO ...
        g = fx.Gain(); g.left = lfo; g.right = fix(0.3 * cut)
        m = fx.Mix(); m.left = g; m.right = fix(2.0 * cut); m.mix = fix([[0.5]])            # ... around the cutoff
        lp = fx.LowPass(); lp.input = mkosc('Sawtooth', p['hertz'][:, 6:], p['phase'][:, 6:]); lp.cutoff = m
        return lp
    rm = R.Binary('Mix', R.Binary('Gain', RA(organ, R.Fixed([[2.0]])), R.Fixed(0.3 * cut)), R.Fixed(2.0 * cut), R.Fixed([[0.5]]))
    ref = R.Filter('lp', R.Osc('Sawtooth', R.Fixed(p['hertz'][:, 6:]), R.Fixed(p['phase'][:, 6:])), rm)
    with pytest.raises(NotBatchable, match='a wavetable oscillator has no block-rate'):
        BatchRenderer(build(), V - 6, RATE).render(0, 256, 2)
    got = stream(build(), 0, 256, 3, V - 6)                                   # the eager node serves the one-frame reads in float64
    want = R.render_stream(ref, 0, 256, 3, V - 6)
    err = maxerr(got, f32(want))
    print('additive on a cutoff', 'max|err|', err, 'tol', tolerance(want))
    assert err <= tolerance(want)
