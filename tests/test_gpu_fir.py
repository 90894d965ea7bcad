"""The dense FIR filter on the GPU: sig_fir_taps against tests/fir_reference.py bit for bit, the eager node (BlockDriver, eager pulls)
against the batched engine (BatchRenderer) bit for bit, and both against a float64 chain of oracle.chain_ref plus fir_reference.

Bars.  The formula is products and sums in a fixed order and the library is built with contraction off, so the kernel's float64 output
equals the reference bit for bit (NaN where the reference has NaN) and its float32 output equals float32(reference) bit for bit: no
tolerance.  The batched engine launches the same kernels on the same stored float32 rows as the eager path, so the two are bit-equal
on every graph here wherever no fused kernel takes a node BEHIND the FIR (the test asserts which).  Against the float64 restatement
chain every route is held to the project's bar scaled by the filter's gain bound: 1e-6 * G * max(1, max|ref|), G = max_w sum_k |h[k, w]|
of the graph's widest FIR and 1 where that is below 1 -- a FIR carries its input's error (one float32 rounding per stored node, 2^-24
relative) times at most G and adds one float32 rounding of its own output.  Each graph case first checks, from the reference alone,
that 2^-24 * max|ref| is under a quarter of its bar.  The designs used have G <= 4 (asserted here and, for the shipped Blackman and
Hilbert designs, in tests/test_fir_host.py).

Shapes.  V crosses a wave and a 64-voice tile (1, 3, 64, 70, 130); N in {16, 101, 128}, K in {1, 3}; positions 0, 37 (zero fill and
c0 < 100), 4096 and one hour; L in {1, 2, 17, 100, 101}; W in {1, 3} with the voices of one wave on different columns, one select row
and one per block with the column changing at the block boundary.  3 x 101 = 303 rows cross the kernel's 256-row staging tile inside a
block, and neither 101 nor 303 is a multiple of the 8-row run a lane computes at once; one 300-row block does the same in one block.
The references are computed once per (V, N, K, position, L, W, select form) and shared by the dtype combinations."""
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import dev, gpu_ready, render_batches
from helpers import HOUR, RATE, f32, fix, maxerr, mkosc
import delay_reference as DR
import fir_reference as FR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    gpu_ready()


def same(got, want):
    """bit for bit: the same NaN positions, the same bit patterns elsewhere"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    bits = np.uint64 if got.dtype == np.float64 else np.uint32
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(bits), want[~nan].view(bits)))


# every voice takes the next select value, so the lanes of one wave sit on different columns; block b starts 5 further on
SELECTS = [0.0, 1.0, 2.0, -0.0, 0.99, 2.5, 7.0, -3.0, np.inf, -np.inf, np.nan, 1.5]


def selects(blocks, V):
    return np.array([SELECTS[(v + 5 * b) % len(SELECTS)] for b in range(blocks) for v in range(V)]).reshape(blocks, V)


def table(L, W):
    rng = np.random.default_rng(100 * L + W)
    h = rng.uniform(-1, 1, (L, W))
    if L >= 17:
        h[3, 0] = 0.0                                                          # zero taps are multiplied and added like the rest
        h[L - 1, W - 1] = -0.0
    return h


@functools.lru_cache(maxsize=None)
def kernel_case(V, N, K, pos, L, W, per_block):
    """(window float32-representable float64, select rows, taps, float64 reference): computed once, read-only"""
    rng = np.random.default_rng(V * 1000 + N * 10 + K + pos % 1000 + L)
    c0 = min(100, pos)
    x = rng.uniform(-1.5, 1.5, (c0 + N * K, V)).astype(np.float32).astype(np.float64)
    x[rng.integers(0, x.shape[0], 3), rng.integers(0, V, 3)] = 0.0
    s = selects(K if per_block else 1, V)
    h = table(L, W)
    want = FR.fir(x, c0, N, s, h, blocks=K)
    for a in (x, s, h, want):
        a.setflags(write=False)
    return x, s, h, want


FORMS = ((1, False), (3, False), (3, True))                                    # (W, one select row per block)


@pytest.mark.parametrize('pos', [0, 37, 4096, HOUR])
@pytest.mark.parametrize('V', [1, 3, 64, 70, 130])
def test_fir_taps_matches_the_reference_bit_for_bit(V, pos):
    """every N, K, L, W, select form and dtype combination at one (V, position); outputs are padded and the padding must stay untouched"""
    from signals_amd import _native
    c0 = min(100, pos)
    for N in (16, 101, 128):
        for K in (1, 3):
            for L in (1, 2, 17, 100, 101):
                for W, per_block in FORMS:
                    x, s, h, want = kernel_case(V, N, K, pos, L, W, per_block)
                    assert not np.isnan(want).any()
                    tab = dev(h)
                    for t_in in (torch.float32, torch.float64):
                        for t_out, cast in ((torch.float64, lambda a: a), (torch.float32, f32)):
                            obuf = torch.zeros((N * K, V + 3), dtype=t_out, device='cuda:0')
                            _native.fir_taps(RATE, pos, N, K, dev(x, t_in), c0, dev(s), tab, obuf[:, :V])
                            assert not obuf[:, V:].any(), (V, pos, N, K, L, W)
                            assert same(obuf[:, :V].cpu().numpy(), cast(want)), (V, pos, N, K, L, W, per_block, t_in, t_out)


@pytest.mark.parametrize('N,K', [(300, 1), (101, 3), (517, 2), (256, 2), (257, 1)])
def test_rows_that_cross_the_staging_tile_inside_a_block(N, K):
    """the 256-row tile ends inside a block, at a row that is no multiple of the 8-row run; a padded input beside the padded output.
    (256, 2): a block ends exactly on the tile, a tile per block; (257, 1): one row past it, a second tile of one row"""
    from signals_amd import _native
    V, pos, L, W = 70, 4096, 101, 3
    x, s, h, want = kernel_case(V, N, K, pos, L, W, True)
    xbuf = torch.zeros((100 + N * K, V + 5), dtype=torch.float32, device='cuda:0')
    xbuf[:, :V] = dev(x, torch.float32)
    obuf = torch.zeros((N * K, V + 3), dtype=torch.float64, device='cuda:0')
    _native.fir_taps(RATE, pos, N, K, xbuf[:, :V], 100, dev(s), dev(h), obuf[:, :V])
    assert not obuf[:, V:].any() and same(obuf[:, :V].cpu().numpy(), want)


def test_nonfinite_input_propagates_as_in_numpy():
    """NaN and +-inf in the input: no tap is skipped, so inf * 0 is NaN for the zero taps too, exactly where numpy has it"""
    from signals_amd import _native
    rng = np.random.default_rng(3)
    V, N, K, pos = 70, 128, 3, 37
    x = rng.uniform(-1.5, 1.5, (pos + N * K, V)).astype(np.float32).astype(np.float64)
    x[60, 5], x[200, 5], x[10, 66], x[300, 40] = np.inf, -np.inf, np.nan, np.inf
    h = table(17, 3)
    s = selects(K, V)
    want = FR.fir(x, pos, N, s, h, blocks=K)
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
    for t_in in (torch.float32, torch.float64):
        out = torch.empty((N * K, V), dtype=torch.float64, device='cuda:0')
        _native.fir_taps(RATE, pos, N, K, dev(x, t_in), pos, dev(s), dev(h), out)
        assert same(out.cpu().numpy(), want), t_in


def test_identity_unit_taps_broadcast_input_and_unplugged_select():
    from signals_amd import _native
    rng = np.random.default_rng(21)
    V, N, K = 70, 128, 3
    x = rng.uniform(-1.5, 1.5, (100 + N * K, V)).astype(np.float32)
    out = torch.empty((N * K, V), dtype=torch.float32, device='cuda:0')
    _native.fir_taps(RATE, 4096, N, K, dev(x, torch.float32), 100, None, dev([[1.0]]), out)          # the default table: the identity
    assert same(out.cpu().numpy(), x[100:])
    delayed = torch.empty_like(out)
    for d in (1, 50, 99):
        unit = np.zeros((d + 1, 1)); unit[d] = 1.0
        _native.fir_taps(100, 4096, N, K, dev(x, torch.float32), 100, dev([[0.0]]), dev(unit), out)
        assert same(out.cpu().numpy(), x[100 - d:100 - d + N * K]), d
        _native.delay_taps(100, 4096, N, K, dev(x, torch.float32), 100, dev([[d / 100.0]]), np.array([[1.0, 1.0]]), delayed)   # t * rate = d exactly
        assert same(out.cpu().numpy(), delayed.cpu().numpy()), d
    unit = np.zeros((76, 1)); unit[75] = 1.0
    _native.fir_taps(RATE, 50, N, K, dev(x[50:], torch.float32), 50, None, dev(unit), out)          # position 50, 75 frames back: zeros first
    assert same(out.cpu().numpy(), np.concatenate([np.zeros((25, V), np.float32), x[50:50 + N * K - 25]]))
    # a one-column input broadcast over the voices, per-voice columns
    h, s = table(100, 3), selects(1, V)
    for t_in in (torch.float32, torch.float64):
        _native.fir_taps(RATE, 4096, N, K, dev(x[:, :1], t_in), 100, dev(s), dev(h), out)
        assert same(out.cpu().numpy(), f32(FR.fir(x[:, :1].astype(np.float64), 100, N, s, h, blocks=K)))


def test_wrapper_refusals():
    from signals_amd import _native
    x = torch.zeros((100 + 256, 8), dtype=torch.float32, device='cuda:0')
    out = torch.zeros((256, 8), dtype=torch.float32, device='cuda:0')
    one = dev([[1.0]])
    with pytest.raises(_native.NativeError, match='fir shapes'):
        _native.fir_taps(RATE, 4096, 256, 1, x[:300], 100, None, one, out)
    with pytest.raises(_native.NativeError, match='hipError_t 1'):
        _native.fir_taps(RATE, 37, 256, 1, x, 100, None, one, out)                                   # c0 inconsistent with the position
    with pytest.raises(_native.NativeError, match='FIR table'):
        _native.fir_taps(RATE, 4096, 256, 1, x, 100, None, dev(np.zeros((102, 1))), out)
    with pytest.raises(_native.NativeError, match='FIR table'):
        _native.fir_taps(RATE, 4096, 256, 1, x, 100, None, dev(np.zeros((17, 241))), out)            # 4097 points
    with pytest.raises(_native.NativeError, match='FIR table'):
        _native.fir_taps(RATE, 4096, 256, 1, x, 100, None, dev([[1.0]], torch.float32), out)
    assert not out.any()


# ---------------------------------------------------------------------------------------------- graphs: eager against batched against the oracle
GV, GK = 70, 3
SHIFT_HZ = 5.0


def fir_node(input_, taps, select=None):
    from signals_amd.chain import ext
    n = ext.FIR()
    n.get_state().taps = np.asarray(taps, dtype=np.float64)
    n.input = input_
    if select is not None:
        n.select = select if not isinstance(select, np.ndarray) else fix(select)
    return n


@functools.lru_cache(maxsize=None)
def designs():
    from signals_amd.chain.ext import FIR
    d = dict(lp=FIR.lowpass(3000.0, RATE), hp=FIR.highpass(500.0, RATE), bp=FIR.bandpass(800.0, 4000.0, RATE), hil=FIR.hilbert(),
             short=FIR.lowpass(6000.0, RATE, taps=17, window='hamming'))
    d['bank'] = np.hstack([d['lp'], d['hp'], d['bp']])
    for h in d.values():
        assert np.abs(h).sum(axis=0).max() <= 4.0                             # G <= 4 for every design the graphs use
        h.setflags(write=False)
    return d


def gain_bound(*tables):
    return max(1.0, *(float(np.abs(h).sum(axis=0).max()) for h in tables))


def draw():
    rng = np.random.default_rng(17)
    th = rng.uniform(0, np.pi / 2, GV)
    return dict(hertz=rng.uniform(55, 1760, (1, GV)), phase=rng.uniform(0, 1, (1, GV)), cut=rng.uniform(200, 8000, (1, GV)),
                select=rng.uniform(-0.5, 3.5, (1, GV)), time=rng.uniform(0, 0.002, (1, GV)), pan=np.stack([np.cos(th), np.sin(th)]) / GV)


def graph(which, p):
    """(GPU node, oracle node, rendered width, G) of one voice shape"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    RF, RD = FR.oracle_node(), DR.oracle_node()
    D = designs()
    saw = lambda: mkosc('Sawtooth', p['hertz'], p['phase'])
    rsaw = lambda: R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase']))
    if which == 'fir_saw':                                                     # a bank of three, a column per voice
        return fir_node(saw(), D['bank'], p['select']), RF(rsaw(), R.Fixed(p['select']), D['bank']), GV, gain_bound(D['bank'])
    if which == 'swept_bank':                                                  # the column follows a block-rate LFO: per-block select rows
        def lfo():
            g = fx.Gain(); g.left = mkosc('Sine', [[40.0]], p['phase']); g.right = fix([[4.0]])
            m = fx.Mix(); m.left = g; m.right = fix([[2.0]]); m.mix = fix([[0.5]])     # 1 +- 2
            return m
        rlfo = R.Binary('Mix', R.Binary('Gain', R.Osc('Sine', R.Fixed([[40.0]]), R.Fixed(p['phase'])), R.Fixed([[4.0]])), R.Fixed([[2.0]]),
                        R.Fixed([[0.5]]))
        return fir_node(saw(), D['bank'], lfo()), RF(rsaw(), rlfo, D['bank']), GV, gain_bound(D['bank'])
    if which == 'lowpass_over':
        f = fx.LowPass(); f.input = fir_node(saw(), D['hp']); f.cutoff = fix(p['cut'])
        return f, R.Filter('lp', RF(rsaw(), None, D['hp']), R.Fixed(p['cut'])), GV, gain_bound(D['hp'])
    if which == 'over_lowpass':
        f = fx.LowPass(); f.input = saw(); f.cutoff = fix(p['cut'])
        return fir_node(f, D['bp']), RF(R.Filter('lp', rsaw(), R.Fixed(p['cut'])), None, D['bp']), GV, gain_bound(D['bp'])
    if which == 'twice':
        return (fir_node(fir_node(saw(), D['lp']), D['short']), RF(RF(rsaw(), None, D['lp']), None, D['short']), GV,
                gain_bound(D['lp'], D['short']))
    if which == 'over_delay':
        comb = np.array([[1.0, 0.5], [0.5, 0.25], [0.25, -0.25]])             # sum |g| = 1
        d = ext.Delay(); d.get_state().taps = comb; d.input = saw(); d.time = fix(p['time'])
        return fir_node(d, D['lp']), RF(RD(rsaw(), R.Fixed(p['time']), comb), None, D['lp']), GV, gain_bound(D['lp'])
    if which == 'shifter':
        # the single-sideband frequency shifter: 0.5 * (x[n - 50] * cos - hilbert(x)[n] * sin); Sine at phase 1/4 is cos, at 1/2 is -sin
        x = saw()
        d = ext.Delay(); d.input = x; d.time = fix([[50.0 / RATE]])
        a = fx.RingMod(); a.left = d; a.right = mkosc('Sine', [[SHIFT_HZ]], [[0.25]])
        b = fx.RingMod(); b.left = fir_node(x, D['hil']); b.right = mkosc('Sine', [[SHIFT_HZ]], [[0.5]])
        m = fx.Mix(); m.left = a; m.right = b; m.mix = fix([[0.5]])
        rx = rsaw()
        ra = R.Binary('RingMod', RD(rx, R.Fixed([[50.0 / RATE]])), R.Osc('Sine', R.Fixed([[SHIFT_HZ]]), R.Fixed([[0.25]])))
        rb = R.Binary('RingMod', RF(rx, None, D['hil']), R.Osc('Sine', R.Fixed([[SHIFT_HZ]]), R.Fixed([[0.5]])))
        return m, R.Binary('Mix', ra, rb, R.Fixed([[0.5]])), GV, gain_bound(D['hil'])
    if which == 'bus':
        b = ext.SumBus(); b.input = fir_node(saw(), D['lp']); b.get_state().gains = np.ascontiguousarray(p['pan'])
        return b, R.SumBus(RF(rsaw(), None, D['lp']), p['pan']), 2, gain_bound(D['lp'])
    raise KeyError(which)


GRAPHS = ('fir_saw', 'swept_bank', 'lowpass_over', 'over_lowpass', 'twice', 'over_delay', 'shifter', 'bus')
FUSED = ('fused', 'latency', 'cascade', 'steady', 'walk', 'biquad_bus', 'biquad_coldstart_env', 'voice_program')


def eager_rows(top, C, pos, N, blocks):
    """sequential eager pulls through a BlockDriver: the reference-shaped path"""
    from signals_amd.chain.driver import BlockDriver
    d = BlockDriver(RATE, N)
    d.get_state().channels = C
    d.input = top
    d.frame_position = pos
    rows = np.concatenate([d.pull(eager=True) for _ in range(blocks)])
    del d.input
    return rows


def batched_rows(top, C, pos, N, ks, **kw):
    return render_batches(top, C, pos, N, ks, names=True, **kw)[:2]


def bar_of(want, G):
    """the bar of one case, and the check that the float32 store's own rounding leaves three quarters of it"""
    peak = float(np.abs(want).max())
    bar = 1e-6 * G * max(1.0, peak)
    assert 2.0 ** -24 * peak < bar / 4, (peak, G)
    return bar


def check_routes(which, p, eager, want, G, pos, N, ks):
    """one kernel per node (fuse=False): bit-equal to the eager path; the default route: the same launches, so bit-equal too, but for
    the LowPass(Sawtooth) BEHIND a FIR, which it may render as one fused kernel; every route within the bar of the restatement chain.
    No fused kernel and no voice program takes the FIR itself on either route"""
    bar = bar_of(want, G)
    assert eager.dtype == np.float32 and maxerr(eager, want) <= bar, (which, N, maxerr(eager, want), bar)
    for kw in ({'fuse': False}, {}):
        got, names = batched_rows(graph(which, p)[0], want.shape[1], pos, N, ks, **kw)
        firs = {n for n in names if n.startswith('fir_taps[')}
        assert firs and (which != 'swept_bank' or firs == {'fir_taps[101,per-block]'}), names
        assert which != 'twice' or firs == {'fir_taps[101]', 'fir_taps[17]'}, names
        fused = {n for n in names if any(w in n for w in FUSED)}
        assert fused <= ({'fused_osc_biquad[Sawtooth,lp]'} if which == 'over_lowpass' and not kw else set()), (kw, names)
        assert got.dtype == np.float32 and maxerr(got, want) <= bar, (which, N, kw, maxerr(got, want), bar)
        if not fused:
            assert same(got, eager), (which, N, kw, maxerr(got, eager))


@pytest.mark.parametrize('which', GRAPHS)
def test_batched_equals_eager_and_both_meet_the_restatement(which):
    """from position 0, two batches of K = 3: the second continues the first (the tails path)"""
    from oracle import chain_ref as R
    p, N = draw(), 128
    top, ref, C, G = graph(which, p)
    want = R.render_stream(ref, 0, N, 2 * GK, C)
    eager = eager_rows(graph(which, p)[0], C, 0, N, 2 * GK)
    check_routes(which, p, eager, want, G, 0, N, (GK, GK))
    assert np.abs(want).max() > (0.005 if which == 'bus' else 0.1)            # (the graphs sound)


@pytest.mark.parametrize('which', GRAPHS)
def test_a_fresh_batch_at_position_4096_takes_the_own_history_path(which):
    """a fresh renderer and a fresh graph at 4096: history rows come from blocks rendered in front, not from tails"""
    from oracle import chain_ref as R
    p, N, pos = draw(), 256, 4096
    top, ref, C, G = graph(which, p)
    want = R.render_stream(ref, pos, N, GK, C)
    eager = eager_rows(graph(which, p)[0], C, pos, N, GK)
    check_routes(which, p, eager, want, G, pos, N, (GK,))


def test_short_blocks_over_an_impure_input_render_eagerly():
    """N = 64 with a filter in front: the batch refuses (the after-window cache decides what the next block reads), the driver falls
    back to the eager path and that meets the restatement chain"""
    from oracle import chain_ref as R
    from signals_amd.chain.driver import BlockDriver
    from signals_amd.engine import BatchRenderer, NotBatchable
    p, N = draw(), 64
    top, ref, C, G = graph('over_lowpass', p)
    with pytest.raises(NotBatchable, match='block size <= 100'):
        BatchRenderer(top, C, RATE).render(0, N, 3)
    d = BlockDriver(RATE, N)
    d.get_state().channels = C
    d.input = graph('over_lowpass', p)[0]
    got = d.render(4)                                                         # batched=True: falls back
    assert d._engine_ok is False
    want = R.render_stream(ref, 0, N, 4, C)
    assert got.shape == want.shape and maxerr(got, want) <= bar_of(want, G)
    assert same(got, eager_rows(graph('over_lowpass', p)[0], C, 0, N, 4))


@pytest.mark.parametrize('pos', [0, 37, 4096])
def test_one_frame_requests(pos):
    """frames == 1: float64 from the same kernel; in a control path the batch refuses with the reason and the eager path serves it"""
    from helpers import render
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    from signals_amd.engine import BatchRenderer, NotBatchable
    p, D = draw(), designs()
    RF = FR.oracle_node()
    got = render(fir_node(mkosc('Sawtooth', p['hertz'], p['phase']), D['bank'], p['select']), pos, 1, GV)
    ref = RF(R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase'])), R.Fixed(p['select']), D['bank'])
    want = R.render(ref, pos, 1, GV)
    assert got.shape == (1, GV) and got.dtype == np.float64
    assert maxerr(got, want) <= bar_of(want, gain_bound(D['bank']))           # (the context rows are the oscillator's stored float32 blocks)
    # the one-frame window: float32 context rows widened, the float64 frame itself: the reference over exactly those rows, bit for bit
    c0 = min(100, pos)
    rows = [f32(R.osc('Sawtooth', pos - c0, c0, RATE, p['hertz'], p['phase'])).astype(np.float64)] if c0 else []
    window = np.concatenate(rows + [R.osc('Sawtooth', pos, 1, RATE, p['hertz'], p['phase'])])
    assert same(got, FR.fir_block(window, c0, 1, p['select'], D['bank']))

    # a FIR in a cutoff's control path: Mix(FIR(Sine LFO), cutoffs)
    def voice():
        lfo = fir_node(mkosc('Sine', [[3.0]]), D['short'])
        hz = fx.Mix(); hz.left = lfo; hz.right = fix(p['cut']); hz.mix = fix([[0.001]])       # the cutoffs, moved by the smoothed LFO
        f = fx.LowPass(); f.input = mkosc('Sawtooth', p['hertz'], p['phase']); f.cutoff = hz
        return f
    with pytest.raises(NotBatchable, match='FIR in a control path: a FIR filter has no block-rate'):
        BatchRenderer(voice(), GV, RATE).render(pos, 256, 2)
    lfo_ref = RF(R.Osc('Sine', R.Fixed([[3.0]])), None, D['short'])
    vref = R.Filter('lp', R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase'])),
                    R.Binary('Mix', lfo_ref, R.Fixed(p['cut']), R.Fixed([[0.001]])))
    eager = eager_rows(voice(), GV, pos, 256, 2)
    assert maxerr(eager, R.render_stream(vref, pos, 256, 2, GV)) < 1e-6
