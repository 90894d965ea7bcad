"""The short multi-tap delay line on the GPU: sig_delay_taps against tests/delay_reference.py bit for bit, the eager node (BlockDriver,
eager pulls) against the batched engine (BatchRenderer) bit for bit, and both against a float64 chain of oracle.chain_ref plus
delay_reference.

Bars.  The formula has no transcendental and the library is built with contraction off, so the kernel's float64 output equals the
reference bit for bit (NaN where the reference has NaN) and its float32 output equals float32(reference) bit for bit: no tolerance.
The batched engine launches the same kernels on the same stored float32 rows as the eager path, so the two are bit-equal on every
graph here (none of them is taken by a fused kernel or a voice program; the test asserts that).  Against the float64 oracle chain
both are held to the project's 1e-6: the delay line is a convex combination of two input samples per tap, so it carries its input's
error times sum |g_u| (<= 1 for the tap sets used on these graphs) and adds one float32 rounding of a value within +-1.5.

Shapes.  V crosses a wave and a 64-voice tile (1, 3, 64, 70, 130); N in {16, 101, 128}, K in {1, 3}; positions 0, 37 (zero fill and
c0 < 100), 4096 and one hour; U in {1, 4, 16}; one launch of 3 x 128 = 384 rows crosses the 220-row tile at a row count that is no
multiple of it, inside a block.  The per-voice delays cycle through 0, integers, 98.999, 99, beyond 99, negative, +-inf and one NaN
voice.  The references are computed once per (V, N, K, position, U) and shared by the dtype combinations."""
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import dev, gpu_ready, render_batches
from helpers import HOUR, RATE, f32, fix, maxerr, mkosc
import delay_reference as DR

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


# the delays in frames: every voice takes the next one, so V = 1 takes 0 and V >= 14 all of them; the NaN goes to ONE voice
DELAYS = [0.0, 1.0, 98.999, 99.0, 37.0, 99.5, 1e5, -3.0, np.inf, -np.inf, 17.25, 2.0, 63.5, 0.001]


def times(rng, blocks, V, nan_voice=True):
    d = np.array([DELAYS[(v + 5 * b) % len(DELAYS)] for b in range(blocks) for v in range(V)]).reshape(blocks, V)
    d[:, 1::3] += rng.uniform(0, 1, d[:, 1::3].shape)                          # fractions on a third of the voices
    if nan_voice and V > 1:
        d[:, V // 2] = np.nan
    return d / RATE


def taps_set(U):
    rng = np.random.default_rng(U)
    taps = np.stack([rng.uniform(0, 1.2, U), rng.uniform(-1, 1, U)], axis=1)
    taps[0] = (1.0, 1.0)                                                       # the first tap reads d itself: every case of DELAYS as drawn
    if U >= 4:
        taps[1] = (0.0, 0.5)                                                   # a tap at no delay (and inf * 0 = NaN on the +-inf voices)
        taps[2] = (-1.0, 0.25)                                                 # a negative multiplier: clipped to 0
    return taps


@functools.lru_cache(maxsize=None)
def kernel_case(V, N, K, pos, U, per_block):
    """(window float32-representable float64, time rows, taps, float64 reference): computed once, read-only"""
    rng = np.random.default_rng(V * 1000 + N * 10 + K + pos % 1000 + U)
    c0 = min(100, pos)
    x = rng.uniform(-1.5, 1.5, (c0 + N * K, V)).astype(np.float32).astype(np.float64)
    x[rng.integers(0, x.shape[0], 3), rng.integers(0, V, 3)] = 0.0
    t = times(rng, K if per_block else 1, V)
    taps = taps_set(U)
    want = DR.delay(x, c0, N, t, RATE, taps, blocks=K)
    for a in (x, t, taps, want):
        a.setflags(write=False)
    return x, t, taps, want


@pytest.mark.parametrize('pos', [0, 37, 4096, HOUR])
@pytest.mark.parametrize('V', [1, 3, 64, 70, 130])
def test_delay_taps_matches_the_reference_bit_for_bit(V, pos):
    """every N, K, U, time form and dtype combination at one (V, position); outputs are padded and the padding must stay untouched"""
    from signals_amd import _native
    c0 = min(100, pos)
    for N in (16, 101, 128):
        for K in (1, 3):
            for U in (1, 4, 16):
                for per_block in (False, True):
                    x, t, taps, want = kernel_case(V, N, K, pos, U, per_block)
                    assert V == 1 or np.isnan(want[:, V // 2]).all()          # the NaN voice: every row of it
                    for t_in in (torch.float32, torch.float64):
                        for t_out, cast in ((torch.float64, lambda a: a), (torch.float32, f32)):
                            obuf = torch.zeros((N * K, V + 3), dtype=t_out, device='cuda:0')
                            _native.delay_taps(RATE, pos, N, K, dev(x, t_in), c0, dev(t), taps, obuf[:, :V])
                            assert not obuf[:, V:].any(), (V, pos, N, K, U)
                            assert same(obuf[:, :V].cpu().numpy(), cast(want)), (V, pos, N, K, U, per_block, t_in, t_out)


@pytest.mark.parametrize('N, K', [(220, 2), (221, 1), (110, 4)])
def test_blocks_that_end_on_the_staging_tile_bit_for_bit(N, K):
    """the 220-row staging tile's edge: a block that ends exactly on it (220 x 2: a tile per block), one row past it (221: a second tile
    of one row) and two blocks per tile (110 x 4) -- V on both sides of a wave, positions 0 (zero fill) and 4096, U = 4 with a time row
    per block, float32 in and out, and the float64 window's gather once per shape"""
    from signals_amd import _native
    assert N * K % 220 in (0, 1)                                               # SIG_DELAY_TILE_ROWS
    for V in (3, 70):
        for pos in (0, 4096):
            x, t, taps, want = kernel_case(V, N, K, pos, 4, True)
            c0 = min(100, pos)
            for t_in in (torch.float32,) + ((torch.float64,) if (V, pos) == (70, 4096) else ()):
                obuf = torch.zeros((N * K, V + 3), dtype=torch.float32, device='cuda:0')
                _native.delay_taps(RATE, pos, N, K, dev(x, t_in), c0, dev(t), taps, obuf[:, :V])
                assert not obuf[:, V:].any(), (V, pos, t_in)
                assert same(obuf[:, :V].cpu().numpy(), f32(want)), (V, pos, t_in)


def test_identity_shift_broadcast_input_and_unplugged_time():
    from signals_amd import _native
    rng = np.random.default_rng(21)
    V, N, K = 70, 128, 3
    x = rng.uniform(-1.5, 1.5, (100 + N * K, V)).astype(np.float32)
    out = torch.empty((N * K, V), dtype=torch.float32, device='cuda:0')
    one = np.array([[1.0, 1.0]])
    _native.delay_taps(RATE, 4096, N, K, dev(x, torch.float32), 100, None, one, out)              # time unplugged: the identity
    assert same(out.cpu().numpy(), x[100:])
    _native.delay_taps(RATE, 4096, N, K, dev(x, torch.float32), 100, dev([[0.0]]), one, out)
    assert same(out.cpu().numpy(), x[100:])
    for shift in (1, 25, 99):
        _native.delay_taps(100, 4096, N, K, dev(x, torch.float32), 100, dev([[shift / 100.0]]), one, out)   # t * rate = shift exactly
        assert same(out.cpu().numpy(), x[100 - shift:100 - shift + N * K]), shift
    _native.delay_taps(100, 50, N, K, dev(x[50:], torch.float32), 50, dev([[0.75]]), one, out)   # position 50, 75 frames back: zeros first
    assert same(out.cpu().numpy(), np.concatenate([np.zeros((25, V), np.float32), x[50:50 + N * K - 25]]))
    # a one-column input broadcast over the voices, per-voice time rows; a padded input
    t = times(rng, 1, V)
    for t_in in (torch.float32, torch.float64):
        _native.delay_taps(RATE, 4096, N, K, dev(x[:, :1], t_in), 100, dev(t), taps_set(4), out)
        assert same(out.cpu().numpy(), f32(DR.delay(x[:, :1].astype(np.float64), 100, N, t, RATE, taps_set(4), blocks=K)))
    xbuf = torch.zeros((100 + N * K, V + 5), dtype=torch.float32, device='cuda:0')
    xbuf[:, :V] = dev(x, torch.float32)
    _native.delay_taps(RATE, 4096, N, K, xbuf[:, :V], 100, dev(t), taps_set(16), out)
    assert same(out.cpu().numpy(), f32(DR.delay(x.astype(np.float64), 100, N, t, RATE, taps_set(16), blocks=K)))


def test_wrapper_refusals():
    from signals_amd import _native
    x = torch.zeros((100 + 256, 8), dtype=torch.float32, device='cuda:0')
    out = torch.zeros((256, 8), dtype=torch.float32, device='cuda:0')
    with pytest.raises(_native.NativeError, match='delay shapes'):
        _native.delay_taps(RATE, 4096, 256, 1, x[:300], 100, None, np.array([[1.0, 1.0]]), out)
    with pytest.raises(_native.NativeError, match='hipError_t 1'):
        _native.delay_taps(RATE, 37, 256, 1, x, 100, None, np.array([[1.0, 1.0]]), out)            # c0 inconsistent with the position
    with pytest.raises(_native.NativeError, match='delay taps'):
        _native.delay_taps(RATE, 4096, 256, 1, x, 100, None, np.zeros((17, 2)), out)
    assert not out.any()


# ---------------------------------------------------------------------------------------------- graphs: eager against batched against the oracle
GV, GK = 70, 3
LFO_HZ = 2.3


def delay_node(input_, time, taps=None):
    from signals_amd.chain import ext
    d = ext.Delay()
    if taps is not None:
        d.get_state().taps = np.asarray(taps, dtype=np.float64)
    d.input = input_
    d.time = time if not isinstance(time, np.ndarray) else fix(time)
    return d


def draw():
    rng = np.random.default_rng(17)
    th = rng.uniform(0, np.pi / 2, GV)
    return dict(hertz=rng.uniform(55, 1760, (1, GV)), phase=rng.uniform(0, 1, (1, GV)), cut=rng.uniform(200, 8000, (1, GV)),
                time=rng.uniform(0, 0.002, (1, GV)), time2=rng.uniform(0, 0.002, (1, GV)), pan=np.stack([np.cos(th), np.sin(th)]) / GV)


COMB = np.array([[1.0, 0.5], [0.5, 0.25], [0.25, -0.25]])                     # sum |g| = 1


def graph(which, p):
    """(GPU node, oracle node, rendered width) of one voice shape"""
    from oracle import chain_ref as R
    from signals_amd.chain import ext, fx
    RD = DR.oracle_node()
    saw = lambda: mkosc('Sawtooth', p['hertz'], p['phase'])
    rsaw = lambda: R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase']))

    def flanger():
        # Mix(Saw, Delay(Saw, time = a Sine LFO scaled into 0 .. 1.5 ms)): time = 0.5 * (0.00075 * sine) + 0.5 * 0.0015 ... per voice offset
        lfo = fx.Gain(); lfo.left = mkosc('Sine', [[LFO_HZ]], p['phase']); lfo.right = fix([[0.0015]])
        time = fx.Mix(); time.left = lfo; time.right = fix([[0.0015]]); time.mix = fix([[0.5]])
        dry = saw()
        mix = fx.Mix(); mix.left = dry; mix.right = delay_node(dry, time); mix.mix = fix([[0.5]])
        rtime = R.Binary('Mix', R.Binary('Gain', R.Osc('Sine', R.Fixed([[LFO_HZ]]), R.Fixed(p['phase'])), R.Fixed([[0.0015]])),
                         R.Fixed([[0.0015]]), R.Fixed([[0.5]]))
        rdry = rsaw()
        return mix, R.Binary('Mix', rdry, RD(rdry, rtime), R.Fixed([[0.5]]))
    if which == 'flanger':
        return (*flanger(), GV)
    if which == 'flanger_bus':
        top, ref = flanger()
        b = ext.SumBus(); b.input = top; b.get_state().gains = np.ascontiguousarray(p['pan'])
        return b, R.SumBus(ref, p['pan']), 2
    if which == 'lowpass_over':
        f = fx.LowPass(); f.input = delay_node(saw(), p['time'], COMB); f.cutoff = fix(p['cut'])
        return f, R.Filter('lp', RD(rsaw(), R.Fixed(p['time']), COMB), R.Fixed(p['cut'])), GV
    if which == 'over_lowpass':
        f = fx.LowPass(); f.input = saw(); f.cutoff = fix(p['cut'])
        return delay_node(f, p['time'], COMB), RD(R.Filter('lp', rsaw(), R.Fixed(p['cut'])), R.Fixed(p['time']), COMB), GV
    if which == 'narrow_swept':
        # ONE column: a Sine whose hertz follows a block-rate LFO (440 +- 60 Hz), into a Delay with per-voice time rows
        def hertz():
            g = fx.Gain(); g.left = mkosc('Triangle', [[7.0]]); g.right = fix([[120.0]])
            m = fx.Mix(); m.left = g; m.right = fix([[880.0]]); m.mix = fix([[0.5]])
            return m
        from signals_amd.chain import osc
        src = osc.Sine(); src.hertz = hertz()
        rhertz = R.Binary('Mix', R.Binary('Gain', R.Osc('Triangle', R.Fixed([[7.0]])), R.Fixed([[120.0]])), R.Fixed([[880.0]]), R.Fixed([[0.5]]))
        return delay_node(src, p['time'], COMB), RD(R.Osc('Sine', rhertz), R.Fixed(p['time']), COMB), GV
    if which == 'twice':
        return (delay_node(delay_node(saw(), p['time']), p['time2'], COMB),
                RD(RD(rsaw(), R.Fixed(p['time'])), R.Fixed(p['time2']), COMB), GV)
    raise KeyError(which)


GRAPHS = ('flanger', 'lowpass_over', 'over_lowpass', 'twice', 'flanger_bus')
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


def check_routes(which, p, eager, want, pos, N, ks):
    """one kernel per node (fuse=False): bit-equal to the eager path; the default route: the same launches, so bit-equal too, but
    for the LowPass(Sawtooth) BEHIND a Delay, which it may render as one fused kernel -- then the project's 1e-6; both within 1e-6
    of the oracle.  No fused kernel and no voice program takes the Delay itself on either route"""
    assert eager.dtype == np.float32 and maxerr(eager, want) < 1e-6, (which, N, maxerr(eager, want))
    for kw in ({'fuse': False}, {}):
        got, names = batched_rows(graph(which, p)[0], want.shape[1], pos, N, ks, **kw)
        delays = {n for n in names if n.startswith('delay_taps[')}
        assert delays and (not which.startswith('flanger') or delays == {'delay_taps[1,per-block]'}), names
        fused = {n for n in names if any(w in n for w in FUSED)}
        assert fused <= ({'fused_osc_biquad[Sawtooth,lp]'} if which == 'over_lowpass' and not kw else set()), (kw, names)
        assert got.dtype == np.float32 and maxerr(got, want) < 1e-6, (which, N, kw, maxerr(got, want))
        if not fused:
            assert same(got, eager), (which, N, kw, maxerr(got, eager))


@pytest.mark.parametrize('N', [128, 256])
@pytest.mark.parametrize('which', GRAPHS)
def test_batched_equals_eager_and_both_meet_the_oracle(which, N):
    """from position 0, two batches of K = 3: the second continues the first (the tails path)"""
    from oracle import chain_ref as R
    p = draw()
    top, ref, C = graph(which, p)
    want = R.render_stream(ref, 0, N, 2 * GK, C)
    eager = eager_rows(graph(which, p)[0], C, 0, N, 2 * GK)
    check_routes(which, p, eager, want, 0, N, (GK, GK))
    assert np.abs(want).max() > (0.005 if which == 'flanger_bus' else 0.3)   # (the graphs sound)


@pytest.mark.parametrize('which', GRAPHS)
def test_a_fresh_batch_at_position_4096_takes_the_own_history_path(which):
    """a fresh renderer and a fresh graph at 4096: history rows come from blocks rendered in front, not from tails"""
    from oracle import chain_ref as R
    p, N, pos = draw(), 256, 4096
    top, ref, C = graph(which, p)
    want = R.render_stream(ref, pos, N, GK, C)
    eager = eager_rows(graph(which, p)[0], C, pos, N, GK)
    check_routes(which, p, eager, want, pos, N, (GK,))


@pytest.mark.parametrize('pos,N,ks', [(0, 128, (3, 3)), (4096, 256, (3,)), (37, 128, (2, 1))])
def test_a_one_column_swept_input_is_evaluated_afresh_for_every_context_request(pos, N, ks):
    """Delay(Sine with its hertz on a block-rate LFO, ONE column; time per voice), the reduced form of the random graphs that found it
    (tests/test_gpu_random_ext_graphs.py, seed 0 among 17).  The block cache files a reply under the reply's own shape, so a one-column
    reply never serves a later request of the asked width: the eager path (and the oracle) evaluates the Delay's `before` request
    [p - 100, p) afresh, hertz read at p - 100, where the batched engine took the last rows of the block in front, hertz read at p - N:
    off by 1e-2 from the second block of a batch on.  Continuing batches, a fresh start mid-stream and one with fewer than 100 rows"""
    from oracle import chain_ref as R
    p = draw()
    top, ref, C = graph('narrow_swept', p)
    want = R.render_stream(ref, pos, N, sum(ks), C)
    eager = eager_rows(graph('narrow_swept', p)[0], C, pos, N, sum(ks))
    check_routes('narrow_swept', p, eager, want, pos, N, ks)
    # not vacuous: the second block's context rows with hertz read at their own position, and as the block in front holds them
    hertz = graph('narrow_swept', p)[1].inputs['input'].inputs['hertz']
    first = pos + N - 100
    fresh = R.osc('Sine', first, 100, RATE, R.render(hertz, first, 1, 1))
    stale = R.osc('Sine', first, 100, RATE, R.render(hertz, pos, 1, 1))
    assert maxerr(fresh, stale) > 1e-3


def test_short_blocks_over_an_impure_input_render_eagerly():
    """N = 64 with a filter in front: the batch refuses (the after-window cache decides what the next block reads), the driver falls
    back to the eager path and that meets the oracle"""
    from oracle import chain_ref as R
    from signals_amd.chain.driver import BlockDriver
    from signals_amd.engine import BatchRenderer, NotBatchable
    p, N = draw(), 64
    top, ref, C = graph('over_lowpass', p)
    with pytest.raises(NotBatchable, match='block size <= 100'):
        BatchRenderer(top, C, RATE).render(0, N, 3)
    d = BlockDriver(RATE, N)
    d.get_state().channels = C
    d.input = graph('over_lowpass', p)[0]
    got = d.render(4)                                                         # batched=True: falls back
    assert d._engine_ok is False
    want = R.render_stream(ref, 0, N, 4, C)
    assert got.shape == want.shape and maxerr(got, want) < 1e-6
    assert same(got, eager_rows(graph('over_lowpass', p)[0], C, 0, N, 4))


@pytest.mark.parametrize('pos', [0, 37, 4096])
def test_one_frame_requests(pos):
    """frames == 1: float64 from the same kernel; in a control path the batch refuses with the reason and the eager path serves it"""
    from helpers import render
    from oracle import chain_ref as R
    from signals_amd.chain import fx
    from signals_amd.engine import BatchRenderer, NotBatchable
    p = draw()
    RD = DR.oracle_node()
    got = render(delay_node(mkosc('Sawtooth', p['hertz'], p['phase']), p['time'], COMB), pos, 1, GV)
    ref = RD(R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase'])), R.Fixed(p['time']), COMB)
    want = R.render(ref, pos, 1, GV)
    assert got.shape == (1, GV) and got.dtype == np.float64
    assert maxerr(got, want) < 1e-6                                           # (the context rows are the oscillator's stored float32 blocks)
    # the one-frame window: float32 context rows widened, the float64 frame itself: the reference over exactly those rows, bit for bit
    c0 = min(100, pos)
    rows = [f32(R.osc('Sawtooth', pos - c0, c0, RATE, p['hertz'], p['phase'])).astype(np.float64)] if c0 else []
    window = np.concatenate(rows + [R.osc('Sawtooth', pos, 1, RATE, p['hertz'], p['phase'])])
    assert same(got, DR.delay_block(window, c0, 1, p['time'], RATE, COMB))
    # a Delay in a cutoff's control path: Mix(Delay(Sine LFO), cutoffs)
    def voice():
        lfo = delay_node(mkosc('Sine', [[3.0]]), np.array([[0.001]]))
        hz = fx.Mix(); hz.left = lfo; hz.right = fix(p['cut']); hz.mix = fix([[0.001]])       # the cutoffs, moved by the delayed LFO
        f = fx.LowPass(); f.input = mkosc('Sawtooth', p['hertz'], p['phase']); f.cutoff = hz
        return f
    with pytest.raises(NotBatchable, match='Delay in a control path: a delay line has no block-rate'):
        BatchRenderer(voice(), GV, RATE).render(pos, 256, 2)
    lfo_ref = RD(R.Osc('Sine', R.Fixed([[3.0]])), R.Fixed([[0.001]]))
    vref = R.Filter('lp', R.Osc('Sawtooth', R.Fixed(p['hertz']), R.Fixed(p['phase'])),
                    R.Binary('Mix', lfo_ref, R.Fixed(p['cut']), R.Fixed([[0.001]])))
    eager = eager_rows(voice(), GV, pos, 256, 2)
    assert maxerr(eager, R.render_stream(vref, pos, 256, 2, GV)) < 1e-6
